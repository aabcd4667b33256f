// sample_groups.hpp -- SAMPLE GROUPS (m3_set_sample_groups): a partition of a planner's samples into groups
// whose members roll the same control sequence out in different models, and the aggregation of a group's costs into one number.
// Host only, plain C++, includes nothing of the library: the one owner of the conditions under which a handle or a partition is
// refused (enumerators and texts), of the table the kernel reads (sample_groups.hip) and of the aggregate's arithmetic, restated
// here over the same compare-exchange network and the same summation tree.  m3_api.hip fills SampleGroupsInput from the handle
// and maps a refusal to its code; tests/native/sample_groups_host.cpp compiles this header on its own.
//
// THE ARITHMETIC (a spec, pinned bit for bit):
//   * a group's member costs are sorted in DESCENDING order c(0) >= c(1) >= ..., the 16-lane row padded with -inf.  The order is
//     the total order of the binary32 encodings (sample_group_key: -0.0 sorts below +0.0), so the result is a function of the
//     multiset of member costs, never of the member order;
//   * v(i) = c(i) for i < j, 0 otherwise, with j = max(1, ceil(worst_frac * M_g)) for a group of M_g members (worst_frac is a
//     binary32 value, the product and the ceiling are taken in binary64);
//   * the aggregate is SUM16(v) / (float)j: the fixed pairwise tree of panda_dyn.hpp ("SUM16"), ((v0+v1)+(v2+v3)) + ..., in
//     binary32, then one binary32 division;
//   * a NaN member makes the aggregate the canonical quiet NaN (0x7fc00000), decided ahead of the sort.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace m3 {

constexpr int SAMPLE_GROUP_LANES = 16;      // a group is a DPP row: at most this many members
constexpr int SAMPLE_GROUP_MIN = 2;
constexpr uint32_t SAMPLE_GROUP_NAN_BITS = 0x7fc00000u;

// ---- refusals: one enumerator and one text per condition -----------------------------------------------------------------------
enum SampleGroupRefusal {
    SAMPLE_GROUPS_OK = 0,
    // M3_ERR_UNSUPPORTED: the handle
    SAMPLE_GROUPS_SHARDED,
    SAMPLE_GROUPS_SIM_ONLY,
    SAMPLE_GROUPS_NOISE_BY_INDEX,     // mode_simple or sampling_random
    SAMPLE_GROUPS_HAS_PRIORS,
    // M3_ERR_BAD_ARG: the partition
    SAMPLE_GROUPS_NULL,
    SAMPLE_GROUPS_WRONG_N,
    SAMPLE_GROUPS_WORST_FRAC,
    SAMPLE_GROUPS_ID_RANGE,
    SAMPLE_GROUPS_SPECIAL_NULL_ACTION,
    SAMPLE_GROUPS_SPECIAL_BEST,
    SAMPLE_GROUPS_SINGLETON,
    SAMPLE_GROUPS_TOO_LARGE,
    SAMPLE_GROUPS_STRADDLE
};
constexpr bool sample_groups_refusal_is_unsupported(SampleGroupRefusal r) { return r >= SAMPLE_GROUPS_SHARDED && r <= SAMPLE_GROUPS_HAS_PRIORS; }

// what the decision reads of the handle
struct SampleGroupsInput {
    int K_local, K_global;
    bool multi_modal, mode_simple, sampling_random, sim_only;
    bool priors_on;      // prior samples or a prior controller, of either environment
};

// a refusal and what its text names: the sample, the group id, the group's size
struct SampleGroupFault {
    SampleGroupRefusal r = SAMPLE_GROUPS_OK;
    int k = -1, id = -1, size = 0, n = 0;
    float worst_frac = 0.0f;
};

inline std::string sample_groups_refusal_text(const SampleGroupFault& f, const SampleGroupsInput& in) {
    const std::string who = "m3_set_sample_groups: ";
    const std::string grp = "group " + std::to_string(f.id);
    switch (f.r) {
        case SAMPLE_GROUPS_OK: return "";
        case SAMPLE_GROUPS_SHARDED: return who + "sharded handle (K_local != K_global)";
        case SAMPLE_GROUPS_SIM_ONLY: return who + "planner handles only (the handle was created sim_only)";
        case SAMPLE_GROUPS_NOISE_BY_INDEX:
            return who + "mode_simple / sampling_random handle: its noise is a function of the sample index, so the members of a group cannot share a control sequence";
        case SAMPLE_GROUPS_HAS_PRIORS:
            return who + "the handle has prior samples or a prior controller (m3_set_prior_samples, m3_set_panda_prior_samples, m3_set_prior_controller)";
        case SAMPLE_GROUPS_NULL: return who + "null argument";
        case SAMPLE_GROUPS_WRONG_N: return who + "n is " + std::to_string(f.n) + ", must be K_local = " + std::to_string(in.K_local);
        case SAMPLE_GROUPS_WORST_FRAC: return who + "worst_frac must be in (0, 1]";
        case SAMPLE_GROUPS_ID_RANGE:
            return who + "sample " + std::to_string(f.k) + ": group id " + std::to_string(f.id) + " is outside -1 .. K - 1 = " + std::to_string(in.K_local - 1);
        case SAMPLE_GROUPS_SPECIAL_NULL_ACTION:
            return who + "sample " + std::to_string(f.k) + " is the zero-noise / null-action sample K - 1: it must be -1 (its control is no row of the noise table)";
        case SAMPLE_GROUPS_SPECIAL_BEST:
            return who + "sample " + std::to_string(f.k) + " is a best-trajectory sample of the multi-modal planner (0 and K/2): it must be -1";
        case SAMPLE_GROUPS_SINGLETON: return who + grp + " has 1 member (sample " + std::to_string(f.k) + "): a group has 2 .. 16 members, -1 leaves a sample on its own";
        case SAMPLE_GROUPS_TOO_LARGE: return who + grp + " has " + std::to_string(f.size) + " members: a group has 2 .. 16 members";
        case SAMPLE_GROUPS_STRADDLE:
            return who + grp + " has members in both halves of a multi-modal planner (sample " + std::to_string(f.k) + " and K/2 = " +
                   std::to_string(in.K_local / 2) + "): the halves have different means";
    }
    return "";
}

// the texts of the other entry points' refusals of a handle that has groups
constexpr const char* SAMPLE_GROUPS_UNBATCHED = "it has sample groups (m3_set_sample_groups), which only m3_rollout / m3_command run";
constexpr const char* SAMPLE_GROUPS_REFUSE_PRIORS = ": the handle has sample groups (m3_set_sample_groups), whose members share the noise table's rows";

// j of a group of `size` members: max(1, ceil(worst_frac * size)), at most size
inline int sample_group_worst_j(float worst_frac, int size) {
    int j = (int)std::ceil((double)worst_frac * (double)size);
    if (j < 1) j = 1;
    if (j > size) j = size;
    return j;
}

// ---- the table: what the kernel reads, in the order of the device block ------------------------------------------------------
// member[g][16]: the samples of group g in ascending order, padded with -1 | worst_j[g] | ungrouped[n_ungrouped].  Groups are
// numbered by their smallest member.  dense[k]: the row of sample k, -1 for a sample on its own.
struct SampleGroupTable {
    int n_groups = 0, n_ungrouped = 0;
    std::vector<int> member, worst_j, ungrouped, dense;
};
// ints of the device block of a handle of K samples, whatever the partition: K/2 rows at the most
constexpr size_t sample_group_table_ints(int K) { return (size_t)(K / 2) * SAMPLE_GROUP_LANES + (size_t)(K / 2) + (size_t)K; }

// the handle alone (nothing of the arguments is read)
inline SampleGroupRefusal sample_groups_handle_refusal(const SampleGroupsInput& in) {
    if (in.K_local != in.K_global) return SAMPLE_GROUPS_SHARDED;
    if (in.sim_only) return SAMPLE_GROUPS_SIM_ONLY;
    if (in.mode_simple || in.sampling_random) return SAMPLE_GROUPS_NOISE_BY_INDEX;
    if (in.priors_on) return SAMPLE_GROUPS_HAS_PRIORS;
    return SAMPLE_GROUPS_OK;
}

// validates everything, then builds the table; on a refusal `out` is left as it was
inline SampleGroupFault sample_groups_build(const SampleGroupsInput& in, const int* group_of, int n, float worst_frac, SampleGroupTable& out) {
    SampleGroupFault f;
    f.n = n; f.worst_frac = worst_frac;
    if ((f.r = sample_groups_handle_refusal(in)) != SAMPLE_GROUPS_OK) return f;
    const int K = in.K_local;
    if (!group_of) { f.r = SAMPLE_GROUPS_NULL; return f; }
    if (n != K) { f.r = SAMPLE_GROUPS_WRONG_N; return f; }
    if (!(worst_frac > 0.0f && worst_frac <= 1.0f)) { f.r = SAMPLE_GROUPS_WORST_FRAC; return f; }
    std::vector<int> count((size_t)K, 0), first((size_t)K, -1);
    for (int k = 0; k < K; ++k) {
        const int id = group_of[k];
        f.k = k; f.id = id;
        if (id < -1 || id >= K) { f.r = SAMPLE_GROUPS_ID_RANGE; return f; }
        if (id < 0) continue;
        if (k == K - 1) { f.r = SAMPLE_GROUPS_SPECIAL_NULL_ACTION; return f; }
        if (in.multi_modal && (k == 0 || k == K / 2)) { f.r = SAMPLE_GROUPS_SPECIAL_BEST; return f; }
        if (count[id]++ == 0) first[id] = k;
        // (ascending k: the first member below K/2 and this one at or above it)
        if (in.multi_modal && first[id] < K / 2 && k >= K / 2) { f.r = SAMPLE_GROUPS_STRADDLE; f.size = count[id]; return f; }
    }
    for (int k = 0; k < K; ++k) {   // in the order of the groups' smallest members
        const int id = group_of[k];
        if (id < 0 || first[id] != k) continue;
        f.k = k; f.id = id; f.size = count[id];
        if (count[id] < SAMPLE_GROUP_MIN) { f.r = SAMPLE_GROUPS_SINGLETON; return f; }
        if (count[id] > SAMPLE_GROUP_LANES) { f.r = SAMPLE_GROUPS_TOO_LARGE; return f; }
    }
    SampleGroupTable t;
    t.dense.assign((size_t)K, -1);
    std::vector<int> row_of((size_t)K, -1);
    for (int k = 0; k < K; ++k) {
        const int id = group_of[k];
        if (id < 0) { t.ungrouped.push_back(k); continue; }
        if (first[id] == k) {
            row_of[id] = t.n_groups++;
            t.member.insert(t.member.end(), SAMPLE_GROUP_LANES, -1);
            t.worst_j.push_back(sample_group_worst_j(worst_frac, count[id]));
            count[id] = 0;   // (from here on: the members placed so far)
        }
        const int g = row_of[id];
        t.member[(size_t)g * SAMPLE_GROUP_LANES + count[id]++] = k;
        t.dense[k] = g;
    }
    t.n_ungrouped = (int)t.ungrouped.size();
    out = std::move(t);
    return SampleGroupFault();
}

// ---- the aggregate, restated in plain C++ ------------------------------------------------------------------------------------
// the total order of the binary32 encodings (no NaN): a signed key that grows with the value, -0.0 below +0.0
inline int32_t sample_group_key(float c) {
    int32_t b;
    std::memcpy(&b, &c, sizeof(b));
    return b ^ ((b >> 31) & 0x7fffffff);
}
inline float sample_group_unkey(int32_t k) {
    const int32_t b = k ^ ((k >> 31) & 0x7fffffff);
    float c;
    std::memcpy(&c, &b, sizeof(c));
    return c;
}
// One step of the 16-wide bitonic network: lane l meets lane l ^ x; the lower lane of a pair keeps the larger key.
inline void sample_group_exchange(int32_t key[SAMPLE_GROUP_LANES], int x) {
    int32_t other[SAMPLE_GROUP_LANES];
    for (int l = 0; l < SAMPLE_GROUP_LANES; ++l) other[l] = key[l ^ x];
    for (int l = 0; l < SAMPLE_GROUP_LANES; ++l) {
        const bool lower = l < (l ^ x);
        const int32_t hi = key[l] > other[l] ? key[l] : other[l], lo = key[l] > other[l] ? other[l] : key[l];
        key[l] = lower ? hi : lo;
    }
}
// the network: for every block size 2, 4, 8, 16 the mirror within the block (xor 1, 3, 7, 15), then the halvings (xor 4, 2, 1)
inline void sample_group_sort_desc(int32_t key[SAMPLE_GROUP_LANES]) {
    for (int k = 2; k <= SAMPLE_GROUP_LANES; k *= 2) {
        sample_group_exchange(key, k - 1);
        for (int x = k / 4; x >= 1; x /= 2) sample_group_exchange(key, x);
    }
}
// SUM16 (panda_dyn.hpp): ((v0+v1)+(v2+v3)) + ... in binary32
inline float sample_group_sum16(const float v[SAMPLE_GROUP_LANES]) {
    float a[8], b[4];
    for (int i = 0; i < 8; ++i) a[i] = v[2 * i] + v[2 * i + 1];
    for (int i = 0; i < 4; ++i) b[i] = a[2 * i] + a[2 * i + 1];
    return (b[0] + b[1]) + (b[2] + b[3]);
}
// the aggregate of m member costs (2 .. 16) with the mean taken over the j worst
inline float sample_group_aggregate(const float* cost, int m, int j) {
    for (int i = 0; i < m; ++i)
        if (std::isnan(cost[i])) {
            float q;
            std::memcpy(&q, &SAMPLE_GROUP_NAN_BITS, sizeof(q));
            return q;
        }
    int32_t key[SAMPLE_GROUP_LANES];
    for (int l = 0; l < SAMPLE_GROUP_LANES; ++l) key[l] = sample_group_key(l < m ? cost[l] : -std::numeric_limits<float>::infinity());
    sample_group_sort_desc(key);
    float v[SAMPLE_GROUP_LANES];
    for (int l = 0; l < SAMPLE_GROUP_LANES; ++l) v[l] = l < j ? sample_group_unkey(key[l]) : 0.0f;
    return sample_group_sum16(v) / (float)j;
}

}  // namespace m3
