// sample_groups_host.cpp -- csrc/sample_groups.hpp on the host (its own main; tests/test_sample_groups_cpu.py builds it with g++,
// plain and under -fsanitize=address,undefined).
//   (no argument)  walks the validation (every refusal with its code class and text; sizes 2, 3, 15, 16, 17; the specials; a group
//                  across the halves; worst_frac at 0, 1/16, 1 and above), the table's layout and j per group; proves the network
//                  a sorting network (all 2^16 inputs of zeros and ones: the 0-1 principle); holds the aggregate to a binary64
//                  evaluation within 6 * 2^-24 * sum|v_i| / j; and checks that every permutation of a group's members (all of them
//                  up to 7 members, 4000 shuffles per size above) gives the same bits.  Prints "<n> checks, 0 failures".
//   --emit         prints the fixture tests/golden/sample_groups_aggregate.json: costs (as bit patterns) and the expected bits.
//   --eval         reads lines "j m bits_0 ... bits_m-1" (hex) from standard input, prints the aggregate's bits, one per line.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../m3p2i_aip_amd/csrc/sample_groups.hpp"

using namespace m3;

static long long g_checks = 0, g_failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        ++g_checks;                                                               \
        if (!(cond)) {                                                            \
            ++g_failures;                                                         \
            std::fprintf(stderr, "line %d: %s: ", __LINE__, #cond);              \
            std::fprintf(stderr, __VA_ARGS__);                                    \
            std::fprintf(stderr, "\n");                                          \
        }                                                                         \
    } while (0)

static uint32_t bits_of(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }
static float float_of(uint32_t b) { float x; std::memcpy(&x, &b, 4); return x; }

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 16);
}
static float rnd_cost() {   // positive costs over a few decades, now and then a tie-prone round value
    const float u = (float)(rnd() & 0xffffff) / 16777216.0f;
    const int kind = (int)(rnd() % 8);
    if (kind == 0) return (float)(rnd() % 5);
    if (kind == 1) return -u * 3.0f;
    return u * (float)(1u << (rnd() % 12));
}

static SampleGroupsInput planner(int K, bool multi = false) { return {K, K, multi, false, false, false, false}; }

static SampleGroupFault build(const SampleGroupsInput& in, const std::vector<int>& g, float wf, SampleGroupTable& t) {
    return sample_groups_build(in, g.data(), (int)g.size(), wf, t);
}

// a refusal: its enumerator, its code class, and a text that names the entry point and carries `needle`
static void refused(const SampleGroupsInput& in, const std::vector<int>& g, float wf, SampleGroupRefusal want, bool unsupported,
                    const char* needle, int n_override = -1, bool null_arg = false) {
    SampleGroupTable t;
    t.n_groups = 77;   // (a refused build leaves the table as it was)
    const SampleGroupFault f = sample_groups_build(in, null_arg ? nullptr : g.data(), n_override >= 0 ? n_override : (int)g.size(), wf, t);
    const std::string text = sample_groups_refusal_text(f, in);
    CHECK(f.r == want, "refusal %d, expected %d (%s)", (int)f.r, (int)want, text.c_str());
    CHECK(sample_groups_refusal_is_unsupported(f.r) == unsupported, "code class of %d", (int)f.r);
    CHECK(text.rfind("m3_set_sample_groups: ", 0) == 0, "text does not name the entry point: %s", text.c_str());
    CHECK(text.find(needle) != std::string::npos, "text '%s' lacks '%s'", text.c_str(), needle);
    CHECK(t.n_groups == 77, "a refused build changed the table");
}

static void walk_validation() {
    const int K = 64;
    std::vector<int> none(K, -1);
    // ---- the handle ----
    { SampleGroupsInput in = planner(K); in.K_global = 2 * K; refused(in, none, 1.0f, SAMPLE_GROUPS_SHARDED, true, "sharded handle"); }
    { SampleGroupsInput in = planner(K); in.sim_only = true; refused(in, none, 1.0f, SAMPLE_GROUPS_SIM_ONLY, true, "sim_only"); }
    { SampleGroupsInput in = planner(K); in.mode_simple = true; refused(in, none, 1.0f, SAMPLE_GROUPS_NOISE_BY_INDEX, true, "function of the sample index"); }
    { SampleGroupsInput in = planner(K); in.sampling_random = true; refused(in, none, 1.0f, SAMPLE_GROUPS_NOISE_BY_INDEX, true, "sampling_random"); }
    { SampleGroupsInput in = planner(K); in.priors_on = true; refused(in, none, 1.0f, SAMPLE_GROUPS_HAS_PRIORS, true, "prior samples or a prior controller"); }
    // ---- the arguments ----
    refused(planner(K), none, 1.0f, SAMPLE_GROUPS_NULL, false, "null argument", -1, true);
    refused(planner(K), none, 1.0f, SAMPLE_GROUPS_WRONG_N, false, "n is 63, must be K_local = 64", K - 1);
    refused(planner(K), none, 1.0f, SAMPLE_GROUPS_WRONG_N, false, "n is 65", K + 1);
    std::vector<int> pair = none;
    pair[3] = pair[9] = 5;
    for (float wf : {0.0f, -0.5f, 1.0000001f, 2.0f, float_of(0x7fc00000u)})
        refused(planner(K), pair, wf, SAMPLE_GROUPS_WORST_FRAC, false, "worst_frac must be in (0, 1]");
    { std::vector<int> g = pair; g[20] = K; refused(planner(K), g, 1.0f, SAMPLE_GROUPS_ID_RANGE, false, "sample 20: group id 64 is outside -1 .. K - 1 = 63"); }
    { std::vector<int> g = pair; g[20] = -2; refused(planner(K), g, 1.0f, SAMPLE_GROUPS_ID_RANGE, false, "group id -2"); }
    { std::vector<int> g = pair; g[K - 1] = 5; refused(planner(K), g, 1.0f, SAMPLE_GROUPS_SPECIAL_NULL_ACTION, false, "sample 63 is the zero-noise / null-action sample"); }
    { std::vector<int> g = pair; g[0] = 5; refused(planner(K, true), g, 1.0f, SAMPLE_GROUPS_SPECIAL_BEST, false, "sample 0 is a best-trajectory sample"); }
    { std::vector<int> g = none; g[K / 2] = g[K / 2 + 1] = 1; refused(planner(K, true), g, 1.0f, SAMPLE_GROUPS_SPECIAL_BEST, false, "sample 32 is a best-trajectory sample"); }
    { std::vector<int> g = pair; g[40] = 7; refused(planner(K), g, 1.0f, SAMPLE_GROUPS_SINGLETON, false, "group 7 has 1 member (sample 40)"); }
    { std::vector<int> g = none; for (int k = 1; k <= 17; ++k) g[k] = 2; refused(planner(K), g, 1.0f, SAMPLE_GROUPS_TOO_LARGE, false, "group 2 has 17 members"); }
    { std::vector<int> g = none; g[10] = g[40] = 3; refused(planner(K, true), g, 1.0f, SAMPLE_GROUPS_STRADDLE, false, "both halves"); }
    // ---- what is taken ----
    {   // single mode: samples 0 and K/2 are ordinary samples, a group may span K/2
        std::vector<int> g = none; g[0] = g[K / 2] = g[40] = 9;
        SampleGroupTable t;
        CHECK(build(planner(K), g, 1.0f, t).r == SAMPLE_GROUPS_OK, "single mode refuses samples 0, K/2 in a group");
        CHECK(t.n_groups == 1 && t.n_ungrouped == K - 3, "single-mode group");
    }
    for (float wf : {0.0625f, 1.0f, 1e-30f, 0.5f}) {
        SampleGroupTable t;
        CHECK(build(planner(K), pair, wf, t).r == SAMPLE_GROUPS_OK, "worst_frac %g refused", (double)wf);
    }
    // sizes 2, 3, 15, 16 in one partition of K = 64 (ids out of order, members interleaved), multi-modal sides respected
    {
        const int K2 = 160;
        std::vector<int> g(K2, -1);
        const int sizes[4] = {2, 3, 15, 16}, ids[4] = {150, 0, 77, 3};
        // members of group i: every fourth sample from 1 + i on (interleaved, so rows are not runs of consecutive samples)
        for (int i = 0; i < 4; ++i)
            for (int m = 0; m < sizes[i]; ++m) g[1 + i + 4 * m] = ids[i];
        for (float wf : {0.0625f, 0.25f, 0.5f, 1.0f}) {
            SampleGroupTable t;
            const SampleGroupFault f = build(planner(K2), g, wf, t);
            CHECK(f.r == SAMPLE_GROUPS_OK, "sizes 2, 3, 15, 16: %s", sample_groups_refusal_text(f, planner(K2)).c_str());
            CHECK(t.n_groups == 4 && t.n_ungrouped == K2 - 36, "counts %d %d", t.n_groups, t.n_ungrouped);
            CHECK((int)t.member.size() == 4 * 16 && (int)t.worst_j.size() == 4 && (int)t.dense.size() == K2, "table sizes");
            for (int i = 0; i < 4; ++i) {   // rows in the order of the smallest members: 1, 2, 3, 4
                for (int l = 0; l < 16; ++l) {
                    const int want = l < sizes[i] ? 1 + i + 4 * l : -1;
                    CHECK(t.member[i * 16 + l] == want, "member[%d][%d] = %d, expected %d", i, l, t.member[i * 16 + l], want);
                    if (want >= 0) CHECK(t.dense[want] == i, "dense[%d]", want);
                }
                int j = (int)std::ceil((double)wf * sizes[i]);
                if (j < 1) j = 1;
                CHECK(t.worst_j[i] == j, "worst_j[%d] = %d at worst_frac %g, expected %d", i, t.worst_j[i], (double)wf, j);
            }
            int seen = 0;
            for (int k = 0; k < K2; ++k)
                if (g[k] < 0) { CHECK(t.ungrouped[seen] == k && t.dense[k] == -1, "ungrouped[%d]", seen); ++seen; }
        }
    }
    // j = max(1, ceil(worst_frac * M)) at the edges
    CHECK(sample_group_worst_j(0.0625f, 16) == 1 && sample_group_worst_j(0.0625f, 15) == 1 && sample_group_worst_j(0.0626f, 16) == 2, "j at 1/16");
    CHECK(sample_group_worst_j(1.0f, 16) == 16 && sample_group_worst_j(1.0f, 2) == 2 && sample_group_worst_j(0.25f, 4) == 1 &&
          sample_group_worst_j(0.25f, 8) == 2 && sample_group_worst_j(0.5f, 3) == 2 && sample_group_worst_j(1e-30f, 16) == 1, "j");
    CHECK(sample_group_table_ints(64) == 32 * 16 + 32 + 64, "table ints");
}

static void network_sorts() {
    // the 0-1 principle: a comparison network that sorts every sequence of zeros and ones sorts every sequence
    for (unsigned mask = 0; mask < 65536u; ++mask) {
        int32_t key[16];
        int ones = 0;
        for (int l = 0; l < 16; ++l) { key[l] = (mask >> l) & 1; ones += key[l]; }
        sample_group_sort_desc(key);
        bool ok = true;
        for (int l = 0; l < 16; ++l) ok = ok && key[l] == (l < ones ? 1 : 0);
        CHECK(ok, "the network leaves input %04x unsorted", mask);
    }
    // the key: monotone in the value, -0.0 below +0.0, its own inverse
    const float ladder[] = {-INFINITY, -3.5f, -1e-40f, -0.0f, 0.0f, 1e-40f, 1.0f, 3.5f, INFINITY};
    for (size_t i = 0; i + 1 < sizeof(ladder) / sizeof(float); ++i) CHECK(sample_group_key(ladder[i]) < sample_group_key(ladder[i + 1]), "key order at %zu", i);
    for (float x : ladder) CHECK(bits_of(sample_group_unkey(sample_group_key(x))) == bits_of(x), "key round trip");
}

static double aggregate_f64(const std::vector<float>& c, int j, double& sum_abs) {
    std::vector<float> s = c;
    std::sort(s.begin(), s.end(), [](float a, float b) { return a > b; });
    double sum = 0.0;
    sum_abs = 0.0;
    for (int i = 0; i < j; ++i) { sum += (double)s[i]; sum_abs += std::fabs((double)s[i]); }
    return sum / j;
}

static void aggregate_checks() {
    for (int m = 2; m <= 16; ++m)
        for (int rep = 0; rep < 300; ++rep) {
            std::vector<float> c(m);
            for (float& x : c) x = rnd_cost();
            if (rep % 7 == 0) c[rnd() % m] = c[rnd() % m];   // a tie
            for (int j : {1, (m + 1) / 2, m}) {
                const float a = sample_group_aggregate(c.data(), m, j);
                double sum_abs;
                const double ref = aggregate_f64(c, j, sum_abs);
                // tree depth 4 + one division + one rounding of slack
                const double bound = 6.0 * std::ldexp(1.0, -24) * sum_abs / j;
                CHECK(std::fabs((double)a - ref) <= bound, "m %d j %d: %.9g against %.17g, bound %.3g", m, j, (double)a, ref, bound);
                // every permutation (m <= 7) or 4000 / 300 shuffles: the same bits
                std::vector<float> p = c;
                if (m <= 7 && rep < 3) {
                    std::sort(p.begin(), p.end());
                    do {
                        CHECK(bits_of(sample_group_aggregate(p.data(), m, j)) == bits_of(a), "m %d j %d: a permutation changes the bits", m, j);
                    } while (std::next_permutation(p.begin(), p.end()));
                } else {
                    for (int s = 0; s < (rep == 0 ? 4000 : 4); ++s) {
                        for (int i = m - 1; i > 0; --i) std::swap(p[i], p[rnd() % (i + 1)]);
                        CHECK(bits_of(sample_group_aggregate(p.data(), m, j)) == bits_of(a), "m %d j %d: a shuffle changes the bits", m, j);
                    }
                }
            }
        }
    // the edges: +inf, all +inf, NaN, signed zeros, equal values
    const float inf = INFINITY, qnan = float_of(0x7fc00000u);
    { const float c[3] = {1.0f, inf, 2.0f}; CHECK(sample_group_aggregate(c, 3, 1) == inf && sample_group_aggregate(c, 3, 3) == inf, "+inf member"); }
    { const float c[4] = {inf, inf, inf, inf}; CHECK(sample_group_aggregate(c, 4, 4) == inf && sample_group_aggregate(c, 4, 2) == inf, "all +inf"); }
    { const float c[3] = {1.0f, float_of(0xffc12345u), 2.0f};
      for (int j = 1; j <= 3; ++j) CHECK(bits_of(sample_group_aggregate(c, 3, j)) == 0x7fc00000u, "NaN member, j %d", j); }
    { const float c[2] = {qnan, qnan}; CHECK(bits_of(sample_group_aggregate(c, 2, 1)) == 0x7fc00000u, "all NaN"); }
    { const float a[2] = {-0.0f, 0.0f}, b[2] = {0.0f, -0.0f};
      CHECK(bits_of(sample_group_aggregate(a, 2, 1)) == 0u && bits_of(sample_group_aggregate(b, 2, 1)) == 0u, "the maximum of -0, +0 is +0"); }
    for (int m : {2, 4, 8, 16}) {   // power-of-two groups of equal values: the mean is the value, bit for bit
        std::vector<float> c(m, 123.456f);
        CHECK(bits_of(sample_group_aggregate(c.data(), m, m)) == bits_of(123.456f), "mean of %d equal values", m);
    }
    { const float c[3] = {5.0f, 1.0f, 3.0f}; CHECK(sample_group_aggregate(c, 3, 2) == 4.0f && sample_group_aggregate(c, 3, 1) == 5.0f && sample_group_aggregate(c, 3, 3) == 3.0f, "5 1 3"); }
}

static void emit_fixture() {
    g_rng = 0x2545F4914F6CDD1Dull;
    std::printf("{\"about\": \"sample-group aggregates: member costs and the expected aggregate as binary32 bit patterns, printed by "
                "tests/native/sample_groups_host.cpp --emit\",\n \"cases\": [\n");
    bool first = true;
    auto emit = [&](const std::vector<float>& c, int j) {
        std::printf("%s  {\"j\": %d, \"costs\": [", first ? "" : ",\n", j);
        first = false;
        for (size_t i = 0; i < c.size(); ++i) std::printf("%s%" PRIu32, i ? ", " : "", bits_of(c[i]));
        std::printf("], \"expected\": %" PRIu32 "}", bits_of(sample_group_aggregate(c.data(), (int)c.size(), j)));
    };
    for (int m = 2; m <= 16; ++m)
        for (int rep = 0; rep < 4; ++rep) {
            std::vector<float> c(m);
            for (float& x : c) x = rnd_cost();
            if (rep == 3) c[0] = c[m - 1];
            for (int j : {1, (m + 1) / 2, m}) emit(c, j);
        }
    const float inf = INFINITY;
    emit({1.0f, inf, 2.0f}, 1); emit({1.0f, inf, 2.0f}, 3); emit({inf, inf, inf, inf}, 4); emit({inf, inf}, 1);
    emit({1.0f, float_of(0xffc12345u), 2.0f}, 2); emit({float_of(0x7fc00000u), 3.0f}, 1);
    emit({-0.0f, 0.0f}, 1); emit({0.0f, -0.0f}, 1); emit({-0.0f, 0.0f, -0.0f}, 3); emit({-1.5f, -2.5f, -0.25f}, 2);
    emit(std::vector<float>(16, 123.456f), 16); emit(std::vector<float>(3, 0.1f), 3);
    std::printf("\n ]}\n");
}

static int eval_stdin() {
    int j, m;
    while (std::scanf("%d %d", &j, &m) == 2) {
        if (m < 2 || m > 16 || j < 1 || j > m) return 2;
        float c[16];
        for (int i = 0; i < m; ++i) {
            uint32_t b;
            if (std::scanf("%" SCNx32, &b) != 1) return 2;
            c[i] = float_of(b);
        }
        std::printf("%08" PRIx32 "\n", bits_of(sample_group_aggregate(c, m, j)));
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--emit") == 0) { emit_fixture(); return 0; }
    if (argc > 1 && std::strcmp(argv[1], "--eval") == 0) return eval_stdin();
    walk_validation();
    network_sorts();
    aggregate_checks();
    std::printf("%lld checks, %lld failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
