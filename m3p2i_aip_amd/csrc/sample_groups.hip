// sample_groups.hip -- the aggregation of SAMPLE GROUPS (m3_set_sample_groups) on the device: one launch at
// the tail of m3_rollout, behind the last writer of M3_BUF_TRAJ_COST, that replaces the costs of a group's members by the mean of
// the group's j worst.  The arithmetic is sample_groups.hpp's (a host header: this file restates it lane by lane); a translation
// unit of its own: every kernel that was in the library keeps its code.
//
// One group per 16-lane DPP row, four per wavefront.  Lane l of row g reads member l's cost (padding: -inf), keeps it in the
// handle's block of raw costs, takes part in the row's descending bitonic sort and in SUM16, and writes the aggregate over its
// member's cost.  Behind the rows, one lane per sample that is on its own copies its cost into the raw block.  The groups are
// disjoint and a row reads its members only, ahead of its own writes (the aggregate depends on all sixteen loads): no lane reads
// a cost that another lane of the launch writes.
#include "m3_internal.hpp"
#include "panda_dyn.hpp"   // dpp_f and the DPP controls of SUM16

namespace m3 {

namespace {

constexpr int SG_BLOCK = 256;
constexpr int SG_ROWS_PER_BLOCK = SG_BLOCK / 16;

template <int CTRL> __device__ __forceinline__ int dpp_i(int v) { return __float_as_int(dpp_f<CTRL>(__int_as_float(v))); }

// the total order of the encodings (sample_groups.hpp: sample_group_key); its own inverse
__device__ __forceinline__ int sg_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

// lane l meets the lane the control names; lower: l is the lower lane of its pair and keeps the larger key
template <int CTRL> __device__ __forceinline__ int sg_exchange(int key, bool lower) {
    const int other = dpp_i<CTRL>(key);
    return lower ? max(key, other) : min(key, other);
}
// xor 4 as two controls: row_half_mirror (l -> 7 - l within eight) then the quad reversed (3 - l within four)
__device__ __forceinline__ int sg_exchange_xor4(int key, bool lower) {
    const int other = dpp_i<0x1B>(dpp_i<0x141>(key));
    return lower ? max(key, other) : min(key, other);
}

}  // namespace

__global__ __launch_bounds__(SG_BLOCK) void k_sample_groups(const int* __restrict__ tab, int n_groups, int n_ungrouped, int cap_groups,
                                                            int K, float* __restrict__ J, float* __restrict__ raw) {
    const int row_blocks = (n_groups + SG_ROWS_PER_BLOCK - 1) / SG_ROWS_PER_BLOCK;
    if ((int)blockIdx.x >= row_blocks) {
        // ---- a sample on its own: its raw cost is its cost ----
        const int i = ((int)blockIdx.x - row_blocks) * SG_BLOCK + (int)threadIdx.x;
        if (i < n_ungrouped) {
            const int k = tab[(size_t)cap_groups * 17 + i];
            if (k >= 0 && k < K) raw[k] = J[k];
        }
        return;
    }
    // ---- a group: all sixteen lanes of the row stay active through the exchanges (rows are live or idle as a whole) ----
    const int l = (int)threadIdx.x & 15;
    const int g = (int)blockIdx.x * SG_ROWS_PER_BLOCK + ((int)threadIdx.x >> 4);
    const bool live = g < n_groups;
    int m = live ? tab[(size_t)g * 16 + l] : -1;
    if (m >= K) m = -1;
    const int j = live ? tab[(size_t)cap_groups * 16 + g] : 1;
    const float c = m >= 0 ? J[m] : -INFINITY;
    if (m >= 0) raw[m] = c;
    // a NaN anywhere in the row, decided ahead of the sort
    const unsigned long long nan_lanes = __ballot(c != c);
    const bool row_nan = ((nan_lanes >> ((threadIdx.x & 63u) & 48u)) & 0xffffull) != 0;
    // the descending bitonic network (sample_groups.hpp: sample_group_sort_desc): per block size the mirror, then the halvings
    int key = sg_key(__float_as_int(c));
    key = sg_exchange<0xB1>(key, (l & 1) == 0);     // 2: xor 1
    key = sg_exchange<0x1B>(key, (l & 2) == 0);     // 4: xor 3 (the quad reversed)
    key = sg_exchange<0xB1>(key, (l & 1) == 0);
    key = sg_exchange<0x141>(key, (l & 4) == 0);    // 8: xor 7 (row_half_mirror)
    key = sg_exchange<0x4E>(key, (l & 2) == 0);
    key = sg_exchange<0xB1>(key, (l & 1) == 0);
    key = sg_exchange<0x140>(key, (l & 8) == 0);    // 16: xor 15 (row_mirror)
    key = sg_exchange_xor4(key, (l & 4) == 0);
    key = sg_exchange<0x4E>(key, (l & 2) == 0);
    key = sg_exchange<0xB1>(key, (l & 1) == 0);
    // SUM16 over the j worst, then the one division
    float v = l < j ? __int_as_float(sg_key(key)) : 0.0f;
    v = v + dpp_f<0xB1>(v);
    v = v + dpp_f<0x4E>(v);
    v = v + dpp_f<0x141>(v);
    v = v + dpp_f<0x140>(v);
    float agg = v / (float)j;
    if (row_nan) agg = __int_as_float(0x7fc00000);
    if (m >= 0) J[m] = agg;
}

void launch_sample_groups(const SampleGroupArgs& a, hipStream_t s) {
    const int row_blocks = (a.n_groups + SG_ROWS_PER_BLOCK - 1) / SG_ROWS_PER_BLOCK;
    const int copy_blocks = (a.n_ungrouped + SG_BLOCK - 1) / SG_BLOCK;
    if (row_blocks + copy_blocks == 0) return;
    hipLaunchKernelGGL(k_sample_groups, dim3(row_blocks + copy_blocks), dim3(SG_BLOCK), 0, s, a.tab, a.n_groups, a.n_ungrouped,
                       a.cap_groups, a.K, a.J, a.raw);
}

}  // namespace m3
