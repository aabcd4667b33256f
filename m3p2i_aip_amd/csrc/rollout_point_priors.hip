// rollout_point_priors.hip -- the fused rollout of a planner handle with PRIOR SAMPLES (m3_set_prior_samples): a few of the K
// samples take the caller's control sequences verbatim (clamped) instead of clamp(mean + noise).  The twins of the run-time-scene
// builds of the general instance (k_rollout_point<true, -1, PointSceneRT, PointCostWeights> and its occ<2> / occ<3> builds,
// rollout_point.hip) and of their per-sample-arena twins (rollout_point_rollout_scenes.hip): the same body
// (rollout_point_kernel.hpp) with PR = PriorSamples, always weighted, on PointSceneRT.  rows is wave-uniform: null -- every lane
// rolls out in the handle's single scene; else the handle's table of per-sample arenas (point_scene_rows.hpp), so priors and an
// arena per sample work together without a second family.  A translation unit of its own: every kernel that was in the library
// keeps its code.
#include "rollout_point_kernel.hpp"
#include "point_scene_rows.hpp"

namespace m3 {

// the body's own guard and its slot -> sample mapping, in front of the row's loads: false for a lane without a sample
__device__ __forceinline__ bool prior_lane_sample(const RolloutArgs& a, int& i) {
    const int slot = blockIdx.x * a.lanes + threadIdx.x;
    if ((int)threadIdx.x >= a.lanes || slot >= a.Kl) return false;
    i = a.order ? a.order[slot] : slot;
    return true;
}

template <bool LONE>
__device__ __forceinline__ void rollout_point_priors(const RolloutArgs& a, const PointSceneRT& uni, const float* rows,
                                                     const PointCostWeights& wt, const int* prior_slot, const float* prior_tab) {
    int i;
    if (!prior_lane_sample(a, i)) return;
    const PriorSamples pr = {prior_slot, prior_tab};
    // (one body for both: the wave-uniform test only decides where the lane's copy of the arena comes from)
    PointSceneRT sc = uni;
    if (rows) sc = point_scene_row_load(uni, rows, a.Kl, i);
    rollout_point_body<true, -1, LONE, true, PointSceneRT, PriorSamples>(a, sc, &wt, pr);
}

// uni: the handle's scene_rt (rows != null: read for its uniform members only); rows: null or [POINT_SCENE_ROW_WORDS][a.Kl];
// prior_slot: [a.Kl]; prior_tab: [M3_MAX_PRIOR_SAMPLES][a.T][2]
__global__ __launch_bounds__(64) void k_rollout_point_pr(const RolloutArgs a, const PointSceneRT uni,
                                                         const float* __restrict__ rows, const PointCostWeights wt,
                                                         const int* __restrict__ prior_slot, const float* __restrict__ prior_tab) {
    rollout_point_priors<true>(a, uni, rows, wt, prior_slot, prior_tab);
}
template <int OCC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(OCC, OCC))) void k_rollout_point_pr_occ(
    const RolloutArgs a, const PointSceneRT uni, const float* __restrict__ rows, const PointCostWeights wt,
    const int* __restrict__ prior_slot, const float* __restrict__ prior_tab) {
    rollout_point_priors<false>(a, uni, rows, wt, prior_slot, prior_tab);
}

// the builds by the number of wavefronts, as for every other instance (rollout_point_build; no _ref build on PointSceneRT)
void launch_rollout_point_pr(const RolloutArgs& a, const PointSceneRT& uni, const float* rows, const PointCostWeights& wt,
                             const int* prior_slot, const float* prior_tab, int blocks, hipStream_t s) {
    const dim3 grid(blocks), wg(64);
    switch (rollout_point_build(blocks, false)) {
        case BUILD_OCC3: hipLaunchKernelGGL(k_rollout_point_pr_occ<3>, grid, wg, 0, s, a, uni, rows, wt, prior_slot, prior_tab); break;
        case BUILD_OCC2: hipLaunchKernelGGL(k_rollout_point_pr_occ<2>, grid, wg, 0, s, a, uni, rows, wt, prior_slot, prior_tab); break;
        default: hipLaunchKernelGGL(k_rollout_point_pr, grid, wg, 0, s, a, uni, rows, wt, prior_slot, prior_tab); break;
    }
}

}  // namespace m3
