// rollout_point_priors_batch.hip -- batched command (m3_batch_command on a batch with the priors section,
// M3_BATCH_SECTION_POINT_PRIORS): one launch for a group of point_env planner handles with PRIOR SAMPLES that share K, T and lanes.
// blockIdx.y picks the handle's entry (BatchRolloutEntryPR, m3_internal.hpp; read-only): its arguments, its scene's uniform
// members, its weights, null or its OWN table of per-sample arenas, and its OWN slot map and table of priors -- the batch stores
// none of them, and handles with and without an arena per sample share a launch.  The body is the instantiation of the
// single-handle kernels (k_rollout_point_pr*, rollout_point_priors.hip), the build picked by the GROUP's wavefront count: same
// bits.  A translation unit of its own: every kernel that was in the library keeps its code.
#include "rollout_point_kernel.hpp"
#include "point_scene_rows.hpp"

namespace m3 {

// the body's own guard and its slot -> sample mapping, in front of the row's loads: false for a lane without a sample
__device__ __forceinline__ bool rollout_lane_sample(const RolloutArgs& a, int& i) {
    const int slot = blockIdx.x * a.lanes + threadIdx.x;
    if ((int)threadIdx.x >= a.lanes || slot >= a.Kl) return false;
    i = a.order ? a.order[slot] : slot;
    return true;
}

template <bool LONE>
__device__ __forceinline__ void rollout_point_priors_entry(const BatchRolloutEntryPR& e) {
    int i;
    if (!rollout_lane_sample(e.a, i)) return;
    const PriorSamples pr = {e.prior_slot, e.ctl.tab};
    // (one body for both: the wave-uniform test only decides where the lane's copy of the arena comes from)
    PointSceneRT sc = e.sc;
    if (e.rows) sc = point_scene_row_load(e.sc, e.rows, e.a.Kl, i);
    rollout_point_body<true, -1, LONE, true, PointSceneRT, PriorSamples>(e.a, sc, &e.wt, pr);
}

__global__ __launch_bounds__(64) void kb_rollout_point_pr(const BatchRolloutEntryPR* __restrict__ tab) {
    rollout_point_priors_entry<true>(tab[blockIdx.y]);
}
template <int OCC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(OCC, OCC))) void kb_rollout_point_pr_occ(
    const BatchRolloutEntryPR* __restrict__ tab) {
    rollout_point_priors_entry<false>(tab[blockIdx.y]);
}

// blocks: workgroups of ONE handle (all handles of the group have the same); n: handles
void launch_rollout_point_pr_batch(const BatchRolloutEntryPR* tab, int blocks, int n, hipStream_t s) {
    const dim3 grid(blocks, n), wg(64);
    switch (rollout_point_build(blocks * n, false)) {
        case BUILD_OCC3: hipLaunchKernelGGL(kb_rollout_point_pr_occ<3>, grid, wg, 0, s, tab); break;
        case BUILD_OCC2: hipLaunchKernelGGL(kb_rollout_point_pr_occ<2>, grid, wg, 0, s, tab); break;
        default: hipLaunchKernelGGL(kb_rollout_point_pr, grid, wg, 0, s, tab); break;
    }
}

}  // namespace m3
