// rollout_point_rollout_scenes.hip -- the fused rollout of a planner handle with one arena PER SAMPLE
// (m3_set_point_rollout_scenes): the per-row twins of the run-time-scene builds of the general instance (k_rollout_point<true, -1,
// PointSceneRT, PointCostWeights> and its occ<2> / occ<3> builds, rollout_point.hip).  The same body (rollout_point_kernel.hpp) on
// the same scene type, always weighted; each lane builds its PointSceneRT in registers from row i of the handle's table
// (point_scene_rows.hpp) -- i the sample's row of every per-sample buffer, not its wavefront slot.  A translation unit of its
// own, like its step-mode neighbour: every kernel that was in the library keeps its code.
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

// uni: the handle's scene_rt, read for its uniform members only; rows: [POINT_SCENE_ROW_WORDS][a.Kl]
__global__ __launch_bounds__(64) void k_rollout_point_sv(const RolloutArgs a, const PointSceneRT uni,
                                                         const float* __restrict__ rows, const PointCostWeights wt) {
    int i;
    if (!rollout_lane_sample(a, i)) return;
    const PointSceneRT sc = point_scene_row_load(uni, rows, a.Kl, i);
    rollout_point_body<true, -1, true, true>(a, sc, &wt);
}
template <int OCC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(OCC, OCC))) void k_rollout_point_sv_occ(
    const RolloutArgs a, const PointSceneRT uni, const float* __restrict__ rows, const PointCostWeights wt) {
    int i;
    if (!rollout_lane_sample(a, i)) return;
    const PointSceneRT sc = point_scene_row_load(uni, rows, a.Kl, i);
    rollout_point_body<true, -1, false, true>(a, sc, &wt);
}

// the builds by the number of wavefronts, as for every other instance (rollout_point_build; no _ref build on PointSceneRT)
void launch_rollout_point_sv(const RolloutArgs& a, const PointSceneRT& uni, const float* rows, const PointCostWeights& wt,
                             int blocks, hipStream_t s) {
    const dim3 grid(blocks), wg(64);
    switch (rollout_point_build(blocks, false)) {
        case BUILD_OCC3: hipLaunchKernelGGL(k_rollout_point_sv_occ<3>, grid, wg, 0, s, a, uni, rows, wt); break;
        case BUILD_OCC2: hipLaunchKernelGGL(k_rollout_point_sv_occ<2>, grid, wg, 0, s, a, uni, rows, wt); break;
        default: hipLaunchKernelGGL(k_rollout_point_sv, grid, wg, 0, s, a, uni, rows, wt); break;
    }
}

// ---- batched command (m3_batch_command on a batch with the per-sample section): one launch for a group of such handles that
// share K, T and lanes.  blockIdx.y picks the handle's entry (BatchRolloutEntrySV, m3_internal.hpp; read-only); the entry's
// scene_rt gives the uniform members, so handles with different dt / substeps share a launch and every trip count stays
// wave-uniform per handle; the rows are the handle's own device table.  The same body instantiations as the single-handle
// kernels above, the build picked by the GROUP's wavefront count: same bits.
__global__ __launch_bounds__(64) void kb_rollout_point_sv(const BatchRolloutEntrySV* __restrict__ tab) {
    const BatchRolloutEntrySV& e = tab[blockIdx.y];
    int i;
    if (!rollout_lane_sample(e.a, i)) return;
    const PointSceneRT sc = point_scene_row_load(e.sc, e.rows, e.a.Kl, i);
    rollout_point_body<true, -1, true, true>(e.a, sc, &e.wt);
}
template <int OCC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(OCC, OCC))) void kb_rollout_point_sv_occ(
    const BatchRolloutEntrySV* __restrict__ tab) {
    const BatchRolloutEntrySV& e = tab[blockIdx.y];
    int i;
    if (!rollout_lane_sample(e.a, i)) return;
    const PointSceneRT sc = point_scene_row_load(e.sc, e.rows, e.a.Kl, i);
    rollout_point_body<true, -1, false, true>(e.a, sc, &e.wt);
}

// blocks: workgroups of ONE handle (all handles of the group have the same); n: handles
void launch_rollout_point_sv_batch(const BatchRolloutEntrySV* tab, int blocks, int n, hipStream_t s) {
    const dim3 grid(blocks, n), wg(64);
    switch (rollout_point_build(blocks * n, false)) {
        case BUILD_OCC3: hipLaunchKernelGGL(kb_rollout_point_sv_occ<3>, grid, wg, 0, s, tab); break;
        case BUILD_OCC2: hipLaunchKernelGGL(kb_rollout_point_sv_occ<2>, grid, wg, 0, s, tab); break;
        default: hipLaunchKernelGGL(kb_rollout_point_sv, grid, wg, 0, s, tab); break;
    }
}

}  // namespace m3
