// rollout_point_scene_rows.hip -- the step-mode kernels of a sim_only handle with one arena PER ENVIRONMENT
// (m3_set_point_scene_rows): the per-row twins of k_sim_step_s and k_episodes_post_s (rollout_point_scene.hip).  The same bodies
// (point_step_mode.hpp) on the same scene type; each lane builds its PointSceneRT in registers from row i of the handle's table
// (point_scene_rows.hpp).  A translation unit of its own, like its neighbour: every kernel that was in the library keeps its code.
#include "episode_lane.hpp"
#include "point_step_mode.hpp"
#include "point_scene_rows.hpp"

namespace m3 {

// uni: the handle's scene_rt, read for its uniform members only; rows: [POINT_SCENE_ROW_WORDS][Kl]
__global__ __launch_bounds__(64) void k_sim_step_sv(const PointSceneRT uni, const float* __restrict__ rows, const SimViews v,
                                                    float* wd, const float* u, float* u_keep, int Kl) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Kl) return;   // (the body's own guard, in front of the row's loads)
    const PointSceneRT sc = point_scene_row_load(uni, rows, Kl, i);
    sim_step_body(sc, v, wd, u, u_keep, Kl);
}
void launch_sim_step_sv(const PointSceneRT& uni, const float* rows, const SimViews& v, float* world, const float* u,
                        float* u_keep, int Kl, hipStream_t s) {
    hipLaunchKernelGGL(k_sim_step_sv, dim3((Kl + 63) / 64), dim3(64), 0, s, uni, rows, v, world, u, u_keep, Kl);
}

// rows: [POINT_SCENE_ROW_WORDS][a.n] (the world's K_local is the number of episodes)
__global__ __launch_bounds__(64) void k_episodes_post_sv(const PointSceneRT uni, const float* __restrict__ rows,
                                                         const EpisodeArgs a, int tick) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= a.n) return;
    const PointSceneRT sc = point_scene_row_load(uni, rows, a.n, e);
    episodes_post_body(sc, a, tick);
}
void launch_episodes_post_sv(const PointSceneRT& uni, const float* rows, const EpisodeArgs& a, int tick, hipStream_t s) {
    hipLaunchKernelGGL(k_episodes_post_sv, dim3((a.n + 63) / 64), dim3(64), 0, s, uni, rows, a, tick);
}

}  // namespace m3
