// rollout_point_scene.hip -- the step-mode kernels of a handle with a run-time arena (m3_set_point_scene): the twins of
// k_sim_step and k_episodes_post (rollout_point.hip) on PointSceneRT.  A translation unit of their own: compiled next to the
// default-scene kernels they changed the code generated for k_episodes_post.
#include "episode_lane.hpp"
#include "point_step_mode.hpp"

namespace m3 {

// ... of a handle with a run-time scene (m3_set_point_scene)
__global__ __launch_bounds__(64) void k_sim_step_s(const PointSceneRT sc, const SimViews v, float* wd, const float* u,
                                                   float* u_keep, int Kl) {
    sim_step_body(sc, v, wd, u, u_keep, Kl);
}
void launch_sim_step_s(const PointSceneRT& sc, const SimViews& v, float* world, const float* u, float* u_keep, int Kl,
                       hipStream_t s) {
    hipLaunchKernelGGL(k_sim_step_s, dim3((Kl + 63) / 64), dim3(64), 0, s, sc, v, world, u, u_keep, Kl);
}

// ... of a world handle with a run-time scene (m3_set_point_scene)
__global__ __launch_bounds__(64) void k_episodes_post_s(const PointSceneRT sc, const EpisodeArgs a, int tick) {
    episodes_post_body(sc, a, tick);
}
void launch_episodes_post_s(const PointSceneRT& sc, const EpisodeArgs& a, int tick, hipStream_t s) {
    hipLaunchKernelGGL(k_episodes_post_s, dim3((a.n + 63) / 64), dim3(64), 0, s, sc, a, tick);
}

}  // namespace m3
