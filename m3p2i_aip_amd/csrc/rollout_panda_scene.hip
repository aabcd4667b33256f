// rollout_panda_scene.hip -- the panda_env kernels of a handle whose workspace is not the reference's (m3_set_panda_scene,
// include/m3p2i_hip.h): robot mount, table, shelf stand, the plate's size and the contact friction are
// members of the kernel argument (PandaSceneRT) instead of PandaScene's compile-time constants.  The same bodies as
// rollout_panda.hip (rollout_panda_body.inc, panda_step_mode.hpp) over the same device header under the same flags; at the
// default values the same bits.
// New kernels only: a handle with the reference's workspace never launches one of these.
#include "m3_internal.hpp"
#include "noise_stream.hpp"
#include "panda_dyn.hpp"
#include "panda_step_mode.hpp"
#include "rollout_panda_common.hpp"
#include "wave_min.hpp"

namespace m3 {

// k_rollout_panda's body with the run-time scene.  GENERAL is always on: the body turns the general parts off from the
// run-time flags of RolloutArgs, so one build serves both samplers and both mppi modes -- six kernels (FORCES x LPS).
template <bool FORCES, int LPS>
__global__ __launch_bounds__(64) void k_rollout_panda_s(const RolloutArgs a_, const PandaArgs pa, const PandaSceneRT sc_) {
    constexpr bool GENERAL = true;
    using SceneT = PandaSceneRT;
#define PANDA_BODY_COST PANDA_COST_LITERAL
#define PANDA_BODY_SCENE PANDA_SCENE_UNIFORM
#include "rollout_panda_body.inc"
}
// (the form is chosen exactly as for the compiled-in workspace; the literal reach-cost kernel behind it: rollout_panda.hip)
void launch_rollout_panda_scene(const RolloutArgs& a, const PandaArgs& pa, const PandaLaunchScene& sc, const RolloutPlan& p, hipStream_t s) {
    launch_panda_instance(p, dim3(p.blocks), s, [](auto forces, auto, auto lps) {
        return &k_rollout_panda_s<decltype(forces)::value, decltype(lps)::value>;
    }, a, pa, *sc.rt);
}

// ---- step mode: k_psim_step / _pull / _push / _cost (rollout_panda.hip) with the run-time scene ----
__global__ __launch_bounds__(64) void k_psim_step_s(const PandaSceneRT sc, const SimViews v, float* wd, const float* u,
                                                    float* u_keep, int Kl) {
    PANDA_CORNER_LDS(1);
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Kl) return;
    PandaWorld w;
    psoa_load(wd, Kl, i, w);
    float uu[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) uu[j] = u[(size_t)i * 9 + j];
    if (u_keep != u) {   // (targets taken from the caller's tensor: kept for the steps after this one)
#pragma unroll
        for (int j = 0; j < 9; ++j) u_keep[(size_t)i * 9 + j] = uu[j];
    }
    PandaObs obs;
    panda_step(sc, w, uu, obs, cs);
    psoa_store(wd, Kl, i, w);
    panda_push_views(sc, v, i, w);
}
void launch_psim_step_scene(const PandaLaunchScene& sc, const SimViews& v, float* world, const float* u, float* u_keep, int Kl,
                            hipStream_t s) {
    launch_psim(k_psim_step_s, Kl, s, *sc.rt, v, world, u, u_keep, Kl);
}

__global__ __launch_bounds__(64) void k_psim_pull_s(const PandaSceneRT sc, const SimViews v, float* wd, int Kl) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Kl) return;
    psim_pull_body(sc, v, wd, Kl, i);
}
void launch_psim_pull_scene(const PandaLaunchScene& sc, const SimViews& v, float* world, int Kl, hipStream_t s) {
    launch_psim(k_psim_pull_s, Kl, s, *sc.rt, v, world, Kl);
}

__global__ __launch_bounds__(64) void k_psim_push_s(const PandaSceneRT sc, const SimViews v, const float* wd, int Kl) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Kl) return;
    psim_push_body(sc, v, wd, Kl, i);
}
void launch_psim_push_scene(const PandaLaunchScene& sc, const SimViews& v, const float* world, int Kl, hipStream_t s) {
    launch_psim(k_psim_push_s, Kl, s, *sc.rt, v, world, Kl);
}

__global__ __launch_bounds__(64) void k_psim_cost_s(const PandaSceneRT sc, const PandaCostParams cp, const float* wd,
                                                    int Kl, int k0, int env0_cube, float* cost) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Kl) return;
    PandaWorld w;
    psoa_load(wd, Kl, i, w);
    Frame hand;
    PandaObs o;
    panda_fk<false>(sc, w.q, hand, o.left, o.right, nullptr);
    mat2quat(hand, o.left_q);
    // quirk Q8: environment 0's cube position, the orientation of the first environment of the sample's half (rows 18-24)
    float cube0[3], qh0[4];
    const bool env0 = env0_cube != 0;
    const int src = env0 ? ((cp.multi_modal && i >= cp.half_K) ? cp.half_K : 0) : i;
#pragma unroll
    for (int j = 0; j < 3; ++j) cube0[j] = wd[(18 + j) * Kl + (env0 ? 0 : i)];
#pragma unroll
    for (int j = 0; j < 4; ++j) qh0[j] = wd[(21 + j) * Kl + src];
    cost[i] = panda_cost(cp, w, o, k0 + i, cube0, qh0);
}
void launch_psim_cost_scene(const PandaLaunchScene& sc, const PandaCostParams& cp, const float* world, int Kl, int k0, bool env0_cube,
                            float* cost, hipStream_t s) {
    launch_psim(k_psim_cost_s, Kl, s, *sc.rt, cp, world, Kl, k0, env0_cube ? 1 : 0, cost);
}

}  // namespace m3
