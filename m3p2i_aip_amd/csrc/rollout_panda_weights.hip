// rollout_panda_weights.hip -- the panda_env kernels of a handle whose cost weights are not the reference's literals
// (m3_set_panda_cost_weights, include/m3p2i_hip.h): the seven weights are a kernel argument
// (PandaCostWeights) read by the weighted overload of panda_cost.  The same bodies as rollout_panda_scene.hip over the same
// device header under the same flags, on the run-time scene (the handle's PandaSceneRT is always maintained, so one family
// serves the reference's workspace and any other); at the default weights the same bits.
// New kernels only: a handle with the default weights never launches one of these (unless m3_set_panda_weighted_cost_instance
// forces it).
//
// The weights are wave-uniform and are read in one place per step, where the cost is formed after the substeps: the cost hook
// (kernarg_weighted_cost, rollout_panda_common.hpp) reads them from the kernel-argument segment there (kernarg_weights) instead
// of holding seven more scalars over the substep loop, whose builds already spill two to three hundred.
#include "m3_internal.hpp"
#include "noise_stream.hpp"
#include "panda_dyn.hpp"
#include "panda_step_mode.hpp"
#include "rollout_panda_common.hpp"
#include "wave_min.hpp"

namespace m3 {

// k_rollout_panda_s's body with the weighted cost: six kernels (FORCES x LPS), GENERAL always on
template <bool FORCES, int LPS>
__global__ __launch_bounds__(64) void k_rollout_panda_w(const RolloutArgs a_, const PandaArgs pa, const PandaSceneRT sc_,
                                                        const PandaCostWeights wt) {
    constexpr bool GENERAL = true;
    constexpr size_t WT_OFFSET = kernarg_offset<RolloutArgs, PandaArgs, PandaSceneRT, PandaCostWeights>(0);
    using SceneT = PandaSceneRT;
#define PANDA_BODY_COST PANDA_COST_KERNARG_WEIGHTS
#define PANDA_BODY_SCENE PANDA_SCENE_UNIFORM
#include "rollout_panda_body.inc"
}

// k_panda_reach_cost's body with the weighted cost (reads the record buffer, no scene)
__global__ __launch_bounds__(64 * RC_TS) void k_panda_reach_cost_w(const RolloutArgs a, const PandaArgs pa, const PandaCostWeights wt) {
    constexpr size_t WT_OFFSET = kernarg_offset<RolloutArgs, PandaArgs, PandaCostWeights>(0);
#define PANDA_BODY_COST PANDA_COST_KERNARG_WEIGHTS
#include "panda_reach_cost_body.inc"
}

// (the form is chosen exactly as for the literal weights)
void launch_rollout_panda_weighted(const RolloutArgs& a, const PandaArgs& pa, const PandaLaunchScene& sc, const RolloutPlan& p, hipStream_t s) {
    launch_panda_instance(p, dim3(p.blocks), s, [](auto forces, auto, auto lps) {
        return &k_rollout_panda_w<decltype(forces)::value, decltype(lps)::value>;
    }, a, pa, *sc.rt, *sc.wt);
}
void launch_panda_reach_cost_weighted(const RolloutArgs& a, const PandaArgs& pa, const PandaLaunchScene& sc, hipStream_t s) {
    launch_panda_reach_cost(k_panda_reach_cost_w, a.Kl, 1, s, a, pa, *sc.wt);
}

// ---- step mode: k_psim_cost_s (rollout_panda_scene.hip) with the weighted cost, for m3_cost ----
__global__ __launch_bounds__(64) void k_psim_cost_w(const PandaSceneRT sc, const PandaCostParams cp, const PandaCostWeights wt,
                                                    const float* wd, int Kl, int k0, int env0_cube, float* cost) {
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
    cost[i] = panda_cost(cp, wt, w, o, k0 + i, cube0, qh0);
}
void launch_psim_cost_weighted(const PandaLaunchScene& sc, const PandaCostParams& cp, const float* world, int Kl, int k0,
                               bool env0_cube, float* cost, hipStream_t s) {
    launch_psim(k_psim_cost_w, Kl, s, *sc.rt, cp, *sc.wt, world, Kl, k0, env0_cube ? 1 : 0, cost);
}

}  // namespace m3
