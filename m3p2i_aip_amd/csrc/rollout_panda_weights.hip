// rollout_panda_weights.hip -- the panda_env kernels of a handle whose cost weights are not the reference's literals
// (m3_set_panda_cost_weights, include/m3p2i_hip.h): the seven weights are a kernel argument
// (PandaCostWeights) read by the weighted overload of panda_cost.  The same bodies as rollout_panda_scene.hip over the same
// device header under the same flags, on the run-time scene (the handle's PandaSceneRT is always maintained, so one family
// serves the reference's workspace and any other); at the default weights the same bits.
// New kernels only: a handle with the default weights never launches one of these (unless m3_set_panda_weighted_cost_instance
// forces it).
//
// The weights are wave-uniform and are read in one place per step, where the cost is formed after the substeps: the cost hook
// reads them from the kernel-argument segment there (kernarg_weights, rollout_panda_common.hpp) instead of holding seven more
// scalars over the substep loop, whose builds already spill two to three hundred.
#define PANDA_BODY_COST(w, o, k, cube0, qh0) panda_cost(pa.cp, kernarg_weights<WT_OFFSET>(), w, o, k, cube0, qh0)
#include "m3_internal.hpp"
#include "noise_stream.hpp"
#include "panda_dyn.hpp"
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
#include "rollout_panda_body.inc"
}

// k_panda_reach_cost's body with the weighted cost (reads the record buffer, no scene)
__global__ __launch_bounds__(64 * RC_TS) void k_panda_reach_cost_w(const RolloutArgs a, const PandaArgs pa, const PandaCostWeights wt) {
    constexpr size_t WT_OFFSET = kernarg_offset<RolloutArgs, PandaArgs, PandaCostWeights>(0);
#include "panda_reach_cost_body.inc"
}

template <int LPS>
static void launch_rollout_panda_w_lps(const RolloutArgs& a_in, const PandaArgs& pa, const PandaSceneRT& sc,
                                       const PandaCostWeights& wt, const RolloutPlan& p, hipStream_t s) {
    RolloutArgs a = a_in;
    a.lanes = p.lanes;
    const dim3 grid(p.blocks), block(64);
    if (p.forces) hipLaunchKernelGGL((k_rollout_panda_w<true, LPS>), grid, block, 0, s, a, pa, sc, wt);
    else hipLaunchKernelGGL((k_rollout_panda_w<false, LPS>), grid, block, 0, s, a, pa, sc, wt);
}
void launch_panda_reach_cost_w(const RolloutArgs& a, const PandaArgs& pa, const PandaCostWeights& wt, hipStream_t s) {
    hipLaunchKernelGGL(k_panda_reach_cost_w, dim3((a.Kl + 63) / 64), dim3(64 * RC_TS), 0, s, a, pa, wt);
}
// pa, p: as plan_rollout_panda left them (the form is chosen exactly as for the literal weights)
void launch_rollout_panda_w(const RolloutArgs& a, const PandaArgs& pa, const PandaSceneRT& sc, const PandaCostWeights& wt,
                            const RolloutPlan& p, hipStream_t s) {
    if (p.lps == 16) launch_rollout_panda_w_lps<16>(a, pa, sc, wt, p, s);
    else if (p.lps == 8) launch_rollout_panda_w_lps<8>(a, pa, sc, wt, p, s);
    else launch_rollout_panda_w_lps<1>(a, pa, sc, wt, p, s);
    if (p.rec) launch_panda_reach_cost_w(a, pa, wt, s);
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
void launch_psim_cost_w(const PandaSceneRT& sc, const PandaCostParams& cp, const PandaCostWeights& wt, const float* world, int Kl,
                        int k0, bool env0_cube, float* cost, hipStream_t s) {
    hipLaunchKernelGGL(k_psim_cost_w, dim3((Kl + 63) / 64), dim3(64), 0, s, sc, cp, wt, world, Kl, k0, env0_cube ? 1 : 0, cost);
}

}  // namespace m3
