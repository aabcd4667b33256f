// rollout_panda_priors.hip -- the panda_env rollout kernels of a planner handle with prior samples (m3_set_panda_prior_samples,
// DESIGN.md section 7l): some of the K samples take a caller-given control sequence verbatim -- clamp(seqs[j][t]) in place of
// clamp(mean[shift(t)] + noise) -- and everything behind that select (the gripper command's override of controls 7 and 8,
// u_scale, the stored actions, simple mode's perturbation cost, the update) is what it is for every other sample.
//
// The construction of k_rollout_panda_v (rollout_panda_rows.hip): the workspace a kernel argument, the cost weights read from
// the kernel-argument segment at the cost site, a table of workspaces per sample -- which here may be null (wave-uniform: the
// handle's one workspace), so that one family serves prior samples with and without m3_set_panda_rollout_scenes.  On top of it
// the third hook of the shared body (rollout_panda_common.hpp: PANDA_PRIORS_KERNARG).  New kernels only: a handle without prior
// samples never launches one of these, and a handle that clears them is back on the kernels it ran before.
//
// Which prior: the prior follows the SAMPLE i, as the scene row does -- the hook reads prior_slot[i] where `i` is final (a_.lanes,
// the shadow slots and the ragged last wavefront applied; lanes that left never reach it, so every read is inside [Kl], and a row
// read is inside the table: the slot is < the rows the setter wrote).  The lanes of one sample read one slot and one row, so the
// sharing inside a sample keeps its precondition; a shadow slot (i = 0 or K / 2) takes that sample's prior.
#include "m3_internal.hpp"
#include "noise_stream.hpp"
#include "panda_dyn.hpp"
#include "panda_scene_rows.hpp"
#include "rollout_panda_common.hpp"
#include "wave_min.hpp"

namespace m3 {

// six kernels (FORCES x LPS), GENERAL always on
template <bool FORCES, int LPS>
__global__ __launch_bounds__(64) void k_rollout_panda_pr(const RolloutArgs a_, const PandaArgs pa, const PandaSceneRT sc_,
                                                         const PandaCostWeights wt, const float* scene_rows, const int* prior_slot,
                                                         const float* prior_tab) {
    constexpr bool GENERAL = true;
    constexpr size_t WT_OFFSET = kernarg_offset<RolloutArgs, PandaArgs, PandaSceneRT, PandaCostWeights>(0);
    using SceneT = PandaSceneRT;
#define PANDA_BODY_COST PANDA_COST_KERNARG_WEIGHTS
#define PANDA_BODY_SCENE PANDA_SCENE_KERNARG_ROWS_OR_UNIFORM
#define PANDA_BODY_PRIORS PANDA_PRIORS_KERNARG
#include "rollout_panda_body.inc"
}

// (lanes per sample, shadow slots or record as for every family; sc.rows: null unless the handle has a workspace per sample.  The
// record path: the weighted reach-cost kernel of rollout_panda_weights.hip behind the rollout, as for the rows family)
void launch_rollout_panda_priors(const RolloutArgs& a, const PandaArgs& pa, const PandaLaunchScene& sc, const RolloutPlan& p, hipStream_t s) {
    launch_panda_instance(p, dim3(p.blocks), s, [](auto forces, auto, auto lps) {
        return &k_rollout_panda_pr<decltype(forces)::value, decltype(lps)::value>;
    }, a, pa, *sc.rt, *sc.wt, sc.rows, sc.prior_slot, sc.prior_tab);
}

}  // namespace m3
