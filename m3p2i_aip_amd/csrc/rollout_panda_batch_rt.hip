// rollout_panda_batch_rt.hip -- the batched panda_env kernels of handles with a run-time workspace (m3_set_panda_scene), tuned
// cost weights (m3_set_panda_cost_weights) or a workspace per sample (m3_set_panda_rollout_scenes): what m3_batch_command
// launches for the second section of a panda table (BatchPandaEntryRT; a batch created with M3_BATCH_PANDA_RUNTIME, DESIGN.md
// section 7b.2).  The same bodies as rollout_panda_weights.hip / rollout_panda_rows.hip over the same device header under the
// same flags, with every argument read from the table entry of blockIdx.y (as kb_rollout_panda, rollout_panda.hip).
// New kernels only: thirteen -- kb_rollout_panda_w and kb_rollout_panda_v (FORCES x LPS each), kb_panda_reach_cost_w.
//
// ONE construction serves every such handle: the weighted cost on the run-time scene, GENERAL on.
//   - At the default weights the weighted cost gives the literal cost's bits, and GENERAL on gives the bits of GENERAL off
//     (section 7f).  So a handle that has a run-time scene ALONE -- whose own m3_command runs k_rollout_panda_s<.., GENERAL, ..>,
//     the literal cost -- goes through kb_rollout_panda_w here and still reproduces its own command bit for bit; likewise a
//     handle with m3_set_panda_scene_instance(h, 1) / m3_set_panda_weighted_cost_instance(h, 1) at the default values
//     reproduces the literal kernels (tests/test_batch_panda_runtime_gpu.py pins both).
//   - A handle with rows takes kb_rollout_panda_v whether its weights are tuned or not, as its own command takes
//     k_rollout_panda_v.
//
// The weights are read from the table entry AT THE COST SITE, through a reference into the read-only `__restrict__` table, not
// from a copy taken before the substep loop: rollout_panda_weights.hip says why (these builds already spill two to three
// hundred scalars; seven more values held over the loop are seven more spills).
// The row of kb_rollout_panda_v follows the SAMPLE index `i` as the body finalises it (a_.lanes, the shadow slots -- which load
// rows 0 and K / 2 -- and the ragged last wavefront applied; rollout_panda_rows.hip), never the lane, the slot or blockIdx.y:
// blockIdx.y only picks WHICH handle's table [22][K_local] is read.  Lanes that left (slot >= a_.lanes, i >= Kl) never reach
// the hook, so every read is inside that table.
#include "m3_internal.hpp"
#include "noise_stream.hpp"
#include "panda_dyn.hpp"
#include "panda_scene_rows.hpp"
#include "rollout_panda_common.hpp"
#include "wave_min.hpp"

namespace m3 {

// k_rollout_panda_w's construction from the table: six kernels (FORCES x LPS), GENERAL always on
template <bool FORCES, int LPS>
__global__ __launch_bounds__(64) void kb_rollout_panda_w(const BatchPandaEntryRT* __restrict__ tab) {
    constexpr bool GENERAL = true;
    const RolloutArgs& a_ = tab[blockIdx.y].a;
    const PandaArgs& pa = tab[blockIdx.y].pa;
    const PandaSceneRT& sc_ = tab[blockIdx.y].sc;
    using SceneT = PandaSceneRT;
#define PANDA_BODY_COST PANDA_COST_TABLE_WEIGHTS
#define PANDA_BODY_SCENE PANDA_SCENE_UNIFORM
#include "rollout_panda_body.inc"
}

// k_panda_reach_cost_w's body from the table (reads the record buffer, no scene): behind a group of either family that keeps
// the record
__global__ __launch_bounds__(64 * RC_TS) void kb_panda_reach_cost_w(const BatchPandaEntryRT* __restrict__ tab) {
    const RolloutArgs& a = tab[blockIdx.y].a;
    const PandaArgs& pa = tab[blockIdx.y].pa;
#define PANDA_BODY_COST PANDA_COST_TABLE_WEIGHTS
#include "panda_reach_cost_body.inc"
}

// k_rollout_panda_v's construction from the table: the sample's 22 workspace words from row i of the handle's own rows
template <bool FORCES, int LPS>
__global__ __launch_bounds__(64) void kb_rollout_panda_v(const BatchPandaEntryRT* __restrict__ tab) {
    constexpr bool GENERAL = true;
    const RolloutArgs& a_ = tab[blockIdx.y].a;
    const PandaArgs& pa = tab[blockIdx.y].pa;
    const PandaSceneRT& sc_ = tab[blockIdx.y].sc;
    using SceneT = PandaSceneRT;
#define PANDA_BODY_COST PANDA_COST_TABLE_WEIGHTS
#define PANDA_BODY_SCENE PANDA_SCENE_TABLE_ROWS
#include "rollout_panda_body.inc"
}

// p: the group's plan (every member's own); per_sample: the group's entries carry rows (variant 2)
void launch_rollout_panda_batch_rt(const BatchPandaEntryRT* tab, int n, bool per_sample, const RolloutPlan& p, int Kl, hipStream_t s) {
    const dim3 grid(p.blocks, n);
    if (per_sample)
        launch_panda_instance(p, grid, s, [](auto forces, auto, auto lps) {
            return &kb_rollout_panda_v<decltype(forces)::value, decltype(lps)::value>;
        }, tab);
    else
        launch_panda_instance(p, grid, s, [](auto forces, auto, auto lps) {
            return &kb_rollout_panda_w<decltype(forces)::value, decltype(lps)::value>;
        }, tab);
    if (p.rec) launch_panda_reach_cost(kb_panda_reach_cost_w, Kl, n, s, tab);
}

}  // namespace m3
