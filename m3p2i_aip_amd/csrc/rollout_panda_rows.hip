// rollout_panda_rows.hip -- the panda_env kernels of a handle with one workspace per row: per SAMPLE of a
// planner handle's fused rollout (m3_set_panda_rollout_scenes) and per ENVIRONMENT of a sim_only handle's step mode
// (m3_set_panda_scene_rows).  The same bodies as rollout_panda_weights.hip / rollout_panda_scene.hip over the same device header
// under the same flags; a lane overwrites the 22 workspace words of its PandaSceneRT from the word-major table
// (panda_scene_rows.hpp) before anything reads them.  Rows that all equal one scene give the bits of the twin in that scene.
// New kernels only: a handle without rows never launches one of these.
//
// The rollout family always takes the cost weights (the construction of k_rollout_panda_w): at the default weights the
// weighted cost gives the literal cost's bits (section 7f), so one family serves rows with and without tuned weights.
//
// Which row: the scene follows the SAMPLE.  The hook runs where the body's `i` is final -- a_.lanes, the shadow slots (which
// re-simulate samples 0 and K / 2 and so load rows 0 and K / 2: quirk Q8 reads the cube of sample 0 as simulated in scenes[0])
// and the ragged last wavefront applied; lanes that left (slot >= a_.lanes, i >= Kl) never reach it, so every read is inside
// [22][Kl].  The lanes of one sample read one row: the DPP / bpermute sharing inside a sample keeps its precondition, and the
// wave-level decisions of panda_dyn.hpp are ballots of per-lane predicates, each formed from the lane's own scene.
#include "m3_internal.hpp"
#include "noise_stream.hpp"
#include "panda_dyn.hpp"
#include "panda_scene_rows.hpp"
#include "panda_step_mode.hpp"
#include "rollout_panda_common.hpp"
#include "wave_min.hpp"

namespace m3 {

// k_rollout_panda_w's body with the sample's workspace from row i: six kernels (FORCES x LPS), GENERAL always on
template <bool FORCES, int LPS>
__global__ __launch_bounds__(64) void k_rollout_panda_v(const RolloutArgs a_, const PandaArgs pa, const PandaSceneRT sc_,
                                                        const PandaCostWeights wt, const float* scene_rows) {
    constexpr bool GENERAL = true;
    constexpr size_t WT_OFFSET = kernarg_offset<RolloutArgs, PandaArgs, PandaSceneRT, PandaCostWeights>(0);
    using SceneT = PandaSceneRT;
#define PANDA_BODY_COST PANDA_COST_KERNARG_WEIGHTS
#define PANDA_BODY_SCENE PANDA_SCENE_KERNARG_ROWS
#include "rollout_panda_body.inc"
}

// (lanes per sample, shadow slots or record exactly as for a single scene.  The record path needs no scene: the weighted
// reach-cost kernel of rollout_panda_weights.hip behind the rollout)
void launch_rollout_panda_rows(const RolloutArgs& a, const PandaArgs& pa, const PandaLaunchScene& sc, const RolloutPlan& p, hipStream_t s) {
    launch_panda_instance(p, dim3(p.blocks), s, [](auto forces, auto, auto lps) {
        return &k_rollout_panda_v<decltype(forces)::value, decltype(lps)::value>;
    }, a, pa, *sc.rt, *sc.wt, sc.rows);
}

// ---- step mode: the bodies of k_psim_step_s / _pull_s / _push_s and of k_psim_cost_w with lane e's scene from row e ----
__global__ __launch_bounds__(64) void k_psim_step_v(const PandaSceneRT uni, const float* scene_rows, const SimViews v, float* wd,
                                                    const float* u, float* u_keep, int Kl) {
    PANDA_CORNER_LDS(1);
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Kl) return;
    const PandaSceneRT sc = panda_scene_row_scene(uni, scene_rows, Kl, i);
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
void launch_psim_step_rows(const PandaLaunchScene& sc, const SimViews& v, float* world, const float* u, float* u_keep, int Kl,
                           hipStream_t s) {
    launch_psim(k_psim_step_v, Kl, s, *sc.rt, sc.rows, v, world, u, u_keep, Kl);
}

__global__ __launch_bounds__(64) void k_psim_pull_v(const PandaSceneRT uni, const float* scene_rows, const SimViews v, float* wd,
                                                    int Kl) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Kl) return;
    const PandaSceneRT sc = panda_scene_row_scene(uni, scene_rows, Kl, i);
    psim_pull_body(sc, v, wd, Kl, i);
}
void launch_psim_pull_rows(const PandaLaunchScene& sc, const SimViews& v, float* world, int Kl, hipStream_t s) {
    launch_psim(k_psim_pull_v, Kl, s, *sc.rt, sc.rows, v, world, Kl);
}

__global__ __launch_bounds__(64) void k_psim_push_v(const PandaSceneRT uni, const float* scene_rows, const SimViews v,
                                                    const float* wd, int Kl) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Kl) return;
    const PandaSceneRT sc = panda_scene_row_scene(uni, scene_rows, Kl, i);
    psim_push_body(sc, v, wd, Kl, i);
}
void launch_psim_push_rows(const PandaLaunchScene& sc, const SimViews& v, const float* world, int Kl, hipStream_t s) {
    launch_psim(k_psim_push_v, Kl, s, *sc.rt, sc.rows, v, world, Kl);
}

__global__ __launch_bounds__(64) void k_psim_cost_v(const PandaSceneRT uni, const float* scene_rows, const PandaCostParams cp,
                                                    const PandaCostWeights wt, const float* wd, int Kl, int k0, int env0_cube,
                                                    float* cost) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Kl) return;
    const PandaSceneRT sc = panda_scene_row_scene(uni, scene_rows, Kl, i);
    PandaWorld w;
    psoa_load(wd, Kl, i, w);
    Frame hand;
    PandaObs o;
    panda_fk<false>(sc, w.q, hand, o.left, o.right, nullptr);
    mat2quat(hand, o.left_q);
    // quirk Q8: environment 0's cube position, the orientation of the first environment of the sample's half (rows 18-24) --
    // each as its own environment's workspace left it
    float cube0[3], qh0[4];
    const bool env0 = env0_cube != 0;
    const int src = env0 ? ((cp.multi_modal && i >= cp.half_K) ? cp.half_K : 0) : i;
#pragma unroll
    for (int j = 0; j < 3; ++j) cube0[j] = wd[(18 + j) * Kl + (env0 ? 0 : i)];
#pragma unroll
    for (int j = 0; j < 4; ++j) qh0[j] = wd[(21 + j) * Kl + src];
    cost[i] = panda_cost(cp, wt, w, o, k0 + i, cube0, qh0);
}
void launch_psim_cost_rows(const PandaLaunchScene& sc, const PandaCostParams& cp, const float* world, int Kl, int k0, bool env0_cube,
                           float* cost, hipStream_t s) {
    launch_psim(k_psim_cost_v, Kl, s, *sc.rt, sc.rows, cp, *sc.wt, world, Kl, k0, env0_cube ? 1 : 0, cost);
}

}  // namespace m3
