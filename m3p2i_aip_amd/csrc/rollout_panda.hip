// rollout_panda.hip -- fused MPPI rollout kernel for the panda_env + step-mode kernels (gfx950).
//
// Same structure as rollout_point.hip: one launch = MPPI._compute_rollout_costs
// (mppi.py:296-315) for all K samples with the 9-dof action assembly (mppi.py:381-416, gripper
// override :412-416), T x { chain step (replaces reactive_tamp.py:63-70 -> Isaac Gym), task
// cost (cost_functions.py:91-169) }.  `dynamics` still reports dofs 0 and 1 as the 4-vector
// state (reactive_tamp.py:66-70), so states stay [T][K][4]; actions are [T][K][9].
// Algorithmic traffic per state-step: delta 36 B read; state 16 + action 36 + cost 4 B written.
#include "m3_internal.hpp"
#include "noise_stream.hpp"
#include "panda_dyn.hpp"
#include "panda_episode_lane.hpp"
#include "panda_step_mode.hpp"
#include "rollout_panda_common.hpp"
#include "wave_min.hpp"

#include <cstdlib>

namespace m3 {

// GENERAL = false: the reference's default sampler (halton-spline noise table), the path of every BASELINE
// config.  GENERAL = true adds what no shipped config turns on: the in-kernel random stream with a noise mean and a
// full covariance (sampling_method = 'random', mppi.py:129-131, :481; quirk Q4: that sample is scaled by
// sqrt(diag Sigma) once more) and mppi_mode = 'simple' (mppi.py:220-233, :335-372).
// LPS = lanes per sample (panda_dyn.hpp, world spec v3): 1 -- a lane simulates a sample on its own, 64 samples per wavefront;
// 16 -- the sixteen lanes of a DPP row simulate ONE sample together: everything but the contact solver's generalized vectors
// is replicated in them, the joint-space rows of the gripper contacts run across them.  Four samples per wavefront, so K = 4000
// is 1000 wavefronts, one per SIMD, instead of 63: the launch is as long as its slowest wavefront either way, and a wavefront's
// velocity passes are ~2.3x shorter (tools/ubench/coop_panda_rows.hip).  Chosen by plan_rollout_panda.
template <bool FORCES, bool GENERAL, int LPS>
__global__ __launch_bounds__(64) void k_rollout_panda(const RolloutArgs a_, const PandaArgs pa,
                                                      const PandaScene sc_) {
    using SceneT = PandaScene;
#define PANDA_BODY_COST PANDA_COST_LITERAL
#define PANDA_BODY_SCENE PANDA_SCENE_UNIFORM
#include "rollout_panda_body.inc"
}

// The reach cost of a launch that ran WITHOUT shadow slots (PandaArgs::reach_rec): quirk Q8 measures every rollout against the
// cube of environment 0 (and the tilted mode's orientation term against the first environment of the second half), which a
// rollout kernel can only know inside a wavefront by re-simulating those samples in it -- a quarter (half) of the sample slots
// with sixteen lanes per sample, a second round of wavefronts at K = 4000.  Instead the rollout leaves, per (step, sample), the
// seventeen floats the cost reads (finger positions 6, finger orientation 4, the sample's cube orientation 4 and position 3:
// [T][17][Kl], 5.4 MB at C4) and this kernel -- one lane per sample, the same panda_cost on the same values, the same
// discounted sum in the same order -- forms cost_horizon, the trajectory costs and the update's minima rows.
// Round 6: the T steps of a sample are independent until the discounted sum, so a workgroup is 64 samples x RC_TS time slices
// (one wavefront per slice): slice s forms the costs of steps s, s + RC_TS, ... -- seventeen loads per step in flight in four
// wavefronts instead of one lane walking all T x 17 of them --, the costs meet in LDS and the first wavefront adds them in step
// order with the rollout's own recurrence (J = J + g c; g = g gamma): the same operations on the same values, the same bits
// (16 -> 7 us at C4: profiles/r06).
__global__ __launch_bounds__(64 * RC_TS) void k_panda_reach_cost(const RolloutArgs a, const PandaArgs pa) {
#define PANDA_BODY_COST PANDA_COST_LITERAL
#include "panda_reach_cost_body.inc"
}

// Lanes per sample, by what was measured at C4's size (profiles/r05/panda_lps_bench.json, panda_reach_mid_bench.json; K = 4000,
// T = 20):
//   pick / place (no shadow slots, gripper + manifold rows in most wavefronts): 16 lanes 0.74 ms, 8 lanes 0.82, 1 lane 1.57 -- a
//     wavefront is the union of what its samples do and its rows run across the lanes: sixteen while the launch has <= 1024
//     wavefronts (one per SIMD: the launch lasts as long as its slowest wavefront), eight up to there, else one;
//   reach (quirk Q8): with the arm away from everything nothing touches anything, the time is the replicated part of the step,
//     which more lanes per sample only repeat in more wavefronts -- one lane with its shadow slots, 0.167 ms with the cubes asleep;
//     once the rollouts are next to the cube (most of an episode's reach phase) the many-lane forms win by up to 2x: sixteen lanes
//     WITHOUT shadow slots + k_panda_reach_cost where the launch has the record buffer, else eight lanes with them (sixteen
//     would lose 1-2 of 4 sample slots and need two rounds of wavefronts).  pa.reach_busy says which (m3_api.hip).
// Beyond 1024 wavefronts the launch is throughput-bound and the replicated work (16x / 8x more instructions per sample
// outside the solver) decides: one lane.  pa.lps (m3_set_panda_lanes_per_sample) forces a form.
static int panda_lps_for(const RolloutArgs& a, const PandaArgs& pa) {
    if (pa.lps == 1 || pa.lps == 8 || pa.lps == 16) return pa.lps;
    auto waves = [&](int lps) { const int per = 64 / lps - pa.shadows; return (a.Kl + per - 1) / per; };
    if (pa.shadows != 0) {
        // reach: one lane while next to nothing is near anything; eight lanes (one round of wavefronts with the shadow slots) once
        // the last command's rollouts had the gripper within reach of the cubes / the table often enough (pa.reach_busy: the share
        // the kernel reports, with hysteresis; m3_api.hip) -- the scenes 20 / 40 / 60 ticks
        // into an episode's reach phase (tools/panda_reach_mid_bench.py): 1 lane 0.174 / 0.778 / 1.535 ms, 8 lanes 0.198 /
        // 0.445 / 0.828, 16 lanes 0.271 / 0.561 / 1.265
        const bool busy = pa.reach_busy != 0;
        return (busy && waves(8) <= 1024) ? 8 : 1;
    }
    if (waves(16) <= 1024) return 16;
    if (waves(8) <= 1024) return 8;
    return 1;
}
// The form of a launch: the lanes per sample, the instance, the lanes per wavefront adjusted for the shadow slots and the grid;
// pa becomes what the kernels receive (no shadow slots with the record buffer; without it, and with the shadow slots again,
// when the one-lane form is chosen).
RolloutPlan plan_rollout_panda(const RolloutArgs& a, PandaArgs& pa) {
    const PandaArgs pa_in = pa;
    // reach without shadow slots (k_panda_reach_cost): when the handle holds the record buffer (m3_api.hip: K up to 8192), the
    // sampler is the default one and a many-lane form is what the launch
    // sixteen (eight) lanes per sample run in; automatic choice: while few of the last command's (sample, substep) pairs had the
    // gripper within reach of a box the one-lane form with its shadow slots is the faster launch (pa.reach_busy, m3_api.hip:
    // K = 4000, rollout ms one lane / sixteen lanes + cost kernel: arm at its initial pose 0.169 / 0.190, 20 ticks into an episode
    // 0.182 / 0.187, 30 ticks 0.388 / 0.248, 40 ticks 0.798 / 0.419, 60 ticks 1.541 / 0.778; profiles/r05/panda_reach_mid_bench.json)
    int lps = 0;
    if (pa.reach_rec != nullptr) {
        pa.shadows = 0;
        // (round 6: with the cost kernel in time slices the sixteen-lane form + cost kernel is at least as fast as one lane + shadow
        // slots in EVERY scene of an episode -- 10 ticks in 0.160 / 0.161 ms, 20 ticks 0.168 / 0.190, cubes settled 0.174 / 0.177,
        // initial scene 0.324 / 0.362, 60 ticks 0.744 / 1.545: profiles/r06/panda_reach_mid_bench.json -- so wherever one round of
        // sixteen-lane wavefronts fits (K <= 4096) the form no longer depends on the reported share; the eight-lane form, which
        // loses to one lane in quiet scenes, keeps following it)
        const bool sixteen_fits = (a.Kl + 3) / 4 <= 1024;
        const bool want = pa_in.shadows != 0 && !(a.sampling_random || a.mode_simple) && (pa.lps != 0 || pa.reach_busy != 0 || sixteen_fits);
        lps = want ? panda_lps_for(a, pa) : 1;
        if (lps == 1) pa = pa_in, pa.reach_rec = nullptr;
    }
    if (pa.reach_rec == nullptr) lps = panda_lps_for(a, pa);
    RolloutPlan p{};
    p.lps = lps;
    p.forces = pa.cp.task == 5 ? 1 : 0;
    p.general = (a.sampling_random || a.mode_simple) ? 1 : 0;
    p.shadows = pa.shadows;
    p.rec = pa.reach_rec != nullptr ? 1 : 0;
    const int spw = 64 / lps;
    int lanes = (a.lanes >= 1 && a.lanes <= spw) ? a.lanes : spw;
    if (lanes > spw - pa.shadows) lanes = spw - pa.shadows;
    p.lanes = lanes;
    p.blocks = (a.Kl + lanes - 1) / lanes;
    p.rows = !a.wave_min ? 0 : p.rec ? (a.Kl + 63) / 64 : p.blocks;
    return p;
}
static void launch_rollout_panda_literal(const RolloutArgs& a, const PandaArgs& pa, const PandaLaunchScene& sc, const RolloutPlan& p,
                                            hipStream_t s) {
    launch_panda_instance(p, dim3(p.blocks), s, [](auto forces, auto general, auto lps) {
        return &k_rollout_panda<decltype(forces)::value, decltype(general)::value, decltype(lps)::value>;
    }, a, pa, *sc.lit);
}
static void launch_panda_reach_cost_literal(const RolloutArgs& a, const PandaArgs& pa, const PandaLaunchScene&, hipStream_t s) {
    launch_panda_reach_cost(k_panda_reach_cost, a.Kl, 1, s, a, pa);
}
// pa: as plan_rollout_panda left it
void launch_rollout_panda(const RolloutArgs& a_in, const PandaArgs& pa, const PandaLaunchScene& sc, const RolloutPlan& p, hipStream_t s) {
    RolloutArgs a = a_in;
    a.lanes = p.lanes;
    switch (sc.variant) {
        case PANDA_LITERAL: launch_rollout_panda_literal(a, pa, sc, p, s); break;
        case PANDA_SCENE: launch_rollout_panda_scene(a, pa, sc, p, s); break;
        case PANDA_WEIGHTED: launch_rollout_panda_weighted(a, pa, sc, p, s); break;
        case PANDA_ROWS: launch_rollout_panda_rows(a, pa, sc, p, s); break;
        case PANDA_PRIORS: launch_rollout_panda_priors(a, pa, sc, p, s); break;
    }
    if (!p.rec) return;
    // (the reach-cost kernel reads the record buffer, no scene: the literal one or the weighted one serve every family)
    if (panda_cost_weighted(sc.variant)) launch_panda_reach_cost_weighted(a, pa, sc, s);
    else launch_panda_reach_cost_literal(a, pa, sc, s);
}

// ---- batched command (m3_batch_command) ---------------------------------------------------------------------------
// One workgroup of the handle tab[blockIdx.y], its own grid's workgroup blockIdx.x: the unchanged body.  The table is
// read-only during the launch (`__restrict__`).  A group's handles share K and the adjusted lanes, so gridDim.x is every
// handle's own grid -- which the busy report's last-wavefront ticket counts against (each handle has its own counter).
template <bool FORCES, bool GENERAL, int LPS>
__global__ __launch_bounds__(64) void kb_rollout_panda(const BatchPandaEntry* __restrict__ tab) {
    const RolloutArgs& a_ = tab[blockIdx.y].a;
    const PandaArgs& pa = tab[blockIdx.y].pa;
    const PandaScene& sc_ = tab[blockIdx.y].sc;
    using SceneT = PandaScene;
#define PANDA_BODY_COST PANDA_COST_LITERAL
#define PANDA_BODY_SCENE PANDA_SCENE_UNIFORM
#include "rollout_panda_body.inc"
}
__global__ __launch_bounds__(64 * RC_TS) void kb_panda_reach_cost(const BatchPandaEntry* __restrict__ tab) {
    const RolloutArgs& a = tab[blockIdx.y].a;
    const PandaArgs& pa = tab[blockIdx.y].pa;
#define PANDA_BODY_COST PANDA_COST_LITERAL
#include "panda_reach_cost_body.inc"
}
static void launch_rollout_panda_batch_literal(const BatchPandaEntry* tab, int n, const RolloutPlan& p, int Kl, hipStream_t s) {
    launch_panda_instance(p, dim3(p.blocks, n), s, [](auto forces, auto general, auto lps) {
        return &kb_rollout_panda<decltype(forces)::value, decltype(general)::value, decltype(lps)::value>;
    }, tab);
    if (p.rec) launch_panda_reach_cost(kb_panda_reach_cost, Kl, n, s, tab);
}
void launch_rollout_panda_batch(const void* tab, int n, PandaVariant variant, const RolloutPlan& p, int Kl, hipStream_t s) {
    if (variant == PANDA_LITERAL) launch_rollout_panda_batch_literal(static_cast<const BatchPandaEntry*>(tab), n, p, Kl, s);
    else launch_rollout_panda_batch_rt(static_cast<const BatchPandaEntryRT*>(tab), n, variant == PANDA_ROWS, p, Kl, s);
}

// ======================= step mode (pull and push bodies: panda_step_mode.hpp; rows and views: rollout_panda_common.hpp) ==========
// one sim.step() of every environment and the refresh of the wrapper's views in the same launch
__global__ __launch_bounds__(64) void k_psim_step(const PandaScene sc, const SimViews v, float* wd, const float* u,
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
static void launch_psim_step_literal(const PandaLaunchScene& sc, const SimViews& v, float* world, const float* u, float* u_keep,
                                        int Kl, hipStream_t s) {
    launch_psim(k_psim_step, Kl, s, *sc.lit, v, world, u, u_keep, Kl);
}

__global__ __launch_bounds__(64) void k_psim_pull(const PandaScene sc, const SimViews v, float* wd, int Kl) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Kl) return;
    psim_pull_body(sc, v, wd, Kl, i);
}
static void launch_psim_pull_literal(const PandaLaunchScene& sc, const SimViews& v, float* world, int Kl, hipStream_t s) {
    launch_psim(k_psim_pull, Kl, s, *sc.lit, v, world, Kl);
}

__global__ __launch_bounds__(64) void k_psim_push(const PandaScene sc, const SimViews v, const float* wd, int Kl) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Kl) return;
    psim_push_body(sc, v, wd, Kl, i);
}
static void launch_psim_push_literal(const PandaLaunchScene& sc, const SimViews& v, const float* world, int Kl, hipStream_t s) {
    launch_psim(k_psim_push, Kl, s, *sc.lit, v, world, Kl);
}

__global__ __launch_bounds__(64) void k_psim_cost(const PandaScene sc, const PandaCostParams cp, const float* wd,
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
    const bool env0 = env0_cube != 0;      // (the host's condition, the one m3_rollout uses for its shadow lanes)
    const int src = env0 ? ((cp.multi_modal && i >= cp.half_K) ? cp.half_K : 0) : i;
#pragma unroll
    for (int j = 0; j < 3; ++j) cube0[j] = wd[(18 + j) * Kl + (env0 ? 0 : i)];
#pragma unroll
    for (int j = 0; j < 4; ++j) qh0[j] = wd[(21 + j) * Kl + src];
    cost[i] = panda_cost(cp, w, o, k0 + i, cube0, qh0);
}
static void launch_psim_cost_literal(const PandaLaunchScene& sc, const PandaCostParams& cp, const float* world, int Kl, int k0,
                                        bool env0_cube, float* cost, hipStream_t s) {
    launch_psim(k_psim_cost, Kl, s, *sc.lit, cp, world, Kl, k0, env0_cube ? 1 : 0, cost);
}

// The launchers: PANDA_WEIGHTED has kernels of its own for the cost only -- step, pull and push read no cost, and a handle's
// weights never make m3_api.hip ask for them there.
void launch_psim_step(const PandaLaunchScene& sc, const SimViews& v, float* world, const float* u, float* u_keep, int Kl,
                      hipStream_t s) {
    switch (sc.variant) {
        case PANDA_LITERAL: return launch_psim_step_literal(sc, v, world, u, u_keep, Kl, s);
        case PANDA_ROWS: return launch_psim_step_rows(sc, v, world, u, u_keep, Kl, s);
        default: return launch_psim_step_scene(sc, v, world, u, u_keep, Kl, s);
    }
}
void launch_psim_pull(const PandaLaunchScene& sc, const SimViews& v, float* world, int Kl, hipStream_t s) {
    switch (sc.variant) {
        case PANDA_LITERAL: return launch_psim_pull_literal(sc, v, world, Kl, s);
        case PANDA_ROWS: return launch_psim_pull_rows(sc, v, world, Kl, s);
        default: return launch_psim_pull_scene(sc, v, world, Kl, s);
    }
}
void launch_psim_push(const PandaLaunchScene& sc, const SimViews& v, const float* world, int Kl, hipStream_t s) {
    switch (sc.variant) {
        case PANDA_LITERAL: return launch_psim_push_literal(sc, v, world, Kl, s);
        case PANDA_ROWS: return launch_psim_push_rows(sc, v, world, Kl, s);
        default: return launch_psim_push_scene(sc, v, world, Kl, s);
    }
}
void launch_psim_cost(const PandaLaunchScene& sc, const PandaCostParams& cp, const float* world, int Kl, int k0, bool env0_cube,
                      float* cost, hipStream_t s) {
    switch (sc.variant) {
        case PANDA_LITERAL: return launch_psim_cost_literal(sc, cp, world, Kl, k0, env0_cube, cost, s);
        case PANDA_SCENE: return launch_psim_cost_scene(sc, cp, world, Kl, k0, env0_cube, cost, s);
        case PANDA_WEIGHTED: return launch_psim_cost_weighted(sc, cp, world, Kl, k0, env0_cube, cost, s);
        case PANDA_ROWS: return launch_psim_cost_rows(sc, cp, world, Kl, k0, env0_cube, cost, s);
        case PANDA_PRIORS: return;   // (a rollout family only: the cost side never decides it, panda_variant.hpp)
    }
}

// ======================= batched closed-loop episodes (m3_panda_episodes_*) =======================
// One lane per episode e of an N-env world.  Both kernels live in this translation unit so that panda_world_from_sim,
// panda_infer_held, panda_step and panda_push_views are the same text under the same flags as in k_psim_pull / k_psim_step,
// whose sequence on a 1-env world (and on row 0 of a planner's K-env simulator) they reproduce: same arithmetic, same bits.
// (Written out, not instances of panda_step_mode.hpp's bodies: as instances their machine code moved.)

// before the command: what run_tamp's state upload and update_plan's sim.step() leave in row 0 of the planner's simulator
__global__ __launch_bounds__(64) void k_panda_episodes_pre(const PandaScene sc, const PandaEpisodeArgs a) {
    PANDA_CORNER_LDS(1);
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= a.n) return;
    if (a.st[e].phase != PE_RUNNING) return;      // (an ended episode's planner is not asked any more)
    const SimViews& v = a.v;
    PandaWorld w;
    // (1) set_dof_state_tensor / set_actor_root_state_tensor of the world's row: k_psim_pull.  Everything derived (sleep flags,
    //     warm-started impulses, contact forces) is cleared and the held latch inferred from geometry there, so NOTHING of the
    //     planner's simulator survives the upload but the velocity targets of (2)
    panda_world_from_sim(v.dof_state + (size_t)e * 18, v.root_state + (size_t)e * v.n_actors * 13,
                         v.box_actor, v.dyn_actor, v.obs_actor, w);
    panda_infer_held(sc, w);
    // (2) update_plan's sim.step(): k_psim_step under the targets that simulator holds -- on the fused path the ones the probe's
    //     step leg set last at tick 0 (m3_panda_episodes_act_first), zero before
    float uu[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) uu[j] = a.kept[(size_t)e * 9 + j];
    PandaObs obs;
    panda_step(sc, w, uu, obs, cs);
    // (3) the views after that step: what PLANNER_AIF_PANDA reads (rigid-body rows) and the fused rollout starts from (dof and
    //     root rows, m3_bind_sim_panda)
    panda_push_views(sc, a.pv, e, w);
}
// (PANDA_ROWS: a set created with M3_PANDA_EPISODES_RUNTIME -- its kernels and tables: rollout_panda_episodes_rt.hip)
void launch_panda_episodes_pre(const PandaEpisodesLaunchScene& sc, const PandaEpisodeArgs& a, hipStream_t s) {
    switch (sc.variant) {
        case PANDA_LITERAL: hipLaunchKernelGGL(k_panda_episodes_pre, dim3((a.n + 63) / 64), dim3(64), 0, s, *sc.lit, a); return;
        default: return launch_panda_episodes_pre_rows(sc, a, s);
    }
}

// after the command: trace row, the 1-env world's step (k_psim_step's body on row e), the end of an episode
__global__ __launch_bounds__(64) void k_panda_episodes_post(const PandaScene sc, const PandaEpisodeArgs a, int tick) {
    PANDA_CORNER_LDS(1);
    const int e = blockIdx.x * 64 + threadIdx.x;
    const SimViews& v = a.v;
    // everything that is not the step itself comes first and leaves nothing in registers across panda_step: from the second exit
    // on the kernel is k_psim_step
    if (e >= a.n) return;
    int op;
    {
        m3_panda_episode_status st = a.st[e];
        op = pe_advance(st, a.ended[e], tick, a.last_tick, a.settle_ticks);   // (4) panda_episode_lane.hpp
        if (op != 0) a.st[e] = st;
    }
    if (!(op & PE_OP_STEP)) return;
    float uu[9];
    {
        const float* plan = a.plan[e];
#pragma unroll
        for (int j = 0; j < 9; ++j) uu[j] = pe_target(op, plan, j);
    }
    if ((op & PE_OP_TRACE) && a.trace) {   // (5) the views BEFORE the step, the action the step runs under
        float* o = a.trace + ((size_t)tick * a.n + e) * PE_TRACE_FLOATS;
        const float* d = v.dof_state + (size_t)e * 18;
        const float* r = v.root_state + (size_t)e * v.n_actors * 13;
        const float* rb = v.rigid_body_state + (size_t)e * v.n_bodies * 13;
        for (int j = 0; j < 18; ++j) o[PE_TR_DOF + j] = d[j];
        for (int j = 0; j < PE_TR_ACTION - PE_TR_ROOT; ++j) o[PE_TR_ROOT + j] = r[j];
        for (int j = 0; j < 9; ++j) o[PE_TR_ACTION + j] = uu[j];
        for (int j = 0; j < 7; ++j) {
            o[PE_TR_HAND + j] = rb[(v.robot_body + 8) * 13 + j];     // panda_hand: link 8 of the robot's 11
            o[PE_TR_CUBE + j] = rb[v.box_body * 13 + j];
        }
    }
    // set_dof_velocity_target_tensor(action) + step(): k_psim_step on row e
    PandaWorld w;
    psoa_load(a.world, a.n, e, w);
    PandaObs obs;
    panda_step(sc, w, uu, obs, cs);
    psoa_store(a.world, a.n, e, w);
    panda_push_views(sc, v, e, w);
    // (6) no lane steps after its episode's last step (op == 0 from then on): row e of the views KEEPS the cubes' positions the
    // serial loop reads after its loops -- m3_panda_episodes_status takes them from there
}
void launch_panda_episodes_post(const PandaEpisodesLaunchScene& sc, const PandaEpisodeArgs& a, int tick, hipStream_t s) {
    switch (sc.variant) {
        case PANDA_LITERAL: hipLaunchKernelGGL(k_panda_episodes_post, dim3((a.n + 63) / 64), dim3(64), 0, s, *sc.lit, a, tick); return;
        default: return launch_panda_episodes_post_rows(sc, a, tick, s);
    }
}

}  // namespace m3
