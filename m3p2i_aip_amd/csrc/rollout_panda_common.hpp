// rollout_panda_common.hpp -- what the panda_env kernel families share (rollout_panda.hip: the reference's workspace and cost
// compiled in; rollout_panda_scene.hip, _weights.hip, _rows.hip, _batch_rt.hip: the workspace, the cost weights, a workspace
// per row as kernel arguments): the world's loads from the raw row and from the wrapper's tensors, the solver's per-lane LDS
// store, the hooks of the two shared bodies, the launch switches, the step-mode SoA rows and the refresh of the wrapper's
// views.  One text for every translation unit, so that all compile the same operations (panda_step_mode.hpp: the step-mode
// kernels' bodies).
#pragma once
#include "m3_internal.hpp"
#include "panda_dyn.hpp"
#include "panda_scene_rows.hpp"

#include <cstddef>
#include <type_traits>

namespace m3 {

// raw world, 57 floats: q9 qd9 | cubeA13 | cubeB13 | dyn-obs13 (each: pos3 quat4(xyzw) linvel3 angvel3)
__device__ __forceinline__ void body_from13(const float* b, Body& o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { o.p[i] = b[i]; o.v[i] = b[7 + i]; o.w[i] = b[10 + i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) o.q[i] = b[3 + i];
}
__device__ __forceinline__ void panda_world_clear_derived(PandaWorld& w) {
    w.held = 0.0f;
    w.rel_p[0] = w.rel_p[1] = w.rel_p[2] = 0.0f;
    w.rel_q[0] = w.rel_q[1] = w.rel_q[2] = 0.0f; w.rel_q[3] = 1.0f;
    w.awake[0] = w.awake[1] = 1.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) { w.f_table[i] = 0.0f; w.f_shelf[i] = 0.0f; w.f_cubeB[i] = 0.0f; }
#pragma unroll
    for (int i = 0; i < 4; ++i) { w.warm_t[i] = 0.0f; w.warm_l[i] = 0.0f; }
}
__device__ __forceinline__ void panda_world_from_raw(const float* p, PandaWorld& w) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { w.q[i] = p[i]; w.qd[i] = p[9 + i]; }
    body_from13(p + 18, w.A);
    body_from13(p + 31, w.B);
#pragma unroll
    for (int i = 0; i < 3; ++i) { w.obs_p[i] = p[44 + i]; w.obs_v[i] = p[51 + i]; }
    panda_world_clear_derived(w);
}

// env 0 of the wrapper's tensors: dof_state row = 9 x (pos, vel) interleaved
// (isaacgym_wrapper.py:98-100), root_state row = pos3 quat4 vel3 ang3 (:102-104)
__device__ __forceinline__ void panda_world_from_sim(const float* dof, const float* root, int ia, int ib, int io,
                                                     PandaWorld& w) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { w.q[i] = dof[2 * i]; w.qd[i] = dof[2 * i + 1]; }
    body_from13(root + (size_t)ia * 13, w.A);
    body_from13(root + (size_t)ib * 13, w.B);
    const float* o = root + (size_t)io * 13;
#pragma unroll
    for (int i = 0; i < 3; ++i) { w.obs_p[i] = o[i]; w.obs_v[i] = o[7 + i]; }
    panda_world_clear_derived(w);
}

// the per-lane store of the contact solver in LDS (manifold contact points: 120 floats per lane = 30 KB per wavefront; with one
// lane per sample also the gripper contacts' generalized rows: 312 floats, 78 KB), lane-strided: conflict-free, one wavefront
// per workgroup
#define PANDA_CORNER_LDS(LPS) __shared__ float corner_lds[panda_store_floats(LPS) * 64]; const CornerStore cs{corner_lds + threadIdx.x, 64}

__device__ __forceinline__ float in_vgpr(float v) {   // keep a uniform value in a vector register
    asm volatile("" : "+v"(v));
    return v;
}

// The kernels' `wt` (the weighted families: rollout_panda_weights.hip, rollout_panda_rows.hip) as it lies in the kernel-argument
// segment (arguments are laid out like the members of a struct), read through a pointer the compiler cannot see through: named
// as an ordinary argument, the seven floats were loaded at kernel entry and held (spilled) over the whole step loop -- eight
// scalar spills more than the twin in every rollout build.  This way each step issues its own scalar load where the cost is
// formed, and nothing of the weights lives across the substeps.
// offset of the last of the listed argument types: each argument at the next multiple of its alignment
template <class Last>
constexpr size_t kernarg_offset(size_t at) { return (at + alignof(Last) - 1) / alignof(Last) * alignof(Last); }
template <class First, class Second, class... Rest>
constexpr size_t kernarg_offset(size_t at) { return kernarg_offset<Second, Rest...>(kernarg_offset<First>(at) + sizeof(First)); }
template <size_t OFFSET>
__device__ __forceinline__ PandaCostWeights kernarg_weights() {
    typedef const char __attribute__((address_space(4)))* kernarg_bytes;
    typedef const float __attribute__((address_space(4)))* kernarg_floats;
    kernarg_floats p = (kernarg_floats)((kernarg_bytes)__builtin_amdgcn_kernarg_segment_ptr() + OFFSET);
    asm volatile("" : "+s"(p));
    return PandaCostWeights{p[0], p[1], p[2], p[3], p[4], p[5], p[6]};
}

// ---- the two hooks of the rollout body (rollout_panda_body.inc) and the reach-cost body (panda_reach_cost_body.inc) ----
// Where a step's cost is formed the bodies expand PANDA_BODY_COST(w, o, k, cube0, qh0); where the kernel-argument scene has been
// copied into `sc` and the sample index `i` is final (a_.lanes, the shadow slots and the ragged last wavefront applied) the
// rollout body expands PANDA_BODY_SCENE(sc, i).  A shell selects each hook IN FRONT OF EVERY #include of a body, by defining the
// hook's name as one of the selections below -- the only definitions there are; the body refuses to compile (#error) without a
// selection and forgets it at its end, so none leaks into the next shell of the file.
// They are macros and not callables because the rollout kernels' machine code does not survive a callable that holds or forms
// anything: with lambdas the register allocation of 4 of the 6 k_rollout_panda_s builds moved, with function objects that of 16
// of the 24 weighted builds (profiles/panda_variant_dispatch/README.md).
//
// the cost: panda_cost with the reference's literals ...
#define PANDA_COST_LITERAL(w, o, k, cube0, qh0) panda_cost(pa.cp, w, o, k, cube0, qh0)
// ... with the direct kernels' argument `wt`, read from the kernel-argument segment at the cost site (kernarg_weights, above; the
// shell names the argument's offset WT_OFFSET) ...
#define PANDA_COST_KERNARG_WEIGHTS(w, o, k, cube0, qh0) panda_cost(pa.cp, kernarg_weights<WT_OFFSET>(), w, o, k, cube0, qh0)
// ... with the weights of the table entry, read through the read-only `__restrict__` table at the cost site (never a copy taken
// before the substep loop: rollout_panda_batch_rt.hip)
#define PANDA_COST_TABLE_WEIGHTS(w, o, k, cube0, qh0) panda_cost(pa.cp, tab[blockIdx.y].wt, w, o, k, cube0, qh0)
// the scene: as the kernel received it ...
#define PANDA_SCENE_UNIFORM(sc, i)
// ... or its workspace words from row i of a per-sample table [PANDA_SCENE_ROW_WORDS][Kl] (panda_scene_rows.hpp): the direct
// kernels' argument `scene_rows`, the table entry's `rows`
#define PANDA_SCENE_KERNARG_ROWS(sc, i) panda_scene_row_load(sc, scene_rows, a_.Kl, i);
#define PANDA_SCENE_TABLE_ROWS(sc, i) panda_scene_row_load(sc, tab[blockIdx.y].rows, a_.Kl, i);
// ... or the same where the argument may be null (wave-uniform: the handle's one scene then; rollout_panda_priors.hip)
#define PANDA_SCENE_KERNARG_ROWS_OR_UNIFORM(sc, i) if (scene_rows != nullptr) panda_scene_row_load(sc, scene_rows, a_.Kl, i);
//
// The third hook, PANDA_BODY_PRIORS(part, ...): the prior samples of rollout_panda_priors.hip.  It is
// OPTIONAL -- a shell that selects nothing gets PANDA_PRIORS_NONE, which expands to nothing at each of the four places, so the
// shells from before the hook compile the tokens they compiled.  The places: SLOT(i) where `i` is final; FETCH(t) inside the
// body's `fetch`, a step ahead like nd / nm and behind them; HOLD() where the step has taken its copies cd / cm of them; SELECT(aj, j) beside
// use_best, in simple mode behind that branch's clamp.
#define PANDA_PRIORS_NONE(part, ...)
// ... with the kernel's arguments `prior_slot` ([Kl]: row of the table, -1 none) and `prior_tab` ([rows][T][9]).  The slot
// follows the SAMPLE i (the lanes of a sample, and the shadow slots of samples 0 and K / 2, read one slot and one row).  Both
// pointers are consumed ahead of the step loop: what the loop keeps is the lane's row pointer (null: no prior), in vector
// registers.  A prior lane has no use for its noise row -- whatever the mode and the sampler, its control never reads `cd` -- so
// the nine values of the next step are fetched INTO `nd`, behind the body's own load, and cost no register across the step
// (with registers of their own the one-lane builds, which sit at the 512-register limit, spilled 8 and 18 more vector
// registers to scratch than their twins).  HOLD takes them out of `cd` before the random sampler overwrites it.  No branch
// around the step: lanes without a prior skip the loads and keep their `aj`.
#define PANDA_PRIORS_KERNARG(part, ...) PANDA_PRIORS_KERNARG_##part(__VA_ARGS__)
#define PANDA_PRIORS_KERNARG_SLOT(i)                                                                                       \
    const int prior_row = prior_slot[i];                                                                                   \
    const float* const prow = prior_row < 0 ? nullptr : prior_tab + (size_t)prior_row * (size_t)(a_.T * 9);
#define PANDA_PRIORS_KERNARG_FETCH(t)                                                                                      \
    if (prow != nullptr) {                                                                                                 \
        _Pragma("unroll") for (int j = 0; j < 9; ++j) nd[j] = prow[(t) * 9 + j];                                           \
    }
#define PANDA_PRIORS_KERNARG_HOLD()                                                                                        \
    float pcur[9];                                                                                                         \
    _Pragma("unroll") for (int j = 0; j < 9; ++j) pcur[j] = cd[j];
#define PANDA_PRIORS_KERNARG_SELECT(aj, j) aj = prow != nullptr ? fmaxf(fminf(pcur[j], a.u_max[j]), a.u_min[j]) : aj;

// k_panda_reach_cost (rollout_panda.hip) and its weighted twin (rollout_panda_weights.hip)
constexpr int RC_TS = 4, RC_CH = 32;      // time slices per workgroup; steps per LDS chunk

// ---- host: the launch switches, written once ----
// The GENERAL x FORCES x LPS instance of a rollout kernel family for a plan: pick(forces, general, lps) -- a generic lambda over
// three std::integral_constant -- names the family's kernel (only the literal family has GENERAL = false builds; the others
// ignore `general`), args are the kernel's.  (The kernels are instantiated in the order this switch names them -- lanes per
// sample, then GENERAL, then FORCES -- and that order is the layout of the code object.)
template <class Pick, class... Args>
void launch_panda_instance(const RolloutPlan& p, dim3 grid, hipStream_t s, Pick pick, const Args&... args) {
    using std::false_type;
    using std::true_type;
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(64), 0, s, args...); };
    auto with_lps = [&](auto lps) {
        if (p.general) {
            if (p.forces) launch(pick(true_type{}, true_type{}, lps));
            else launch(pick(false_type{}, true_type{}, lps));
        } else if (p.forces) launch(pick(true_type{}, false_type{}, lps));
        else launch(pick(false_type{}, false_type{}, lps));
    };
    if (p.lps == 16) with_lps(std::integral_constant<int, 16>{});
    else if (p.lps == 8) with_lps(std::integral_constant<int, 8>{});
    else with_lps(std::integral_constant<int, 1>{});
}
// the reach-cost kernel behind a rollout that kept the record buffer: n handles of K_local = Kl (a direct launch: one)
template <class Kernel, class... Args>
void launch_panda_reach_cost(Kernel kernel, int Kl, int n, hipStream_t s, const Args&... args) {
    hipLaunchKernelGGL(kernel, dim3((Kl + 63) / 64, n), dim3(64 * RC_TS), 0, s, args...);
}
// a step-mode kernel: one lane per environment
template <class Kernel, class... Args>
void launch_psim(Kernel kernel, int Kl, hipStream_t s, const Args&... args) {
    hipLaunchKernelGGL(kernel, dim3((Kl + 63) / 64), dim3(64), 0, s, args...);
}

// The launchers of m3_internal.hpp (rollout_panda.hip) forward by variant to the translation unit that holds the family's
// kernels -- there is no relocatable device code: a kernel is launched where it is defined.  One signature per operation, every
// family's part of it takes what it needs from the PandaLaunchScene (the literal parts are local to rollout_panda.hip).
// (the rollout kernel alone, a.lanes the plan's)
using PandaRolloutLaunch = void(const RolloutArgs& a, const PandaArgs& pa, const PandaLaunchScene& sc, const RolloutPlan& p, hipStream_t s);
PandaRolloutLaunch launch_rollout_panda_scene, launch_rollout_panda_weighted, launch_rollout_panda_rows, launch_rollout_panda_priors;
// (the reach-cost kernel reads no scene: the literal one and this one serve every family)
void launch_panda_reach_cost_weighted(const RolloutArgs& a, const PandaArgs& pa, const PandaLaunchScene& sc, hipStream_t s);
// (the table's run-time section: kb_rollout_panda_w, with per_sample kb_rollout_panda_v, + the weighted reach-cost kernel)
void launch_rollout_panda_batch_rt(const BatchPandaEntryRT* tab, int n, bool per_sample, const RolloutPlan& p, int Kl, hipStream_t s);
using PsimStepLaunch = void(const PandaLaunchScene& sc, const SimViews& v, float* world, const float* u, float* u_keep, int Kl, hipStream_t s);
using PsimPullLaunch = void(const PandaLaunchScene& sc, const SimViews& v, float* world, int Kl, hipStream_t s);
using PsimPushLaunch = void(const PandaLaunchScene& sc, const SimViews& v, const float* world, int Kl, hipStream_t s);
using PsimCostLaunch = void(const PandaLaunchScene& sc, const PandaCostParams& cp, const float* world, int Kl, int k0, bool env0_cube,
                            float* cost, hipStream_t s);
PsimStepLaunch launch_psim_step_scene, launch_psim_step_rows;
PsimPullLaunch launch_psim_pull_scene, launch_psim_pull_rows;
PsimPushLaunch launch_psim_push_scene, launch_psim_push_rows;
PsimCostLaunch launch_psim_cost_scene, launch_psim_cost_weighted, launch_psim_cost_rows;
// (the lockstep episodes' pre and post kernels on the set's tables: rollout_panda_episodes_rt.hip)
void launch_panda_episodes_pre_rows(const PandaEpisodesLaunchScene& sc, const PandaEpisodeArgs& a, hipStream_t s);
void launch_panda_episodes_post_rows(const PandaEpisodesLaunchScene& sc, const PandaEpisodeArgs& a, int tick, hipStream_t s);

// ======================= step mode ======================================================
// SoA world rows (NWP = 77): q 0-8 | qd 9-17 | cubeA 18-30 (pos3 quat4 vel3 angvel3) | cubeB 31-43 | plate pos 44-46,
// vel 47-49 | held 50 | rel_p 51-53 | rel_q 54-57 | awake 58-59 | f_table 60-62 | f_shelf 63-65 | f_cubeB 66-68 |
// warm_t 69-72 | warm_l 73-76
__device__ __forceinline__ void psoa_load(const float* wd, int Kl, int i, PandaWorld& w) {
    const float* p = wd + i;
    auto body = [&](int r0, Body& b) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { b.p[j] = p[(r0 + j) * Kl]; b.v[j] = p[(r0 + 7 + j) * Kl]; b.w[j] = p[(r0 + 10 + j) * Kl]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) b.q[j] = p[(r0 + 3 + j) * Kl];
    };
#pragma unroll
    for (int j = 0; j < 9; ++j) { w.q[j] = p[j * Kl]; w.qd[j] = p[(9 + j) * Kl]; }
    body(18, w.A);
    body(31, w.B);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        w.obs_p[j] = p[(44 + j) * Kl]; w.obs_v[j] = p[(47 + j) * Kl]; w.rel_p[j] = p[(51 + j) * Kl];
        w.f_table[j] = p[(60 + j) * Kl]; w.f_shelf[j] = p[(63 + j) * Kl]; w.f_cubeB[j] = p[(66 + j) * Kl];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { w.rel_q[j] = p[(54 + j) * Kl]; w.warm_t[j] = p[(69 + j) * Kl]; w.warm_l[j] = p[(73 + j) * Kl]; }
    w.held = p[50 * Kl];
    w.awake[0] = p[58 * Kl]; w.awake[1] = p[59 * Kl];
}
__device__ __forceinline__ void psoa_store(float* wd, int Kl, int i, const PandaWorld& w) {
    float* p = wd + i;
    auto body = [&](int r0, const Body& b) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { p[(r0 + j) * Kl] = b.p[j]; p[(r0 + 7 + j) * Kl] = b.v[j]; p[(r0 + 10 + j) * Kl] = b.w[j]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) p[(r0 + 3 + j) * Kl] = b.q[j];
    };
#pragma unroll
    for (int j = 0; j < 9; ++j) { p[j * Kl] = w.q[j]; p[(9 + j) * Kl] = w.qd[j]; }
    body(18, w.A);
    body(31, w.B);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        p[(44 + j) * Kl] = w.obs_p[j]; p[(47 + j) * Kl] = w.obs_v[j]; p[(51 + j) * Kl] = w.rel_p[j];
        p[(60 + j) * Kl] = w.f_table[j]; p[(63 + j) * Kl] = w.f_shelf[j]; p[(66 + j) * Kl] = w.f_cubeB[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { p[(54 + j) * Kl] = w.rel_q[j]; p[(69 + j) * Kl] = w.warm_t[j]; p[(73 + j) * Kl] = w.warm_l[j]; }
    p[50 * Kl] = w.held;
    p[58 * Kl] = w.awake[0]; p[59 * Kl] = w.awake[1];
}

// SoA world of environment i -> the wrapper's views (link poses through the forward kinematics)
template <class SC>
__device__ __forceinline__ void panda_push_views(const SC& sc, const SimViews& v, int i, const PandaWorld& w) {
    if (v.dof_state) {
        float* d = v.dof_state + (size_t)i * 18;
#pragma unroll
        for (int j = 0; j < 9; ++j) { d[2 * j] = w.q[j]; d[2 * j + 1] = w.qd[j]; }
    }
    auto body13 = [&](const Body& b, float* o) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { o[j] = b.p[j]; o[7 + j] = b.v[j]; o[10 + j] = b.w[j]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) o[3 + j] = b.q[j];
    };
    if (v.root_state) {
        float* base = v.root_state + (size_t)i * v.n_actors * 13;
        body13(w.A, base + v.box_actor * 13);
        body13(w.B, base + v.dyn_actor * 13);
        float* o = base + v.obs_actor * 13;      // the plate: position and linear velocity (it does not rotate)
#pragma unroll
        for (int j = 0; j < 3; ++j) { o[j] = w.obs_p[j]; o[7 + j] = w.obs_v[j]; }
    }
    if (v.rigid_body_state) {
        float* base = v.rigid_body_state + (size_t)i * v.n_bodies * 13;
        body13(w.A, base + v.box_body * 13);
        body13(w.B, base + v.dyn_body * 13);
        float* o = base + v.obs_body * 13;
#pragma unroll
        for (int j = 0; j < 3; ++j) { o[j] = w.obs_p[j]; o[7 + j] = w.obs_v[j]; }
        // robot links: bodies robot_body .. robot_body + 10 (link0..7, hand, left, right)
        float links[11 * 7];
        Frame hand;
        float pl[3], pr[3];
        panda_fk<true>(sc, w.q, hand, pl, pr, links);
        for (int l = 0; l < 11; ++l) {
            float* ol = base + (v.robot_body + l) * 13;
            for (int j = 0; j < 7; ++j) ol[j] = links[l * 7 + j];
            for (int j = 7; j < 13; ++j) ol[j] = 0.0f;  // link velocities are not reported
        }
    }
    if (v.net_contact_force) {
        float* f = v.net_contact_force + (size_t)i * v.n_bodies * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            f[v.table_body * 3 + j] = w.f_table[j];
            f[v.shelf_body * 3 + j] = w.f_shelf[j];
            f[v.dyn_body * 3 + j] = w.f_cubeB[j];
        }
    }
}

}  // namespace m3
