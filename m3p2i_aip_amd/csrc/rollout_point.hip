// rollout_point.hip -- point_env rollout: launch dispatch, the all-modes instance of the kernel
// (rollout_point_kernel.hpp), the noise transpose and the step-mode (IsaacGymWrapper-like) kernels.
#include "rollout_point_kernel.hpp"
#include "episode_lane.hpp"
#include "point_step_mode.hpp"

namespace m3 {

// lanes per wavefront.  MEASURED on MI355X (tools/lanes_sweep.py, DESIGN.md "Lanes per
// wavefront"): full 64-lane waves are never slower -- K=2000: 0.38 ms at 64 lanes vs 0.83 ms
// at 1 lane (2000 waves), K=10000: 0.36 ms vs 3.3 ms.  Narrow waves do execute ~2x fewer
// instructions each (no divergence), but the kernel ends with its SLOWEST wave, whose
// contact-heavy sample runs the same long path either way, and co-resident waves on a CU
// slow each other down.  So the automatic choice is 64; the knob stays for experiments.
int rollout_lanes_for(int Kl) {
    (void)Kl;
    return 64;
}

// The form of a launch.  Instance -1: the general instance (every sampler mode, task at run time); 0..3: the instance with
// the reference's default sampler and that task compiled in (rollout_point_task*.hip).  Only the general and the push_pull
// instances carry the epilogue that leaves the workgroups' cost minima (rollout_point_kernel.hpp).
// variant POINT_WEIGHTED: the handle's cost weights are not the defaults (or the weighted instance is forced on): the general
// instance with point_cost_w, whatever the sampler and the task.
// form_request: the two-wavefront form (RolloutPlan::form = 1) exists for the navigation and push instances in the builds with
// one resident wavefront per SIMD, with the default weights and a horizon whose tables fit its LDS; 1 takes it wherever it
// exists, -1 where rollout_companion_pays as well, 0 never (m3_batch_command, the episode paths).
// variant POINT_SCENE: the handle's arena is not the default (or the run-time-scene build is forced on): the general instance on
// PointSceneRT, which always takes the weights as well -- instance -1, form 0, ref 0, whatever the sampler, the task and the weights.
// per_sample: the same build with the arena of each lane read from the handle's table (m3_set_point_rollout_scenes): scene = 2.
// priors: the prior build of either (m3_set_prior_samples, rollout_point_priors.hip; the caller passes POINT_SCENE): priors = 1.
RolloutPlan plan_rollout_point(const RolloutArgs& a, const PointScene& sc, PointVariant variant, int form_request, bool per_sample,
                               bool priors) {
    const bool weighted = variant != POINT_PLAIN;
    if (variant == POINT_SCENE) {
        RolloutPlan p{};
        p.scene = per_sample ? 2 : 1; p.weighted = 1;
        p.priors = priors ? 1 : 0;
        p.instance = -1; p.ref = 0; p.form = 0;
        p.lanes = a.lanes;
        p.blocks = (a.Kl + a.lanes - 1) / a.lanes;
        p.rows = a.wave_min ? p.blocks : 0;
        return p;
    }
#if defined(M3_ABL_GENERAL_ONLY) || defined(M3_ABL_COUNT) || defined(M3_ABL_PHASES)   // (experiments: one kernel for all modes;
    // the instrumented builds keep their counters in this translation unit)
    const bool general = true;
#else
    // push_pull without multi_modal is refused upstream (m3_rollout); a task outside 0..3 cannot reach here
    const bool general = a.sampling_random || a.mode_simple || a.cp.task < 0 || a.cp.task > 3 ||
                         (a.cp.task == 3 && !a.multi_modal) || a.scale_dev != nullptr /* update_cov */ ||
                         a.cp.avoid_dyn_obs != 0 /* the extension: the dyn-obs contact force must be formed */ ||
                         weighted /* the extension: only the general instance has a weighted build */;
#endif
    RolloutPlan p{};
    p.weighted = weighted ? 1 : 0;
    p.instance = general ? -1 : a.cp.task;
    p.ref = point_scene_is_reference(sc) ? 1 : 0;
    p.lanes = a.lanes;
    p.blocks = (a.Kl + a.lanes - 1) / a.lanes;
    p.rows = (a.wave_min && (p.instance == -1 || p.instance == 3)) ? p.blocks : 0;
    const RolloutBuild build = rollout_point_build(p.blocks, p.ref != 0);
    const bool exists = (p.instance == 0 || p.instance == 1) && !weighted && (build == BUILD_LONE || build == BUILD_LONE_REF) &&
                        rollout_point2_fits(a.T);
    p.form = (exists && (form_request == 1 || (form_request < 0 && rollout_companion_pays(p.blocks)))) ? 1 : 0;
    return p;
}

void launch_rollout_point(const RolloutArgs& a, const PointScene& sc, const PointSceneRT& rt, const PointCostWeights& wt,
                          const RolloutPlan& p, hipStream_t s, int* err, const float* scene_rows, const int* prior_slot,
                          const float* prior_tab) {
    switch (point_variant(p)) {
        case POINT_SCENE:
            if (p.priors) launch_rollout_point_pr(a, rt, p.scene == 2 ? scene_rows : nullptr, wt, prior_slot, prior_tab, p.blocks, s);
            else if (p.scene == 2) launch_rollout_point_sv(a, rt, scene_rows, wt, p.blocks, s);
            else launch_rollout_point_instance<true, -1>(a, rt, p.blocks, s, wt);
            return;
        case POINT_WEIGHTED: launch_rollout_point_instance<true, -1>(a, sc, p.blocks, s, wt); return;
        default: break;
    }
    if (p.form == 1) {
        if (p.instance == 0) launch_rollout_point_nav2(a, sc, p.blocks, err, s);
        else launch_rollout_point_push2(a, sc, p.blocks, err, s);
        return;
    }
    switch (p.instance) {
        case -1: launch_rollout_point_instance<true, -1>(a, sc, p.blocks, s); break;
        case 0: launch_rollout_point_nav(a, sc, p.blocks, s); break;
        case 1: launch_rollout_point_push(a, sc, p.blocks, s); break;
        case 2: launch_rollout_point_pull(a, sc, p.blocks, s); break;
        default: launch_rollout_point_pushpull(a, sc, p.blocks, s); break;
    }
}

void launch_rollout_point_batch(const void* tab, int n, const RolloutPlan& p, hipStream_t s) {
    const bool ref = p.ref != 0;
    switch (point_variant(p)) {
        case POINT_SCENE:
            if (p.priors) launch_rollout_point_pr_batch(static_cast<const BatchRolloutEntryPR*>(tab), p.blocks, n, s);
            else if (p.scene == 2) launch_rollout_point_sv_batch(static_cast<const BatchRolloutEntrySV*>(tab), p.blocks, n, s);
            else launch_rollout_point_batch_instance<true, -1>(static_cast<const BatchRolloutEntryS*>(tab), p.blocks, n, ref, s);
            return;
        case POINT_WEIGHTED:
            launch_rollout_point_batch_instance<true, -1>(static_cast<const BatchRolloutEntryW*>(tab), p.blocks, n, ref, s);
            return;
        default: break;
    }
    const BatchRolloutEntry* plain = static_cast<const BatchRolloutEntry*>(tab);
    switch (p.instance) {
        case -1: launch_rollout_point_batch_instance<true, -1>(plain, p.blocks, n, ref, s); break;
        case 0: launch_rollout_point_nav_batch(plain, p.blocks, n, ref, s); break;
        case 1: launch_rollout_point_push_batch(plain, p.blocks, n, ref, s); break;
        case 2: launch_rollout_point_pull_batch(plain, p.blocks, n, ref, s); break;
        default: launch_rollout_point_pushpull_batch(plain, p.blocks, n, ref, s); break;
    }
}

// delta [K][T][nu] (reference layout) -> [T][K][nu]
__global__ void k_transpose_noise(const float* __restrict__ src, float* __restrict__ dst, int K,
                                  int T, int nu) {
    const size_t n = (size_t)K * T * nu;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < n;
         o += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(o % nu);
        const size_t r = o / nu;
        const int k = (int)(r % K);
        const int t = (int)(r / K);
        dst[o] = src[((size_t)k * T + t) * nu + j];
    }
}
void launch_transpose_noise(const float* src, float* dst, int K, int T, int nu, hipStream_t s) {
    const size_t n = (size_t)K * T * nu;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_transpose_noise, dim3(blocks), dim3(256), 0, s, src, dst, K, T, nu);
}

// ======================= step mode (IsaacGymWrapper-like surface) =======================
__global__ __launch_bounds__(64) void k_sim_step(const PointScene sc, const SimViews v, float* wd, const float* u,
                                                 float* u_keep, int Kl) {
    sim_step_body(sc, v, wd, u, u_keep, Kl);
}
void launch_sim_step(const PointScene& sc, const SimViews& v, float* world, const float* u, float* u_keep, int Kl,
                     hipStream_t s) {
    hipLaunchKernelGGL(k_sim_step, dim3((Kl + 63) / 64), dim3(64), 0, s, sc, v, world, u, u_keep, Kl);
}

// (two hand-written kernels: as instances of one templated body, k_sim_cost came out with the operands of one v_add_f32 swapped)
__global__ void k_sim_cost(const CostParams cp, float* wd, int Kl, int k0, float* cost) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Kl) return;
    PointWorld w;
    soa_load(wd, Kl, i, w);
    cost[i] = point_cost(cp, w, k0 + i);
    float* p = wd + i;  // only the pending force changes
    p[18 * Kl] = w.fRx; p[19 * Kl] = w.fRy; p[20 * Kl] = w.fBx; p[21 * Kl] = w.fBy;
}
// ... with the handle's cost weights (m3_set_point_cost_weights): what the weighted rollout evaluates after each step
__global__ void k_sim_cost_w(const CostParams cp, const PointCostWeights wt, float* wd, int Kl, int k0, float* cost) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Kl) return;
    PointWorld w;
    soa_load(wd, Kl, i, w);
    cost[i] = point_cost_w(cp, wt, w, k0 + i);
    float* p = wd + i;  // only the pending force changes
    p[18 * Kl] = w.fRx; p[19 * Kl] = w.fRy; p[20 * Kl] = w.fBx; p[21 * Kl] = w.fBy;
}
void launch_sim_cost(const CostParams& cp, const PointCostWeights* wt, float* world, int Kl, int k0, float* cost, hipStream_t s) {
    const dim3 grid((Kl + 255) / 256), wg(256);
    if (wt) hipLaunchKernelGGL(k_sim_cost_w, grid, wg, 0, s, cp, *wt, world, Kl, k0, cost);
    else hipLaunchKernelGGL(k_sim_cost, grid, wg, 0, s, cp, world, Kl, k0, cost);
}

// wrapper views (AoS, torch-owned) -> SoA world.  dof_state row = [x, vx, y, vy]
// (isaacgym_wrapper.py:120-126); root_state row = pos3 quat4(xyzw) linvel3 angvel3 (:102-104)
__device__ __forceinline__ void pull_env(const SimViews& v, float* wd, int Kl, int i) {
    float* p = wd + i;
    const float* d = v.dof_state + (size_t)i * 4;
    p[0 * Kl] = d[0]; p[1 * Kl] = d[2]; p[2 * Kl] = d[1]; p[3 * Kl] = d[3];
    for (int b = 0; b < 2; ++b) {
        const float* r = v.root_state + ((size_t)i * v.n_actors + (b == 0 ? v.box_actor : v.dyn_actor)) * 13;
        const int o = 4 + b * 7;
        float c, s;
        yaw_from_quat(r[5], r[6], &c, &s);
        p[(o + 0) * Kl] = r[0]; p[(o + 1) * Kl] = r[1];
        p[(o + 2) * Kl] = c; p[(o + 3) * Kl] = s;
        p[(o + 4) * Kl] = r[7]; p[(o + 5) * Kl] = r[8]; p[(o + 6) * Kl] = r[12];
    }
}
__global__ void k_sim_pull(const SimViews v, float* wd, int Kl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Kl) return;
    pull_env(v, wd, Kl, i);
}
// update_dyn_obs (isaacgym_wrapper.py:205-220): one actor's root position shifted in the wrapper's root_state
// view + set_actor_root_state_tensor, in one launch
__global__ void k_sim_shift_pull(const SimViews v, float* wd, int Kl, int actor, float dx, float dy, float dz) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Kl) return;
    float* r = v.root_state + ((size_t)i * v.n_actors + actor) * 13;
    r[0] = r[0] + dx; r[1] = r[1] + dy; r[2] = r[2] + dz;
    pull_env(v, wd, Kl, i);
}
void launch_sim_shift_pull(const SimViews& v, float* world, int Kl, int actor, float dx, float dy, float dz, hipStream_t s) {
    hipLaunchKernelGGL(k_sim_shift_pull, dim3((Kl + 255) / 256), dim3(256), 0, s, v, world, Kl, actor, dx, dy, dz);
}
void launch_sim_pull(const SimViews& v, float* world, int Kl, hipStream_t s) {
    hipLaunchKernelGGL(k_sim_pull, dim3((Kl + 255) / 256), dim3(256), 0, s, v, world, Kl);
}

__global__ void k_sim_push(const SimViews v, const float* wd, int Kl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Kl) return;
    PointWorld w;
    soa_load(wd, Kl, i, w);
    push_views(v, i, w);
}
void launch_sim_push(const SimViews& v, const float* world, int Kl, hipStream_t s) {
    hipLaunchKernelGGL(k_sim_push, dim3((Kl + 255) / 256), dim3(256), 0, s, v, world, Kl);
}

// apply_rigid_body_force_tensors: only the box and the robot's last link take forces in
// the reference's use (skill_utils.py:86-90); xy components, consumed by the next step.
__global__ void k_sim_forces(const SimViews v, float* wd, const float* f, int Kl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Kl) return;
    const float* fi = f + (size_t)i * v.n_bodies * 3;
    float* p = wd + i;
    p[18 * Kl] = fi[v.robot_body * 3 + 0]; p[19 * Kl] = fi[v.robot_body * 3 + 1];
    p[20 * Kl] = fi[v.box_body * 3 + 0];   p[21 * Kl] = fi[v.box_body * 3 + 1];
}
void launch_sim_forces(const SimViews& v, float* world, const float* f, int Kl, hipStream_t s) {
    hipLaunchKernelGGL(k_sim_forces, dim3((Kl + 255) / 256), dim3(256), 0, s, v, world, f, Kl);
}

// The 1-env "real world" side of scripts/sim.py:41-49: suction between the robot and the box
// (behaves like utils/skill_utils.py:36-94), evaluated on the wrapper's environments without a
// host round trip.
//   forces != null : calculate_suction -- the [Kl][nB][3] body-force tensor (zero except the box
//                    row and the LAST body's row, +-kp * unit(box - robot) clamped to +-500, only
//                    where 1/|box - robot| exceeds `thresh`)
//   action != null : check_suction_condition -- robot within `reach` of the box and the commanded
//                    velocity pointing away from it -- and, if `apply`, the force of above staged
//                    as the pending external force of the next step (apply_rigid_body_force_tensors)
//   gate != null   : a device flag (the planner's pull preference, m3_info.pull_preference) that must be
//                    non-zero for the suction to act: cfg.suction_active without a host round trip
__global__ void k_sim_suction(const SimViews v, float* wd, int Kl, float kp, float thresh, float reach,
                              const float* action, int apply, float* forces, int* flags, const int* gate) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Kl) return;
    const bool enabled = gate ? (*gate != 0) : true;
    float* p = wd + i;
    const float ex = p[4 * Kl] - p[0 * Kl], ey = p[5 * Kl] - p[1 * Kl];   // robot -> box
    const float len = sqrtf(ex * ex + ey * ey);
    const float inv = 1.0f / len;
    float fx = 0.0f, fy = 0.0f;                                          // force on the robot
    if (inv > thresh) {
        fx = clamp500(kp * (ex * inv));
        fy = clamp500(kp * (ey * inv));
    }
    if (forces) {
        float* f = forces + (size_t)i * v.n_bodies * 3;
        for (int q = 0; q < v.n_bodies * 3; ++q) f[q] = 0.0f;
        f[v.box_body * 3 + 0] = -fx; f[v.box_body * 3 + 1] = -fy;
        f[(v.n_bodies - 1) * 3 + 0] = fx; f[(v.n_bodies - 1) * 3 + 1] = fy;
    }
    if (action) {
        const float along = action[2 * i] * (-ex) + action[2 * i + 1] * (-ey);   // action . (robot - box)
        const bool pulling = enabled && len < reach && along > 0.0f;
        if (flags) flags[i] = pulling ? 1 : 0;
        if (pulling && apply) {
            p[18 * Kl] = fx; p[19 * Kl] = fy; p[20 * Kl] = -fx; p[21 * Kl] = -fy;
        }
    }
}
void launch_sim_suction(const SimViews& v, float* world, int Kl, float kp, float thresh, float reach,
                        const float* action, int apply, float* forces, int* flags, const int* gate, hipStream_t s) {
    hipLaunchKernelGGL(k_sim_suction, dim3((Kl + 255) / 256), dim3(256), 0, s, v, world, Kl, kp, thresh, reach,
                       action, apply, forces, flags, gate);
}

// ======================= batched closed-loop episodes (m3_episodes_*) =======================
// One lane per episode e of an N-env world; lane e does for row e exactly what tools/closed_loop.run does for its 1-env
// world at one tick, in the same order.  The expressions shared with k_sim_shift_pull / k_sim_suction / k_sim_step are
// the same code or the same text in this translation unit, so they compile to the same arithmetic.

// before the command: dyn-obs walk with the episode's phase, success test, suction-gate snapshot
__global__ __launch_bounds__(64) void k_episodes_pre(const EpisodeArgs a, int tick) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= a.n) return;
    const SimViews& v = a.v;
    const EpisodeLane L = a.lane[e];
    // update_dyn_obs(tick + phase): k_sim_shift_pull on row e, with this episode's own phase
    const float d = ep_walk_forth(tick + L.phase) ? 0.01f : -0.01f;
    float* r = v.root_state + ((size_t)e * v.n_actors + v.dyn_actor) * 13;
    r[0] = r[0] + d; r[1] = r[1] + d; r[2] = r[2] + 0.0f;
    pull_env(v, a.world, a.n, e);
    m3_episode_status& st = a.st[e];
    if (st.done_tick < 0) {
        // check_task_success on the wrapper's views: robot_pos (dof_state x, y) for navigation, else the box's root x, y.
        // A success ends the episode before its command; its metrics freeze here.
        float px, py;
        if (L.task == 0) {
            px = v.dof_state[(size_t)e * 4 + 0]; py = v.dof_state[(size_t)e * 4 + 2];
        } else {
            const float* b = v.root_state + ((size_t)e * v.n_actors + v.box_actor) * 13;
            px = b[0]; py = b[1];
        }
        if (ep_success(L.task, px, py, L.gx, L.gy)) {
            // (d) the final error is taken on the host from these f32 positions, as closed_loop.run does with CPU torch
            st.done_tick = tick; st.success = 1; st.final_pos[0] = px; st.final_pos[1] = py;
        }
    }
    // (b) gate of this tick = the previous command's pull preference: read it before this tick's command rewrites it
    a.gate[e] = ep_gate(L.suction, L.pref ? *L.pref : 0);
}
void launch_episodes_pre(const EpisodeArgs& a, int tick, hipStream_t s) {
    hipLaunchKernelGGL(k_episodes_pre, dim3((a.n + 63) / 64), dim3(64), 0, s, a, tick);
}

// after the command: trace row, suction, step + views, collision count, the last tick's end
// (g) not masked: an episode that is done keeps its row evolving (on its last plan); nothing of it is recorded any more
__global__ __launch_bounds__(64) void k_episodes_post(const PointScene sc, const EpisodeArgs a, int tick) {
    episodes_post_body(sc, a, tick);
}
void launch_episodes_post(const PointScene& sc, const EpisodeArgs& a, int tick, hipStream_t s) {
    hipLaunchKernelGGL(k_episodes_post, dim3((a.n + 63) / 64), dim3(64), 0, s, sc, a, tick);
}

}  // namespace m3

// Diagnostic (host only, no device call): the form plan_rollout_point gives a point_env rollout with these settings -- what
// m3_rollout / m3_batch_command would launch.  out: instance, ref, form, weighted, scene, blocks, rows, lanes.
static int point_rollout_plan(int task, int multi_modal, int mode_simple, int sampling_random, int avoid_dyn_obs,
                              int K_local, int T, int lanes, float dt, int substeps, int solver_iters, int weighted,
                              int scene, int form_request, int want_minima, int priors, int* out, int* out9) {
    if (!out || K_local < 1 || T < 1 || lanes < 1 || lanes > 64 || substeps < 1) return M3_ERR_BAD_ARG;
    m3::RolloutArgs a{};
    a.Kl = a.Kg = K_local; a.T = T; a.nu = 2; a.lanes = lanes;
    a.multi_modal = multi_modal; a.mode_simple = mode_simple; a.sampling_random = sampling_random;
    a.cp.task = task; a.cp.multi_modal = multi_modal; a.cp.avoid_dyn_obs = avoid_dyn_obs;
    static float minima_stand_in[3];
    a.wave_min = want_minima ? minima_stand_in : nullptr;   // (only tested against null)
    m3::PointScene sc;
    m3::make_point_scene(sc, dt, substeps, solver_iters);
    if (scene < 0 || scene > 2) return M3_ERR_BAD_ARG;
    if (priors < 0 || priors > 1 || (priors && !scene)) return M3_ERR_BAD_ARG;
    const m3::PointVariant variant = scene ? m3::POINT_SCENE : weighted ? m3::POINT_WEIGHTED : m3::POINT_PLAIN;
    const m3::RolloutPlan p = m3::plan_rollout_point(a, sc, variant, form_request, scene == 2, priors != 0);
    out[0] = p.instance; out[1] = p.ref; out[2] = p.form; out[3] = p.weighted; out[4] = p.scene; out[5] = p.blocks;
    out[6] = p.rows; out[7] = p.lanes;
    if (out9) out9[8] = p.priors;
    return M3_OK;
}
extern "C" int m3_point_rollout_plan(int task, int multi_modal, int mode_simple, int sampling_random, int avoid_dyn_obs,
                                     int K_local, int T, int lanes, float dt, int substeps, int solver_iters, int weighted,
                                     int scene, int form_request, int want_minima, int out[8]) {
    return point_rollout_plan(task, multi_modal, mode_simple, sampling_random, avoid_dyn_obs, K_local, T, lanes, dt, substeps,
                              solver_iters, weighted, scene, form_request, want_minima, 0, out, nullptr);
}
// ... of a handle with prior samples (m3_set_prior_samples): out[8] = priors
extern "C" int m3_point_rollout_plan_ex(int task, int multi_modal, int mode_simple, int sampling_random, int avoid_dyn_obs,
                                        int K_local, int T, int lanes, float dt, int substeps, int solver_iters, int weighted,
                                        int scene, int form_request, int want_minima, int priors, int out[9]) {
    return point_rollout_plan(task, multi_modal, mode_simple, sampling_random, avoid_dyn_obs, K_local, T, lanes, dt, substeps,
                              solver_iters, weighted, scene, form_request, want_minima, priors, out, out);
}

#ifdef M3_ABL_PHASES
extern "C" void m3_dbg_phases(unsigned long long* out, int reset) {
    if (reset) { static unsigned long long z[1024 * 8]; (void)hipMemcpyToSymbol(HIP_SYMBOL(m3::g_phase), z, sizeof(z)); }
    else (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(m3::g_phase), 1024 * 8 * sizeof(unsigned long long));
}
#endif
#ifdef M3_ABL_COUNT
extern "C" void m3_dbg_levels(unsigned int* out, int reset) {
    if (reset) { static unsigned int z[512]; (void)hipMemcpyToSymbol(HIP_SYMBOL(m3::g_lvl), z, sizeof(z)); }
    else (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(m3::g_lvl), 512 * sizeof(unsigned int));
}
extern "C" void m3_dbg_cycles(unsigned int* out, int reset) {
    if (reset) { static unsigned int z[64 * 16]; (void)hipMemcpyToSymbol(HIP_SYMBOL(m3::g_cyc), z, sizeof(z)); }
    else (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(m3::g_cyc), 64 * 16 * sizeof(unsigned int));
}
#endif
