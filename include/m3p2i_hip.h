/*
 * m3p2i_hip.h -- C-ABI of libm3p2i_hip.so: the MI355X (gfx950) implementation of the
 * MPPI / M3P2I command() hot path of tud-amr/m3p2i-aip.
 *
 * The reference is pure Python; the "FFI" a maintainer binds is ctypes (see
 * INTEGRATION.md).  Each entry point names the reference interface it replaces
 * (paths relative to the reference repository root):
 *
 *   m3_create / m3_destroy      MPPI.__init__ / M3P2I.__init__
 *                                 src/m3p2i_aip/planners/motion_planner/mppi.py:82-203,
 *                                 m3p2i.py:5-8; IsaacGymWrapper.__init__/start_sim
 *                                 src/m3p2i_aip/utils/isaacgym_utils/isaacgym_wrapper.py:39-90
 *   m3_set_noise                MPPI.get_samples (cached Halton-spline delta) mppi.py:458-483
 *   m3_set_objective            Objective.update_objective cost_functions.py:15-17,
 *                                 M3P2I.update_gripper_command m3p2i.py:10-14
 *   m3_set_world / m3_bind_sim  run_tamp state upload scripts/reactive_tamp.py:45-48
 *                                 (set_dof_state_tensor / set_actor_root_state_tensor,
 *                                 isaacgym_wrapper.py:190-194)
 *   m3_command                  MPPI.command mppi.py:211-264 (whole call)
 *   m3_rollout                  _compute_total_cost_batch_halton/_simple + _compute_rollout_costs
 *                                 mppi.py:275-332, 335-363, 381-428 with dynamics/running_cost
 *                                 of reactive_tamp.py:63-73 and Objective.compute_cost
 *                                 cost_functions.py:19-169 fused in
 *   m3_update                   _exp_util mppi.py:430-456, _multi_modal_exp_util +
 *                                 update_infinite_beta m3p2i.py:24-64, weighted sums
 *                                 mppi.py:493-498, m3p2i.py:75-83
 *   m3_finalize                 mean update mppi.py:502-503 / m3p2i.py:86-87, top-k +
 *                                 Savitzky-Golay mppi.py:245-264, simple-mode U update :231
 *   m3_sim_*                    IsaacGymWrapper step-mode surface: set_dof_velocity_target_tensor
 *                                 :196, step :354-360, apply_rigid_body_force_tensors :202,
 *                                 refresh of _dof_state/_root_state/_rigid_body_state/
 *                                 _net_contact_force :98-118
 *   m3_cost                     Objective.compute_cost (step mode) cost_functions.py:19-36
 *   m3_sim_suction_forces /     calculate_suction, check_and_apply_suction utils/skill_utils.py:36-94
 *   m3_sim_check_and_apply_suction   (the real-world side of scripts/sim.py:41-49)
 *   m3_get_buffer               attribute access MPPI.states/actions/weights/top_trajs/...
 *   m3_get_info                 M3P2I.get_pull_preference m3p2i.py:16-22 (+ diagnostics)
 *
 * Conventions: plain C, no exceptions cross the boundary.  Every call returns 0 on success
 * or a negative m3_status; m3_last_error() gives the message.  All device work is enqueued
 * on the handle's HIP stream (m3_set_stream); calls are asynchronous unless stated.  A
 * handle is not thread-safe; different handles are independent.  The library owns all
 * device buffers; m3_get_buffer hands out non-owning device pointers valid until
 * m3_destroy.
 */
#ifndef M3P2I_HIP_H
#define M3P2I_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define M3_MAX_NU 9
#define M3_TOPK 20
#define M3_ABI_VERSION 4

typedef enum {
    M3_OK = 0,
    M3_ERR_BAD_ARG = -1,
    M3_ERR_HIP = -2,
    M3_ERR_SHAPE = -3,
    M3_ERR_STATE = -4,
    M3_ERR_UNSUPPORTED = -5
} m3_status;

typedef enum { M3_ENV_POINT = 0, M3_ENV_PANDA = 1 } m3_env;

/* cost_functions.py:19-36 task strings */
typedef enum {
    M3_TASK_NAVIGATION = 0,
    M3_TASK_PUSH = 1,
    M3_TASK_PULL = 2,
    M3_TASK_PUSH_PULL = 3,
    M3_TASK_REACH = 4,
    M3_TASK_PICK = 5,
    M3_TASK_PLACE = 6,
    M3_TASK_IDLE = 7
} m3_task;

typedef struct {
    int abi_version;        /* M3_ABI_VERSION */
    int device;             /* HIP device ordinal */
    /* sampling / sharding: rank owns global samples [k_offset, k_offset + K_local) */
    int K_global;
    int K_local;
    int k_offset;
    int T;                  /* horizon */
    int nu;                 /* 2 (point_env) or 9 (panda_env) */
    int env_type;           /* m3_env */
    int multi_modal;        /* cfg.multi_modal */
    int mode_simple;        /* mppi_mode == 'simple' */
    int sampling_random;    /* sampling_method == 'random' (in-kernel xoshiro128++) */
    int sample_null_action;
    int filter_u;
    int u_per_command;
    float u_min[M3_MAX_NU];
    float u_max[M3_MAX_NU];
    float noise_sigma_diag[M3_MAX_NU]; /* diagonal of cfg.mppi.noise_sigma */
    float u_scale;          /* mppi.py:297.  M3_BUF_ACTIONS holds the SCALED controls u_scale * a (what the dynamics
                               got and what the reference's distribution update consumes, mppi.py:313-331); the
                               division of mppi.py:353 / :420 only concerns the attribute a caller reads */
    float gamma;            /* rollout_var_discount */
    float lambda_;
    float step_size_mean;   /* 0.98, mppi.py:178 */
    float kp_suction;       /* config_point.yaml:9 */
    float pre_height_diff;  /* config_panda.yaml:9 */
    float dt;               /* isaacgym/{point,panda}.yaml:4 */
    int substeps;           /* isaacgym_wrapper.py:10 */
    int solver_iters;       /* isaacgym_wrapper.py:28 */
    int cube_on_shelf;      /* reactive_tamp.py:29 */
    int sim_only;           /* 1: handle is used only through m3_sim_* / m3_cost (the wrapper's
                               environments); planner-shape checks (K >= 20, filter rows) are
                               skipped and m3_rollout/m3_update are refused */
    int shard_mix;          /* sharded handles (K_local < K_global): 1 = ONE collective per command, an
                               all-gather of per-rank records (M3_BUF_RECORD -> M3_BUF_RECORDS_ALL) between
                               m3_update and m3_finalize.
                               * single-mode MPPI (beta fixed during a command, mppi.py:430-456): m3_update
                                 runs the softmin on the rank's own shard (local minimum m_r, local eta_r,
                                 normalised local sums) into the record; m3_finalize mixes the ranks' records
                                 with rho_r = exp(-(m_r - m)/beta) eta_r / sum_r(...) -- exact in real
                                 arithmetic, equal to the gather + reduce protocol up to f32 rounding.
                               * multi-modal M3P2I (on-the-fly beta search over ALL samples, m3p2i.py:24-64):
                                 the record is {the shard's trajectory costs | its top-k}; after the gather
                                 every rank holds all K_global costs and runs the unsharded update on them,
                                 RE-GENERATING the other ranks' actions from the replicated noise table and
                                 plan (a function of the global sample index, mppi.py:381-416) instead of
                                 receiving them: bit-identical to the unsharded handle.  Needs the noise rows
                                 of all K_global samples on every rank (m3_set_noise_global /
                                 m3_set_noise_knots_global; 15 MB at K = 64000).
                               2 = (multi-modal only) the same with each shard's minima and its eta(beta) sums on
                                 the beta ladders added to the record: after the gather the searches walk the
                                 MIXTURE of the shards' tables (eta(beta_j) = sum_r exp(-(m_r - m)/beta_j) eta_r(beta_j))
                                 instead of re-evaluating all K costs -- passes over the gathered costs only when
                                 a search leaves its ladder -- and one kernel forms weights, sums, best rows and the
                                 plan: per-rank work after the collective halves.  Equal to the unsharded run up to
                                 f32 rounding (plan <= 3e-5, same beta-search iteration counts), bit-identical
                                 across ranks.
                               3 = (multi-modal only) TWO small exchanges with O(K_local) work per rank in between
                                 (m3_update_b below): the record of 2, then every rank's weighted sums of its OWN
                                 samples; pays from K_global ~ 300 k (8 x 131072: 0.402 vs 0.441 ms per command).
                               0 = gather + reduce, two collectives (all-gather TRAJ_COST, all-reduce REDUCE) */
    /* ---- the MPPIConfig switches no shipped config turns on (mppi.py:39-54); zero = the defaults ---- */
    int noise_abs_cost;     /* mppi.py:366-367: |noise| in the action cost (read in simple mode only, as in the reference) */
    int update_cov;         /* mppi.py:201, :508-516: after every command of a single-mode halton-spline planner
                               cov_action <- 0.3 cov_action + 0.7 mean_t sum_k w_k (a_k - mean)^2 + 0.005 and
                               scale_tril = sqrt(cov_action) (M3_BUF_COV: the rollout reads its scale from there).
                               Ignored for multi_modal / simple mode, exactly as the reference ignores it there
                               (m3p2i.py:66-92 and mppi.py:220-233 have no such branch); unsharded handles only */
    int full_sigma;         /* 0: noise_sigma = diag(noise_sigma_diag).  1: noise_sigma_full is the matrix; its
                               diagonal must equal noise_sigma_diag.  Only the paths where the reference uses the whole
                               matrix read it: MultivariateNormal sampling (sampling_random / simple mode,
                               mppi.py:129-131, :340, :481) through its Cholesky factor and the action cost
                               (mppi.py:128, :366-372) through its inverse, both formed in binary64 and rounded to f32;
                               the Halton noise is scaled by sqrt(diag) alone (mppi.py:175-176, :394) */
    float noise_mu[M3_MAX_NU];                         /* mppi.py:127-131: mean of the sampled noise */
    float noise_sigma_full[M3_MAX_NU * M3_MAX_NU];     /* row-major [nu][nu] */
    unsigned long long seed;
} m3_config;

/* Planar world state of ONE environment, as the caller sees it through the wrapper's
 * tensors (dof_state = [x, vx, y, vy]; boxes = x, y, yaw quaternion (z, w), vx, vy, wz). */
typedef struct {
    float robot[4];      /* x, y, vx, vy */
    float box[7];        /* x, y, qz, qw, vx, vy, wz */
    float dyn_obs[7];
} m3_point_world;

typedef struct {
    float eta, eta_1, eta_2;
    float beta, beta_1, beta_2;  /* beta AFTER the call (panda single-mode persists it) */
    int iters, iters_1, iters_2; /* beta-search passes */
    int best_idx, best_idx_1, best_idx_2; /* GLOBAL sample indices */
    float wsum_push, wsum_pull;  /* sum of weights of the two halves (m3p2i.py:18-19) */
    int pull_preference;
    int calls;
} m3_info;

typedef struct {
    float rollout_ms, update_ms, finalize_ms, total_ms; /* HIP-event times of the last
                                                           m3_command with timing enabled */
} m3_timing;

/* buffers for m3_get_buffer; shapes in comments (Kl = K_local, Kg = K_global).
 * Layouts are TIME-MAJOR so that consecutive lanes (samples) touch consecutive addresses. */
typedef enum {
    M3_BUF_STATES = 0,      /* f32 [T][Kl][4]   (x, vx, y, vy)  mppi.py:318 (transposed) */
    M3_BUF_ACTIONS = 1,     /* f32 [T][Kl][nu]                 mppi.py:317 (transposed) */
    M3_BUF_COST_HORIZON = 2,/* f32 [T][Kl]                     mppi.py:310 (transposed) */
    M3_BUF_TRAJ_COST = 3,   /* f32 [Kl]  discounted J (halton) / S + perturbation (simple) */
    M3_BUF_TRAJ_COST_ALL = 4,/* f32 [Kg] gathered J used by m3_update */
    M3_BUF_WEIGHTS = 5,     /* f32 [Kg] */
    M3_BUF_WEIGHTS_1 = 6,   /* f32 [Kg/2] */
    M3_BUF_WEIGHTS_2 = 7,   /* f32 [Kg - Kg/2] */
    M3_BUF_MEAN = 8,        /* f32 [T][nu] mean_action (U in simple mode) */
    M3_BUF_MEAN_1 = 9,
    M3_BUF_MEAN_2 = 10,
    M3_BUF_BEST = 11,       /* f32 [T][nu] best_traj */
    M3_BUF_BEST_1 = 12,
    M3_BUF_BEST_2 = 13,
    M3_BUF_ACTION_OUT = 14, /* f32 [T][nu] returned plan (filtered) */
    M3_BUF_TOP_IDX = 15,    /* i32 [M3_TOPK] global indices */
    M3_BUF_TOP_TRAJS = 16,  /* f32 [M3_TOPK][T][2] */
    M3_BUF_REDUCE = 17,     /* f32 [reduce_len] packed partial sums: all-reduce(sum) this
                               buffer between m3_update and m3_finalize when sharded */
    M3_BUF_NOISE = 18,      /* f32 [T][Kl][nu] delta (time-major copy of m3_set_noise) */
    M3_BUF_PENDING_FORCE = 19, /* f32 [4][Kl] suction force pending for the next step */
    M3_BUF_INFO = 20,       /* device copy of m3_info */
    M3_BUF_SIM_WORLD = 21,  /* f32 [28][Kl] step-mode environments (SoA; rows 18..21 = pending
                               force in M3_BUF_PENDING_FORCE order); allocated on first use */
    M3_BUF_RECORD = 22,     /* f32 [record_len] this rank's record (shard_mix).  Single-mode: header {m_r,
                               eta_r, half sums, best idx, top-k costs and indices} + a REDUCE-shaped
                               body (normalised local sums, best rows, top trajectories).  Multi-modal:
                               [Kl] trajectory costs (M3_BUF_TRAJ_COST aliases them) | top-k costs |
                               top-k global indices | top-k trajectories [M3_TOPK][T][2] */
    M3_BUF_RECORDS_ALL = 23,/* f32 [K_global/K_local][record_len]: all-gather M3_BUF_RECORD into
                               this buffer between m3_update and m3_finalize (shard_mix) */
    M3_BUF_NOISE_ALL = 24,  /* f32 [K_global/K_local][T][Kl][nu]: every shard's noise block (one-collective
                               multi-modal shards only; M3_BUF_NOISE is this rank's block of it) */
    M3_BUF_COV = 25,        /* f32 [2][nu]: cov_action | scale_tril (mppi.py:175-176; rewritten by every command
                               when update_cov is on) */
    M3_BUF_RECORD_B = 26,   /* f32 [recb_len] shard_mix = 3: this rank's SECOND record -- {-w, index} of its best sample per
                             * weight set, its half sums, its weighted action sums [3][T][nu] and best rows [3][T][nu] */
    M3_BUF_RECORDS_B_ALL = 27, /* f32 [K_global/K_local][recb_len]: all-gather M3_BUF_RECORD_B into it before m3_finalize */
    M3_BUF_COUNT = 28
} m3_buffer_id;

typedef struct m3_handle m3_handle;

int m3_abi_version(void);
const char* m3_last_error(const m3_handle* h); /* h may be NULL: error of the last failed
                                                  m3_create on this thread */
/* sha256 prefix (16 hex digits) of the kernel sources + compiler flags this library was built from (m3p2i_aip_amd/build.py:
 * source_hash); identical for a rebuild of the same tree: the key of the committed PMC profiles (profiles/, bench.py). */
const char* m3_build_id(void);
void m3_default_config(m3_config* cfg, int env_type);
int m3_create(const m3_config* cfg, m3_handle** out);
void m3_destroy(m3_handle* h);
int m3_set_stream(m3_handle* h, void* hip_stream);
int m3_enable_timing(m3_handle* h, int on);
/* launch geometry of the rollout kernel: samples (active lanes) per 64-wide wavefront,
 * a power of two in 1..64, or 0 = choose from K_local so that the waves fill the chip
 * (DESIGN.md "Lanes per wavefront").  Results do not depend on it. */
int m3_set_rollout_lanes(m3_handle* h, int lanes);
/* point_env: wavefronts per 64 samples in the rollout kernel of the navigation and push tasks (default sampler, default cost
 * weights, at most as many wavefronts as the chip has SIMDs, T <= 31) -- 0 = one wavefront does everything, 1 = two: one runs
 * the dynamics alone, its companion assembles the actions ahead of it and forms costs, stores and sums behind it (hand-over
 * through LDS), wherever that form exists; -1 (default) = automatic: 1 where it exists and was measured not slower.  Every
 * other rollout (pull, push_pull, the other samplers, weighted costs, m3_batch_command, episodes) keeps one wavefront whatever
 * the value.  Results do not depend on it.  A hand-over wait that runs out (bounded) invalidates that rollout's results and
 * makes the handle's NEXT m3_rollout / m3_command fail with M3_ERR_HIP.  DESIGN.md section 6. */
int m3_set_point_rollout_form(m3_handle* h, int form);
/* the form of the last rollout launch of m3_rollout / m3_command (0, 1); -1 before the first */
int m3_point_rollout_form_used(m3_handle* h);
/* panda_env: lanes that simulate ONE sample in the rollout kernel -- 1 (a lane per sample, 64 samples per wavefront), 8 or
 * 16 (the lanes of a DPP row share a sample: the contact solver's joint-space rows run across them; eight / four sample
 * slots per wavefront), 0 = automatic: by size (16 while the launch has no more wavefronts than the chip has SIMDs, then 8,
 * then 1); for the reach task (quirk Q8) 16 with the reach cost kernel (below) wherever that is available and one round of
 * sixteen-lane wavefronts fits (K <= 4096), else by what the last commands' rollouts met -- 1 (with shadow sample slots) while
 * few of them had the gripper within reach of a box or an awake cube, 8 once many did.  Same results, bit for bit
 * (world spec v3 defines the rows' sums as the pairwise tree all forms evaluate).  DESIGN.md section 6. */
int m3_set_panda_lanes_per_sample(m3_handle* h, int lanes_per_sample);
/* panda_env, reach task on an unsharded handle (quirk Q8: every rollout's cost is measured against environment 0's cube):
 * 1 (default) = with K <= 8192 and the default sampler the rollout kernel runs WITHOUT shadow sample slots in a many-lane form
 * and leaves what the cost reads per (step, sample) behind; a second kernel forms the costs (same values, same operations, same
 * bits).  0 = the shadow slots (every wavefront re-simulates samples 0 and K / 2), as for larger K, the random sampler and
 * mppi_mode 'simple'. */
int m3_set_panda_reach_cost_kernel(m3_handle* h, int on);
/* the form the last panda rollout ran in (1, 8, 16; 0 before the first) */
int m3_panda_lanes_per_sample_used(m3_handle* h);
/* what the automatic choice for reach reads: the share, in 1/1000, of the last FINISHED panda rollout launch's (sample,
 * substep) pairs in which the gripper was within reach of a box or a cube was awake (the kernel's last wavefront reports
 * it into mapped host memory; no synchronisation); -1 before the first report */
int m3_panda_near_share(m3_handle* h);
/* EXTENSION, panda_env only: the pick-and-place WORKSPACE as per-handle state -- what a user of the reference edits in the
 * yaml files of config/panda_env (panda, 1_table, 3_shelf_stand, 4_obs, 5_cubeA, 6_cubeB) and the actors' friction.  The
 * defaults are the reference's workspace.
 * NOT part of the scene, and why: the cube's SIZE -- the checker the kernels are held to bit for bit carries the cube's
 * bounding radius as the literal 0.0434 next to its run-time half extent, so another size cannot be verified; the grasp and
 * gripper geometry, the joint limits, inertias and efforts -- they are the Franka URDF's, and other robots are out of scope
 * (DESIGN.md section 9); g, the drive, the solver constants, dt, substeps and iterations -- they are the spec, not the room. */
typedef struct m3_panda_scene {
    float base[3];      /* robot mount (panda.yaml)                     default -0.45, 0, 1.125 */
    float table[6];     /* centre xyz, half extents xyz (1_table.yaml)  default 0,0,1.0, 0.6,0.6,0.025 */
    float shelf[6];     /* shelf_stand likewise                          default 0.5,0,1.175, 0.1,0.1,0.15 */
    float obs_half[3];  /* the dyn-obs plate's half extents              default 0.1,0.1,0.01 */
    float obs_m;        /* its mass                                      default 0.8 */
    float cube_m;       /* mass of cubeA and cubeB                       default 0.125 */
    float mu;           /* contact friction                              default 1.0 */
} m3_panda_scene;
void m3_default_panda_scene(m3_panda_scene* sc);
/* Applies from the next command / rollout / step / cost call; survives m3_reset.  It writes into fixed members of the handle:
 * no allocation, no synchronisation.  sc == NULL: back to the defaults.  Allowed on planner, sharded and sim_only handles; a
 * world handle and its planners may carry different scenes (each handle uses its own).  Sharded handles: set the same scene on
 * every rank.  Every field is checked before any state changes: a NaN or infinite field, a half extent <= 0, a mass <= 0 or
 * mu < 0 is M3_ERR_BAD_ARG and the message names the field ("m3_set_panda_scene: table[5] must be > 0"); a point_env handle
 * is M3_ERR_UNSUPPORTED.  A refused call leaves the handle unchanged.
 * Which kernels run.  A handle whose 21 floats equal the defaults bit for bit runs exactly the kernels it ran before this call
 * existed.  So does a handle that differs in cube_m / obs_m alone, on every path (m3_batch_command and m3_panda_episodes_*
 * included): the masses reach the kernels through values that were kernel arguments already.  Any other handle (base, table,
 * shelf, obs_half, mu) runs the run-time-scene instances of the rollout (all tasks, both samplers, both mppi modes; 1, 8 or 16
 * lanes per sample chosen as before; the reach-cost kernel as before), of the step, of m3_cost and of the views' refresh -- at
 * the default values the same bits.
 * Batched on request: a batch created with m3_batch_create_ex(..., M3_BATCH_PANDA_RUNTIME, ...) takes a handle that needs the
 * run-time-scene instance (bit-identical to its own m3_command, like every batched handle).  A batch made by m3_batch_create
 * -- whose table slots have no room for the larger entry -- returns M3_ERR_UNSUPPORTED for it, and so do
 * m3_panda_episodes_create / _act / _act_first with such a world or planner, whatever batch they are handed (the message
 * names m3_set_panda_scene and the index of the handle); nothing is launched.  A set created by m3_panda_episodes_create_ex
 * with M3_PANDA_EPISODES_RUNTIME takes them (include/m3p2i_hip_ext.h). */
int m3_set_panda_scene(m3_handle* h, const m3_panda_scene* sc);
int m3_get_panda_scene(const m3_handle* h, m3_panda_scene* out);
/* Test and A/B switch: -1 the automatic choice above (default), 1 the run-time-scene instances whatever the values, 0 never --
 * with a geometry or friction other than the default the next command / rollout / step / cost call is then refused
 * (M3_ERR_STATE: "... forced off ..."). */
int m3_set_panda_scene_instance(m3_handle* h, int on);
/* 0 / 1: whether the last rollout or step of the handle launched the run-time-scene instance */
int m3_panda_scene_instance_used(m3_handle* h);
/* One workspace PER ENVIRONMENT of a sim_only panda_env handle (extension): scenes[e] is the workspace of
 * environment e, n must equal K_local.  From the next m3_sim_step*, m3_sim_pull_state / _push_state and m3_cost on, lane e runs
 * in scenes[e] (the link poses of the views through scenes[e].base); the step is panda_step in that workspace, bit for bit the
 * single-scene handle's where the rows agree.  A point_env handle is M3_ERR_UNSUPPORTED ("... panda_env only"), a planner
 * handle M3_ERR_STATE (its samples take their workspaces from m3_set_panda_rollout_scenes below), n != K_local M3_ERR_SHAPE.
 * Every row is checked as m3_set_panda_scene checks its scene, before any state changes: a bad field is M3_ERR_BAD_ARG,
 * "m3_set_panda_scene_rows: row 3: table[5] must be > 0".  scenes == NULL switches the rows off (n is not read): the handle is
 * back on its single workspace and runs exactly the kernels of a handle that never had rows.  Against m3_set_panda_scene the
 * last call wins.  The rows survive m3_reset.  The first call on a handle allocates the table (22 words per row; host, pinned
 * and device copies), later calls reuse it; m3_sim_step*, m3_cost and the views' refresh never allocate because of it.
 * The rows need the run-time scene: with m3_set_panda_scene_instance(h, 0) the next step / cost / view call is M3_ERR_STATE
 * ("... forced off ... m3_set_panda_scene_rows"); m3_panda_scene_instance_used reports 1 while rows are on.  m3_cost takes the
 * handle's cost weights as before (m3_panda_weighted_cost_instance_used keeps saying whether the WEIGHTS needed them).
 * In the lockstep episodes on request: m3_panda_episodes_create / _observe / _act / _act_first with such a world return
 * M3_ERR_UNSUPPORTED (the message names m3_set_panda_scene_rows), nothing is launched; a set created by
 * m3_panda_episodes_create_ex with M3_PANDA_EPISODES_RUNTIME steps row e of the world in scenes[e]. */
int m3_set_panda_scene_rows(m3_handle* h, const m3_panda_scene* scenes, int n);
/* row `row` as it was set; M3_ERR_STATE while the rows are off */
int m3_get_panda_scene_row(const m3_handle* h, int row, m3_panda_scene* out);
/* 0 / 1: whether the handle is on per-environment workspaces */
int m3_panda_scene_rows_set(const m3_handle* h);
/* One workspace PER SAMPLE of a panda_env planner handle's fused rollout (extension) -- a planner that
 * plans over a spread of models: sample i of m3_rollout / m3_command is simulated in scenes[i], all tasks, both samplers, both
 * mppi modes, 1, 8 or 16 lanes per sample chosen as before.  n must equal K_local; a sharded handle passes the K_local rows of
 * its own samples (k_offset .. k_offset + K_local - 1 of the global list).  Checks, NULL, last-call-wins against
 * m3_set_panda_scene, m3_reset and the allocation: as m3_set_panda_scene_rows; a sim_only handle is M3_ERR_STATE.
 * Quirk Q8: the reach cost of every sample reads the cube of sample 0 AS SIMULATED IN scenes[0] (multi-modal: the orientation
 * of sample K / 2 in scenes[K / 2]) -- what the reference would see with per-environment actor properties.
 * The handle's own step, cost and views (m3_sim_*, m3_cost) keep its single workspace.  The rollout always runs the weighted
 * cost's kernels, which give the literal cost's bits at the default weights; rows that all equal one scene give the bits of
 * m3_set_panda_scene with that scene.  m3_panda_scene_instance_used reports 1; m3_set_panda_scene_instance(h, 0) makes the next
 * command / rollout M3_ERR_STATE ("... forced off ... m3_set_panda_rollout_scenes").
 * Batched on request: a batch created with m3_batch_create_ex(..., M3_BATCH_PANDA_RUNTIME, ...) takes such a handle (each
 * sample reads its row of the handle's own table; bit-identical to the handle's own m3_command).  A batch made by
 * m3_batch_create returns M3_ERR_UNSUPPORTED for it, and so do m3_panda_episodes_create / _observe / _act / _act_first with
 * such a planner, whatever batch they are handed (the message names m3_set_panda_rollout_scenes and the index of the handle);
 * nothing is launched.  A set created by m3_panda_episodes_create_ex with M3_PANDA_EPISODES_RUNTIME takes it. */
int m3_set_panda_rollout_scenes(m3_handle* h, const m3_panda_scene* scenes, int n);
int m3_get_panda_rollout_scene(const m3_handle* h, int row, m3_panda_scene* out);
/* 0 / 1: whether the handle's rollout is on per-sample workspaces */
int m3_panda_rollout_scenes_set(const m3_handle* h);
/* launch structure of the unsharded multi-modal update with K beyond the one-launch kernel's range: 0 (default) = three
 * launches (ladder + search in one grid, weights + sums, combine), 5 = the five launches of round 3 (minima, ladder,
 * search, weights, sums), whose sums are added in the order of the sharded "exact" protocols (tests compare those bit
 * for bit).  Pass counts, best samples and the plan (to rounding) do not depend on it. */
int m3_set_update_launches(m3_handle* h, int launches);

/* assignment of samples to wavefronts in the point_env rollout: 1 (default) = sorted by the
 * direction of each sample's noise path (computed on the device whenever the noise is set, so that
 * a wavefront's samples meet the same obstacles), 0 = by index.  Results do not depend on it. */
int m3_set_wave_order(m3_handle* h, int on);
/* bound of the waits inside the multi-modal update's launches (k_update_small's column workgroups wait for each other's
 * beta-ladder points, k_ladder_search's search workgroup for the ladder workgroups' flags; a wait that runs out -- other
 * kernels occupying the CUs -- makes the waiting workgroup run the reference's iterative passes itself: same pass counts,
 * same weights): -1 = default (2^18 polls, ~20 ms), 0 = never wait (every workgroup takes the give-up branch: the tests
 * of that branch), n > 0 = n polls. */
int m3_set_ladder_spins(m3_handle* h, int spins);
/* Relabels the samples instead: the noise rows are permuted ONCE (by the next m3_rollout, which knows
 * the world) into that order, within each mode's half and with the rows of the special samples (0,
 * K/2, K-1) left in place, so that afterwards sample k simply has another row of the SAME noise set
 * and index order is wavefront order (coalesced stores, no per-command scatter).  For a caller whose
 * row labels carry no meaning -- the reference's own Halton sampler: planner._ensure_noise calls it.
 * The sample SET, and with it the plan, is unchanged up to the order of f32 summation; per-sample
 * outputs (weights[k], states[k], top_idx) refer to the new labels. */
int m3_relabel_samples(m3_handle* h);

/* delta: [K_local][T][nu] row-major (the reference's layout, rows of THIS shard).
 * on_device: 0 host pointer, 1 device pointer. */
int m3_set_noise(m3_handle* h, const float* delta, int on_device);
/* The reference's Halton-spline sampler on the device (mppi.py:458-483, mppi_utils.py bspline):
 * knots [K_local][nu][n_knots] (the Gaussian Halton values of THIS shard's samples); every one of
 * the K_local*nu series is fitted with FITPACK's smoothing spline (splrep(linspace(0,n,n), y,
 * k=degree, s=smoothing)) and evaluated at linspace(0, n, T) with ext=3 (splev), one thread per
 * series, into M3_BUF_NOISE.  Bit-identical to scipy 1.15.3's FITPACK (tests/test_spline_fit.py). */
int m3_set_noise_knots(m3_handle* h, const float* knots, int n_knots, int degree, float smoothing,
                       int on_device);
/* the same two for a one-collective multi-modal shard (cfg.shard_mix with multi_modal): rows / knots of
 * ALL K_global samples, [K_global][T][nu] / [K_global][nu][n_knots] -- every rank holds the whole table */
int m3_set_noise_global(m3_handle* h, const float* delta_all, int on_device);
int m3_set_noise_knots_global(m3_handle* h, const float* knots_all, int n_knots, int degree, float smoothing,
                              int on_device);
/* The WHOLE reference sampler on the device: Halton radical inverses (in-tree use_ghalton=False branch,
 * mppi_utils.py:69-96) -> sqrt(2) erfinv(2u - 1) (:99-104) -> the smoothing spline of m3_set_noise_knots, for
 * this shard's samples (all K_global for a one-collective multi-modal shard).  The uniform Halton values are
 * bit-identical to the host sampler's; the Gaussian ones are not promised bit for bit (the device's logf / sqrtf
 * differ from the host's libm in the last ulp): measured against a binary64 evaluation of the same float32
 * argument 2u - 1 they are off by at most 8.9e-8 for |g| < 1, 3.6e-7 for |g| < 4 and 4.6e-7 (one ulp) beyond, over
 * all 64000 samples, 32 and 99 columns, plain and Faure -- within 1.02 x the host sampler's own float32 error in
 * every range (erfinv's two Newton steps run in binary64).  The planner's default stays m3_set_noise_knots with host
 * knots, pinned bit for bit by golden G8; this entry (MPPIConfig.device_knots) removes the last host values. */
int m3_set_noise_halton(m3_handle* h, int n_knots, int degree, float smoothing);
/* The same with a GENERALIZED (digit-permuted) Halton sequence -- the structure of the branch the reference's
 * planner actually executes: mppi.py:465-471 calls generate_gaussian_halton_samples(..., use_ghalton=True) ->
 * ghalton.GeneralizedHalton(EA_PERMS[:ndims]) (mppi_utils.py:89-95).  `ghalton` is a third-party package that is
 * absent here and unpinned in the reference (pyproject.toml:15), so its EA_PERMS table cannot be restated; what can
 * be is the construction with a published, formula-defined permutation set:
 *   M3_HALTON_FAURE   H. Faure, "Good permutations for extreme discrepancy", J. Number Theory 42 (1992) 47-56.
 * The plain sequence's high dimensions are strongly correlated (the panda_env knots are 45-dimensional: primes up to
 * 197, |corr| up to 0.45 between neighbouring dimensions at K = 4000; 0.08 with Faure's permutations).
 * M3_HALTON_PLAIN == m3_set_noise_halton (the default: pinned by golden G8). */
#define M3_HALTON_PLAIN 0
#define M3_HALTON_FAURE 1
int m3_set_noise_halton_scrambled(m3_handle* h, int n_knots, int degree, float smoothing, int scramble);
/* sampling_random / simple mode: the draws of N(noise_mu, noise_sigma) that the NEXT m3_rollout generates in
 * registers (MultivariateNormal(...).sample((K, T)), mppi.py:340 / :481), written to M3_BUF_NOISE for a caller
 * that runs the rollout itself (the planner's STEP mode: user dynamics / running_cost callables) */
int m3_sample_noise(m3_handle* h);
int m3_set_objective(m3_handle* h, int task, const float* goal, int goal_len, int gripper_cmd);
/* EXTENSION, off by default (= the reference): push / pull / push_pull add get_motion_cost -- 1000 while the dyn-obs
 * feels a contact force > 0.1 (cost_functions.py:158-169) -- the way navigation does.  The shipped compute_cost
 * returns before that term for these tasks (cost_functions.py:23-29 vs :36), so the reference's push / pull rollouts are
 * blind to the dyn-obs; its logged experiments `plot/point/case2_halton_{push,pull}_coll.npy` show 3 / 60 and 1 / 60
 * collisions, i.e. were made with the term active.  point_env only.  The rollout then runs its general instance. */
int m3_set_avoid_dyn_obs(m3_handle* h, int on);
/* EXTENSION, point_env only: the literal WEIGHTS of the four point tasks' costs as per-handle state (the defaults = the
 * reference's literals, cost_functions.py:38-89,158-169).  Thresholds and values that are not weights stay literals: the 0.1
 * contact-force threshold, the 0.5 radius and the 0.6 value of the pull's velocity term, the suction constants. */
typedef struct m3_point_cost_weights {
    float nav_dist;      /* 1    :39       navigation: |robot - goal| */
    float collision;     /* 1000 :158-169  the penalty of get_motion_cost (navigation; push / pull with avoid_dyn_obs) */
    float robot_box;     /* 1    :49       calculate_dist: |robot - box| */
    float box_goal;      /* 10   :49       calculate_dist: |box - goal| */
    float push_dist;     /* 3    :60 */
    float push_align;    /* 1    :60 */
    float pull_dist;     /* 3    :89 */
    float pull_vel;      /* 3    :89 */
    float pull_align;    /* 7    :89 */
} m3_point_cost_weights;
void m3_default_point_cost_weights(m3_point_cost_weights* w);
/* Applies from the next command / rollout / cost call (fused rollout, batched command, episodes, step-mode m3_cost alike);
 * survives m3_reset; no allocation, no synchronisation.  w == NULL: back to the defaults.  Negative and zero weights are
 * legal; a NaN or infinite one is M3_ERR_BAD_ARG (the message names the field); a panda_env handle M3_ERR_UNSUPPORTED.
 * A handle whose nine floats equal the defaults bit for bit runs exactly the kernels it ran before this call existed; any
 * other handle runs the weighted build of the general rollout instance (and of the step-mode cost), in which each literal
 * is replaced by its weight one for one -- at the default weights the same bits.  Sharded handles: set the same weights
 * on every rank. */
int m3_set_point_cost_weights(m3_handle* h, const m3_point_cost_weights* w);
int m3_get_point_cost_weights(const m3_handle* h, m3_point_cost_weights* out);
/* Test and A/B switch: -1 the automatic choice above (default), 1 the weighted build whatever the weights, 0 never -- with
 * weights other than the defaults the next command / rollout / cost call is then refused (M3_ERR_STATE). */
int m3_set_weighted_cost_instance(m3_handle* h, int on);
/* EXTENSION, panda_env only: the literal WEIGHTS of the three panda tasks' costs as per-handle state (the defaults = the
 * reference's literals, cost_functions.py:91-170) -- what a user of the reference tunes pick-and-place with.
 * What stays a literal, and why: the 0.1 contact-force threshold of the collision test (a threshold, not a weight; shelf_force
 * scales what is compared with it); the `1 -` of the place cost (an offset: place_grip scales the whole term); the finger-pad
 * offset (geometry of the gripper).  pre_height_diff and tilt_cos_theta are no weights either: they are config and objective
 * (m3_config, m3_set_objective). */
typedef struct m3_panda_cost_weights {
    float reach_dist;   /* 10    cost_functions.py:114      |ee - pre-pick goal| */
    float reach_tilt;   /* 3     :156  get_pick_tilt_cost   ee-to-cube orientation */
    float pick_goal;    /* 10    :125  |pre-place - cubeA| */
    float pick_ori;     /* 15    :125  cube-to-goal orientation */
    float collision;    /* 1000  :170  get_motion_cost's penalty (pick) */
    float shelf_force;  /* 4     :163  weight of the shelf stand's contact force inside the collision test */
    float place_grip;   /* 2     :134 */
} m3_panda_cost_weights;
void m3_default_panda_cost_weights(m3_panda_cost_weights* w);
/* Applies from the next command / rollout / cost call; survives m3_reset.  It writes into a fixed member of the handle: no
 * allocation, no synchronisation.  w == NULL: back to the defaults.  Negative and zero weights are legal; a NaN or infinite
 * field is M3_ERR_BAD_ARG, the message names the field ("m3_set_panda_cost_weights: pick_ori is not finite") and the handle is
 * left unchanged; a point_env handle is M3_ERR_UNSUPPORTED ("panda_env only").  Allowed on planner, sharded and sim_only
 * handles.  Sharded handles: set the same weights on every rank.
 * Which kernels run.  A handle whose seven floats equal the defaults bit for bit runs exactly the kernels it ran before this
 * call existed, on every path.  Any other handle runs the weighted family: the rollout on the run-time scene (all tasks, both
 * samplers, both mppi modes; 1, 8 or 16 lanes per sample and shadow slots versus record + reach-cost kernel chosen as before),
 * the weighted reach-cost kernel and the weighted step-mode cost of m3_cost, in which each literal is replaced by its weight one
 * for one -- at the default weights the same bits.  Step, pull and push read no cost and stay as they are.
 * m3_set_panda_scene_instance / m3_panda_scene_instance_used keep their meaning ("used": whether the handle's workspace needed
 * the run-time scene); scene instance 0 with a geometry other than the default refuses as before, whatever the weights.
 * Batched on request: a batch created with m3_batch_create_ex(..., M3_BATCH_PANDA_RUNTIME, ...) takes a planner that needs the
 * weighted family (bit-identical to its own m3_command).  A batch made by m3_batch_create returns M3_ERR_UNSUPPORTED for it,
 * and so do m3_panda_episodes_create / _observe / _act / _act_first with such a planner, whatever batch they are handed (the
 * message names m3_set_panda_cost_weights and the index of the handle); nothing is launched.  A sim_only world handle with
 * weights is accepted by the episodes: its step reads no weight.  A set created by m3_panda_episodes_create_ex with
 * M3_PANDA_EPISODES_RUNTIME takes such a planner. */
int m3_set_panda_cost_weights(m3_handle* h, const m3_panda_cost_weights* w);
int m3_get_panda_cost_weights(const m3_handle* h, m3_panda_cost_weights* out);
/* Test and A/B switch: -1 the automatic choice above (default), 1 the weighted family whatever the weights, 0 never -- with
 * weights other than the defaults the next command / rollout / m3_cost is then refused (M3_ERR_STATE: "... forced off ..."). */
int m3_set_panda_weighted_cost_instance(m3_handle* h, int on);
/* 0 / 1: whether the last rollout or m3_cost of the handle launched the weighted family */
int m3_panda_weighted_cost_instance_used(m3_handle* h);
/* EXTENSION, point_env only: the ARENA as per-handle state -- what a user of the reference edits in the yaml files of config/point_env
 * (5_obs, 1..4_wall, 7_box, 6_dyn_obs) and pointRobot.urdf.  The physical fields of the dynamics' scene, one for one; g, the
 * velocity drive, the solver constants and the spec switches are not part of it.  The defaults are the reference's arena. */
typedef struct m3_point_scene {
    float robot_r, robot_m;                                  /* the robot disc: radius, mass */
    float box_hx, box_hy, box_m, box_I, box_mu_g, box_req;   /* the pushable box: half extents, mass, inertia, ground friction,
                                                              * mean lever arm of its footprint */
    float dyn_hx, dyn_hy, dyn_m, dyn_I, dyn_mu_g, dyn_req;   /* the dynamic obstacle, likewise */
    float obs_x, obs_y, obs_hx, obs_hy;                      /* the fixed obstacle: centre, half extents */
    float wall;                                              /* inner face of the four walls, a square centred at the origin */
    float mu_rb, mu_rd, mu_ro, mu_rw, mu_bw, mu_dw, mu_bd, mu_bo, mu_do;   /* pair frictions: r robot, b box, d dyn-obs,
                                                                            * o obstacle, w walls */
} m3_point_scene;
void m3_default_point_scene(m3_point_scene* sc);
/* Applies from the next command / rollout / step / episode tick; survives m3_reset; no allocation, no synchronisation.
 * sc == NULL: back to the defaults.  Allowed on planner, sharded and sim_only handles; a world handle and its planners may
 * carry different scenes (each handle uses its own).  Sharded handles: set the same scene on every rank.  A NaN or infinite
 * field, a size / mass / inertia / *_req / robot_r <= 0, a negative friction or wall <= robot_r is M3_ERR_BAD_ARG (the message
 * names the field); a panda_env handle M3_ERR_UNSUPPORTED.  A handle whose fields equal the defaults bit for bit runs exactly
 * the kernels it ran before this call existed; any other handle runs the run-time-scene build of the general rollout instance
 * (which is also its weighted build), of the batched rollout, of the step and of the episode tick. */
int m3_set_point_scene(m3_handle* h, const m3_point_scene* sc);
int m3_get_point_scene(const m3_handle* h, m3_point_scene* out);
/* Test and A/B switch: -1 the automatic choice above (default), 1 the run-time-scene build whatever the values, 0 never --
 * with a scene other than the default the next command / rollout / step is then refused (M3_ERR_STATE). */
int m3_set_point_scene_instance(m3_handle* h, int on);
/* EXTENSION, sim_only point_env handles: one arena PER ENVIRONMENT -- environment i steps in scenes[i] (the N independent "real
 * worlds" of a wrapper with num_envs = N, the world handle of m3_episodes_*).  n must equal the handle's K_local.  Applies from
 * the next m3_sim_step, m3_sim_step_with_target or episode tick / half-tick; survives m3_reset; may be called between ticks of a
 * running m3_episodes set, and m3_episodes_create accepts a world with rows set.  scenes == NULL clears the rows (n is not
 * read): the handle is back on its single scene and runs exactly the kernels it ran before.  Every row gets the checks of
 * m3_set_point_scene; a failing one is M3_ERR_BAD_ARG and the message names the row and the field ("row 2: box_m is not
 * finite").  A panda_env handle is M3_ERR_UNSUPPORTED, a handle that is not sim_only M3_ERR_STATE (a planner's samples get
 * their arenas from m3_set_point_rollout_scenes below), n != K_local M3_ERR_SHAPE.  Every check runs before any state changes: after a refusal the
 * rows and the single scene are what they were.
 * With m3_set_point_scene: the LAST call wins -- m3_set_point_scene on a handle with rows set clears the rows; while rows are
 * set m3_get_point_scene keeps returning the single scene (which no step reads), and m3_set_point_scene_instance(h, 0) refuses
 * the next step as it does for a non-default single scene.
 * Memory: the first call on a handle allocates a device table, its pinned host mirror and a host copy of the rows; later calls
 * reuse them (and wait for the handle's stream before they rewrite the mirror).  The upload is one hipMemcpyAsync on the
 * handle's stream.  m3_sim_step* and m3_episodes_tick / _begin / _end allocate nothing because of the rows. */
int m3_set_point_scene_rows(m3_handle* h, const m3_point_scene* scenes, int n);
/* row `row` as it was set; M3_ERR_STATE while no rows are set, M3_ERR_BAD_ARG for a row outside 0 .. K_local - 1 */
int m3_get_point_scene_row(const m3_handle* h, int row, m3_point_scene* out);
int m3_point_scene_rows_set(const m3_handle* h);   /* 0 / 1 */
/* EXTENSION, point_env PLANNER handles (unsharded or sharded): one arena PER SAMPLE of the fused rollout -- sample i of the handle
 * rolls out in scenes[i], so a planner can spread its K rollouts over K models of a world it knows only roughly (the reference
 * gets this from a simulator with num_envs = K whose environments carry their own actor properties).  n must equal the
 * handle's K_local.  Sample i is row i of every per-sample buffer (M3_BUF_TRAJ_COST[i], states[:, i], the pending force); its
 * global index is k_offset + i.  The row follows the sample, not the wavefront slot: m3_set_wave_order, m3_relabel_samples
 * and m3_set_rollout_lanes do not change which arena a sample gets.  dt, substeps, solver iterations and the solver constants
 * stay the handle's.  Applies from the next m3_rollout / m3_command; survives m3_reset.  scenes == NULL clears the rows (n is
 * not read): the handle is back on its single scene and launches exactly the kernels it launched before.
 * Every row gets the checks of m3_set_point_scene; a failing one is M3_ERR_BAD_ARG and the message names the row and the field
 * ("row 3: box_m is not finite").  A panda_env handle is M3_ERR_UNSUPPORTED, a sim_only handle M3_ERR_STATE (its environments:
 * m3_set_point_scene_rows), n != K_local M3_ERR_SHAPE.  Every check runs before any state changes.
 * With m3_set_point_scene: the LAST call wins, as on sim_only handles; m3_set_point_scene_instance(h, 0) with rows set refuses
 * the next rollout (M3_ERR_STATE).
 * While rows are set m3_rollout / m3_command run the per-sample build of the general, weighted rollout instance (all tasks,
 * multi_modal, both mppi modes, both samplers, avoid_dyn_obs, update_cov; tuned cost weights keep working); the two-wavefront
 * form is never taken (m3_point_rollout_form_used = 0); m3_point_rollout_plan(..., scene = 2, ...) reports the launch.
 * The special samples are the caller's business: the zero-noise / null-action sample K - 1 and, in multi-modal mode, the two
 * best-trajectory samples 0 and K / 2 get their rows like any other sample -- give them the nominal arena to keep them nominal.
 * NOT batched by the calls of this header: m3_batch_command with such a handle and m3_episodes_create / m3_episodes_tick with
 * such a planner return M3_ERR_UNSUPPORTED (the message names this call and the index of the handle); nothing is launched.
 * Batched on request: by the batch and the episode set that m3p2i_hip_ext.h declares.
 * Memory: the first call on a handle allocates a device table, its pinned host mirror and a host copy of the rows; later calls
 * reuse them (and wait for the handle's stream before they rewrite the mirror).  The upload is one hipMemcpyAsync on the
 * handle's stream.  m3_rollout and m3_command allocate nothing because of the rows. */
int m3_set_point_rollout_scenes(m3_handle* h, const m3_point_scene* scenes, int n);
/* row `row` as it was set; M3_ERR_STATE while no rows are set, M3_ERR_BAD_ARG for a row outside 0 .. K_local - 1 */
int m3_get_point_rollout_scene(const m3_handle* h, int row, m3_point_scene* out);
int m3_point_rollout_scenes_set(const m3_handle* h);   /* 0 / 1 */
/* Diagnostic, host only (no device call, no handle): the kernel form a point_env rollout with these settings takes -- what
 * m3_rollout / m3_batch_command would launch for a handle configured so.  weighted / scene: what the handle's cost weights and
 * scene (or their switches) amount to; form_request: m3_set_point_rollout_form's value; want_minima: the command keeps the
 * workgroups' cost minima.  out: instance (-1 general, 0..3 the task's), ref (solver settings compiled in), form (1: two
 * wavefronts), weighted, scene, workgroups, rows of minima, lanes.  scene = 2: the handle has an arena per sample
 * (m3_set_point_rollout_scenes): instance -1, ref 0, form 0, weighted 1, out[4] = 2. */
int m3_point_rollout_plan(int task, int multi_modal, int mode_simple, int sampling_random, int avoid_dyn_obs, int K_local, int T,
                          int lanes, float dt, int substeps, int solver_iters, int weighted, int scene, int form_request,
                          int want_minima, int out[8]);
/* The same with `priors`: 1 for a handle with prior samples set (m3_set_prior_samples below; scene is then 1, or 2 with an arena
 * per sample -- scene = 0 is M3_ERR_BAD_ARG, as a handle with priors always runs the run-time-scene instance).  out[0 .. 7] as
 * above (instance -1, ref 0, form 0, weighted 1, scene 1 or 2), out[8] = priors. */
int m3_point_rollout_plan_ex(int task, int multi_modal, int mode_simple, int sampling_random, int avoid_dyn_obs, int K_local, int T,
                             int lanes, float dt, int substeps, int solver_iters, int weighted, int scene, int form_request,
                             int want_minima, int priors, int out[9]);
/* EXTENSION, point_env PLANNER handles, unsharded: PRIOR SAMPLES -- a few of the K samples of the fused rollout take a control
 * sequence of the caller verbatim instead of clamp(mean + noise): the proposals of ancillary controllers (a straight line to the
 * goal, "go behind the box and push", yesterday's plan, a learned policy), as in Biased-MPPI.  The softmin update is unchanged.
 * seqs: host, [n][T][nu] (sample-major, the reference's layout); sample_idx: host, [n] GLOBAL sample indices.
 * Sample sample_idx[j] of the next rollouts takes a[t] = clamp(seqs[j][t], u_min, u_max), in both mppi modes and with both
 * samplers.  seqs[j][t] is the control of step t of THIS command's horizon: the library shifts nothing between commands, and
 * the priors stay as set until replaced or cleared -- a caller that plans every tick sets them every tick.  Everything behind
 * the select is unchanged: the u_scale multiplication, what is stored in M3_BUF_ACTIONS, the simple mode's noise = e - m
 * perturbation cost, the update (weights, means, best rows, update_cov, top-k).  The choice of index has a meaning only in
 * multi-modal mode, where k < K/2 belongs to mode 1 and k >= K/2 to mode 2: a prior informs the mode whose half it sits in.
 * The prior follows the sample, not the wavefront slot -- as the arena row and the cost weights do: m3_set_wave_order,
 * m3_relabel_samples and m3_set_rollout_lanes do not change which sample is a prior.  seqs == NULL or n == 0 clears the priors:
 * the handle then launches exactly the kernels it launched before the call existed.  Survives m3_reset.
 * Refused, every check before any state changes, the message names the entry: M3_ERR_BAD_ARG for n < 0 or n >
 * M3_MAX_PRIOR_SAMPLES, a null sample_idx, an index outside 0 .. K_global - 1, index K_global - 1 (the zero-noise / null-action
 * sample), in multi-modal mode index 0 or K/2 (the best-trajectory samples), an index listed twice ("prior 3: sample 17 listed
 * twice"), a non-finite value ("prior 2: step 5 control 1 is not finite"; host variant only); M3_ERR_UNSUPPORTED for a
 * panda_env handle and for a sharded handle (K_local != K_global); M3_ERR_STATE for a sim_only handle.
 * Which kernels run.  A handle with priors set runs the prior build of the general, weighted, run-time-scene rollout instance
 * (rollout_point_priors.hip; with or without an arena per sample, tuned cost weights keep working); the two-wavefront form is
 * never taken; m3_point_rollout_plan_ex(..., priors = 1, ...) reports the launch.  m3_set_point_scene_instance(h, 0) with priors
 * set refuses the next rollout (M3_ERR_STATE).
 * Batched ON REQUEST only (m3p2i_hip_ext.h: M3_BATCH_SECTION_POINT_PRIORS, M3_EPISODES_PRIORS; the controllers that fill the
 * table on the device: m3_set_prior_controller).  Every other batch and set: m3_batch_command with such a handle and
 * m3_episodes_create* / m3_episodes_tick / _begin / _end with such a planner return M3_ERR_UNSUPPORTED (the message names
 * m3_set_prior_samples and the index of the handle); nothing is launched and every handle stays as it was.
 * Memory: the first call on a handle allocates, through the handle's ledger, a device table of M3_MAX_PRIOR_SAMPLES x T x nu
 * floats, a device slot map int[K_local] (-1: no prior), one pinned host block that mirrors both, and the event below; later
 * calls reuse them.  Uploads are hipMemcpyAsync on the handle's stream.  Before the mirror is rewritten the setter waits for
 * the previous upload only, through an event recorded behind it -- not for the stream.  The slot map is uploaded again only when
 * the indices changed.  m3_rollout and m3_command allocate nothing and synchronise nothing because of priors. */
#define M3_MAX_PRIOR_SAMPLES 256
int m3_set_prior_samples(m3_handle* h, const float* seqs, const int* sample_idx, int n);
/* the same with seqs in DEVICE memory (an ancillary controller that runs on the GPU): one device-to-device hipMemcpyAsync on
 * the handle's stream; the values are not inspected (the kernel clamps them; a NaN stays a NaN) */
int m3_set_prior_samples_device(m3_handle* h, const float* seqs_dev, const int* sample_idx, int n);
int m3_prior_samples_set(const m3_handle* h);   /* n (0: none) */
/* prior j as it was set: its sample index and, if seq != NULL, its [T][nu] values (host-set priors only: M3_ERR_STATE with seq
 * != NULL after m3_set_prior_samples_device); M3_ERR_BAD_ARG for j outside 0 .. n - 1 */
int m3_get_prior_sample(const m3_handle* h, int j, int* sample_idx, float* seq);
int m3_prior_samples_used(m3_handle* h);        /* 0 / 1: the last rollout launched the prior build; -1 before the first */
/* EXTENSION, panda_env PLANNER handles, unsharded: PRIOR SAMPLES of the arm -- the same mechanism with nu = 9 (seqs: [n][T][9]),
 * through entry points of its own (the five above keep refusing a panda_env handle: "point_env only").  Sample sample_idx[j]
 * of the next rollouts assembles its control of step t as a = clamp(seqs[j][t][c], u_min[c], u_max[c]) in place of
 * clamp(mean[shift(t)] + noise) -- where the multi-modal planner's best-trajectory select sits, in simple mode behind that
 * branch's clamp -- and everything behind the select is what it is for every sample: the GRIPPER COMMAND's override of controls
 * 7 and 8 (gripper_cmd 1 / 2: +-1.5 -- the task's, so a prior cannot move the fingers while a gripper command is set; with
 * gripper_cmd 0 its columns 7 and 8 are taken), u_scale, what is stored in M3_BUF_ACTIONS, simple mode's e - m perturbation
 * cost, the update.  Both mppi modes, both samplers, single mode and multi-modal (k < K/2 informs mode 1, k >= K/2 mode 2).
 * Nothing is shifted between commands; the priors stay until replaced or cleared (seqs == NULL or n == 0: the handle then
 * launches exactly the kernels it launched before).  The prior follows the SAMPLE: m3_set_rollout_lanes,
 * m3_set_panda_lanes_per_sample, the shadow slots of the reach command (which re-simulate samples 0 and K/2 and take those
 * samples' priors) and the ragged last wavefront do not move it.  Survives m3_reset.
 * Refused as above, the message names the entry: M3_ERR_BAD_ARG for n outside 0 .. M3_MAX_PRIOR_SAMPLES, a null sample_idx, an
 * index out of range, index K_global - 1, in multi-modal mode index 0 or K/2, an index listed twice, a non-finite value (host
 * variant); M3_ERR_UNSUPPORTED for a point_env handle ("panda_env only") and for a sharded handle; M3_ERR_STATE for a sim_only
 * handle.
 * Which kernels run: k_rollout_panda_pr (rollout_panda_priors.hip), one family for a handle with priors -- the workspace and
 * the cost weights kernel arguments, with or without m3_set_panda_rollout_scenes; m3_panda_scene_instance_used reports 1,
 * m3_panda_weighted_cost_instance_used follows the weights.  m3_set_panda_scene_instance(h, 0) or
 * m3_set_panda_weighted_cost_instance(h, 0) with priors set refuses the next rollout (M3_ERR_STATE).
 * Not batched: m3_batch_command with such a handle and m3_panda_episodes_create* / _observe / _act / _act_first with such a
 * planner return M3_ERR_UNSUPPORTED (the message names m3_set_panda_prior_samples and the index of the handle); nothing is
 * launched and every handle stays as it was.
 * Memory, uploads and synchronisation: as for m3_set_prior_samples (the table is M3_MAX_PRIOR_SAMPLES x T x 9 floats). */
int m3_set_panda_prior_samples(m3_handle* h, const float* seqs /* [n][T][9] */, const int* sample_idx, int n);
int m3_set_panda_prior_samples_device(m3_handle* h, const float* seqs_dev, const int* sample_idx, int n);
int m3_panda_prior_samples_set(const m3_handle* h);   /* n (0: none) */
int m3_get_panda_prior_sample(const m3_handle* h, int j, int* sample_idx, float* seq);
int m3_panda_prior_samples_used(m3_handle* h);        /* 0 / 1: the last rollout launched k_rollout_panda_pr; -1 before the first */
/* Diagnostic, host only (no device call, no handle): the blocks -- device, pinned and host memory, events, peer mappings -- that
 * the process's handles, batches and episode sets hold right now.  Every object owns its memory through one ledger; an object's
 * destroy call takes its blocks off the count, so after every object is destroyed the count is what it was before the first. */
long long m3_owned_blocks_live(void);
/* Objective.multi_modal (cost_functions.py:9) for a sim_only handle, whose config does not
 * come from an MPPI object; refused on planner handles (fixed at m3_create) */
int m3_set_multi_modal(m3_handle* h, int multi_modal);
/* warm-start state (means, best trajs, U): which = M3_BUF_MEAN.., host pointer [T][nu] */
int m3_set_plan(m3_handle* h, int which, const float* host_values);
/* the persistent softmin temperature (MPPI.beta, mppi.py:184; adapted by the panda_env's single-mode
 * update, mppi.py:446-454): together with m3_set_plan this restores a saved warm start */
int m3_set_beta(m3_handle* h, float beta);
/* the number of finished commands (m3_info.calls) = the index of the next command in the in-kernel noise stream;
 * with m3_set_plan / m3_set_beta this restores a saved planner state exactly */
int m3_set_call_count(m3_handle* h, unsigned calls);
int m3_reset(m3_handle* h); /* zero means/best/pending forces, beta = 1, call counter = 0 */
/* Where m3_finalize writes the returned plan (`action`, mppi.py:257-263): a caller-owned device
 * buffer of [T][nu] floats ([u_per_command][nu] in simple mode), or NULL for the library's
 * M3_BUF_ACTION_OUT.  The reference returns a fresh tensor per command(); a host wrapper that
 * hands out slots of a small ring through this call gets the same aliasing behaviour without a
 * device-to-device copy per command. */
int m3_set_action_out(m3_handle* h, float* dev_ptr);

/* initial state of every rollout (host values; copied by value into the launch) */
int m3_set_world_point(m3_handle* h, const m3_point_world* w);
/* same in the library's internal layout, 18 floats: robot x y vx vy | box x y cos sin vx vy wz
 * | dyn-obs likewise (no quaternion round trip; used by the bit-parity tests) */
int m3_set_world_point_raw(m3_handle* h, const float* w18);
/* ... or read it from env 0 of the wrapper's device tensors at launch time (zero-copy):
 * dof_state f32 [*,4], root_state f32 [*,n_actors,13] */
int m3_bind_sim_point(m3_handle* h, const float* dof_state_dev, const float* root_state_dev,
                      int n_actors, int box_actor, int dyn_obs_actor);

/* panda_env counterparts.  w57 = q[9] qd[9] | cubeA | cubeB | dyn-obs, each pos3 quat4(xyzw) linvel3 angvel3 (the
 * rows of the wrapper's root-state tensor, isaacgym_wrapper.py:102-104; the plate's orientation and angular velocity
 * are not used: it does not rotate in this world);
 * bind: dof_state f32 [*,18] (pos,vel interleaved), root_state f32 [*,n_actors,13].
 * Whether cubeA starts clamped between the finger pads, and whether a cube sleeps on its support, is inferred from the
 * geometry ("Panda world spec v2"): the wrapper's tensors carry no such bits. */
int m3_set_world_panda_raw(m3_handle* h, const float* w57);
int m3_bind_sim_panda(m3_handle* h, const float* dof_state_dev, const float* root_state_dev,
                      int n_actors, int cubeA_actor, int cubeB_actor, int obs_actor);

/* one MPPI iteration = rollout + update + finalize of an UNSHARDED handle.  action_host: optional
 * [T][nu] (or [u_per_command][nu] in simple mode) host buffer; if non-NULL the call synchronises.
 * M3_ERR_STATE on a sharded handle (K_local != K_global): the collectives go between the phases. */
int m3_command(m3_handle* h, float* action_host);
/* the three phases, for sharded use: rollout -> (all-gather TRAJ_COST into TRAJ_COST_ALL)
 * -> update -> (all-reduce REDUCE) -> finalize.  With K_local == K_global m3_update uses
 * TRAJ_COST itself.  With cfg.shard_mix: rollout -> update -> (all-gather RECORD into
 * RECORDS_ALL) -> finalize: one collective (single-mode and multi-modal alike). */
int m3_rollout(m3_handle* h);
int m3_update(m3_handle* h);
int m3_finalize(m3_handle* h);
/* cfg.shard_mix = 3 (multi-modal, more ranks / samples than the one-collective protocol is meant for): TWO small
 * exchanges per command and O(K_local) work per rank after the first --
 *   m3_rollout, m3_update (as shard_mix = 2: costs | top-k | minima + ladder table into M3_BUF_RECORD)
 *   all-gather M3_BUF_RECORD -> M3_BUF_RECORDS_ALL
 *   m3_update_b   searches on the mixture of the tables; weights of the rank's OWN samples; their weighted action
 *                 sums from its own action buffer (nothing re-generated) + its best rows -> M3_BUF_RECORD_B
 *   all-gather M3_BUF_RECORD_B -> M3_BUF_RECORDS_B_ALL      (~6 T nu floats per rank)
 *   m3_finalize   sums in rank order, best rows from the rank whose best sample wins, the plan.
 * Equal to the unsharded run up to f32 rounding, identical on every rank; M3_BUF_WEIGHTS* hold the rank's own
 * samples' entries.  m3_record_b_len: floats of M3_BUF_RECORD_B. */
int m3_update_b(m3_handle* h);
int m3_record_b_len(const m3_handle* h);

/* ---- device-side exchange of the per-rank records (csrc/p2p.hip) -------------------------------------------------
 * The ONE collective of a sharded command (the all-gather of the records between m3_update and m3_finalize;
 * SURVEY.md section 8(e), replaces nothing in the reference: it has no multi-GPU path) without a
 * communication library: every rank owns an exchange block in device memory, maps every peer's block (hipIpc between
 * processes, direct pointers inside one), and an exchange is two small kernels on the handle's stream -- put: this
 * rank's record into its slot of every peer's block (one hop over xGMI) + a release flag; wait: acquire every
 * peer's flag of this exchange (bounded: a missing peer sets an error word after a time-out instead of hanging the
 * GPU).  The m3_finalize that follows reads the records from the block.  Selectable beside RCCL
 * (m3p2i_aip_amd.distributed.attach_p2p / attach_collectives); the records phase of cfg.shard_mix 1 and 2 and
 * of single-mode sharding.
 *   m3_p2p_export         this rank's block as an IPC handle (allocates it: uncached device memory)
 *   m3_p2p_connect        all ranks' handles, in rank order (the own entry is ignored)
 *   m3_p2p_connect_local  the same for handles that live in THIS process (peers[p] = handle of rank p)
 *   m3_p2p_put / _wait    the two halves (a process that drives several handles enqueues every put before any wait)
 *   m3_p2p_exchange       put + wait
 *   m3_p2p_status         synchronises; missing_rank = -1 or the rank a wait gave up on; memory_kind 1 uncached,
 *                         2 fine-grained, 3 plain device memory
 *   m3_p2p_set_timeout_ms how long a wait spins before it gives up: `first_ms` for a channel's FIRST exchange (the
 *                         ranks of a job reach their first command at different times: default 30 000), `ms` for every
 *                         later one (default 500; peers are then at most one command apart).  1 .. 600 000 each. */
typedef struct { unsigned char bytes[64]; } m3_ipc_handle;
int m3_p2p_export(m3_handle* h, m3_ipc_handle* out);
int m3_p2p_connect(m3_handle* h, const m3_ipc_handle* all, int n_ranks);
int m3_p2p_connect_local(m3_handle* h, m3_handle* const* peers, int n_ranks);
int m3_p2p_put(m3_handle* h);
int m3_p2p_wait(m3_handle* h);
int m3_p2p_exchange(m3_handle* h);
/* channel 0: M3_BUF_RECORD (== the three above); channel 1: M3_BUF_RECORD_B, the second exchange of shard_mix = 3 */
int m3_p2p_put_ch(m3_handle* h, int channel);
int m3_p2p_wait_ch(m3_handle* h, int channel);
int m3_p2p_exchange_b(m3_handle* h);
int m3_p2p_status(m3_handle* h, int* missing_rank, int* memory_kind);
int m3_p2p_set_timeout_ms(m3_handle* h, int first_ms, int ms);
/* Recovery after a wait that gave up (sticky error word; the finalize kernels hand out NaN plans while it is set).
 * m3_p2p_clear_error: synchronises the stream, zeroes the OWN block's flags and error word and restarts the sequence
 * numbers -- a COLLECTIVE step: every rank calls it, with a barrier of the caller's (host side) before (nobody is still
 * exchanging) and after (nobody puts into a block about to be zeroed); distributed.p2p_recover does exactly that.
 * m3_p2p_connect / m3_p2p_connect_local on a connected handle re-arm the same way.
 * m3_p2p_detach: this handle stops using the device-side exchange (blocks stay mapped): the finalize kernels no longer
 * read the error word, the records come from M3_BUF_RECORDS_ALL again (an RCCL all-gather) -- distributed.detach_p2p. */
int m3_p2p_clear_error(m3_handle* h);
int m3_p2p_detach(m3_handle* h);
/* where the exchange block's allocation chain starts: 1 (default) uncached device memory, 2 fine-grained, 3 plain
 * device memory (fenced puts / waits); before the block exists (m3_p2p_export / connect), else M3_ERR_STATE.  For the
 * tests of the fallback kinds; m3_p2p_status reports the kind the block ended on. */
int m3_p2p_set_memory_kind(m3_handle* h, int first_kind);
/* m3_update + m3_finalize for an UNSHARDED handle in as few launches as the sizes allow (what
 * m3_command does after its rollout): for a caller that fills TRAJ_COST / ACTIONS itself (step mode,
 * planner._command_step).  M3_ERR_STATE on a sharded handle (the collectives go in between). */
int m3_update_finalize(m3_handle* h);

/* ---- batched command: many independent planners of one environment in one launch -----------------------------------
 * m3_batch_command runs one m3_command of each of hs[0..n-1] -- per group of handles whose own command would run the same
 * kernel instance and build ONE rollout launch and ONE update launch (a multi-modal group: one per residency chunk,
 * DESIGN.md "Batched command").  One environment per call: handle 0's.  point_env groups: the general or the per-task
 * rollout instance, reference scene compiled in or not, K, T, lanes.  panda_env groups: the kernel form each handle's
 * own m3_rollout would choose from its own busy report and hysteresis, or its m3_set_panda_lanes_per_sample /
 * m3_set_panda_reach_cost_kernel overrides (lanes per sample, instance, shadow slots, reach-cost record kept), K, T and
 * lanes per wavefront; a group that keeps the record adds one reach-cost launch, which m3_batch_launches does not count.
 * Update: k_update_small's template arguments, nu and workgroup width.  Mixed tasks and sizes are allowed; the grouping
 * is internal.  Each handle's results are bit-identical to what its own m3_command(hs[i], NULL) would have left: plans,
 * buffers, m3_info, wave-order refresh, update_cov step, m3_set_action_out destination, `calls` + 1, and for panda_env
 * m3_panda_lanes_per_sample_used and m3_panda_near_share.  The handles keep all of their state; the batch adds no
 * planner state, only device workspace (allocated by m3_batch_create, its table slots sized for either environment; a
 * call allocates nothing beyond the lazy allocations m3_command itself makes on a handle's first command).  Handles not
 * listed are not touched: the list may change from call to call.
 * Every check comes before any launch; on a refusal every handle is left as it was:
 *   M3_ERR_BAD_ARG      null batch / handle list / handle, n <= 0, n > max_handles, a handle listed twice, a handle on
 *                       another device
 *   M3_ERR_STATE        a sharded or sim_only handle, handles whose streams differ, and whatever makes m3_rollout refuse
 *                       (no noise set, push_pull without multi_modal)
 *   M3_ERR_UNSUPPORTED  a handle of the other environment than handle 0's, a handle whose command does not take the
 *                       one-launch update (nu = 2: K <= 16384, multi-modal K <= 8192; nu = 9: K <= 4096; T * nu <= 2048)
 * The message (m3_batch_last_error) names the offending index.  All work is enqueued on the handles' common stream.
 * actions_host: NULL, or a host buffer that receives the handles' plans one after the other, [rows][nu] each (rows =
 * u_per_command in simple mode, else T: [n][rows][nu] when all agree); the call then synchronises.
 * Per-handle timing (m3_enable_timing / m3_get_timing) is NOT updated by a batched call.
 *
 * m3_batch_create_ex(device, max_handles, flags, &out): flags == 0 is m3_batch_create; unknown bits are M3_ERR_BAD_ARG.
 * M3_BATCH_PANDA_RUNTIME sizes the table slots and the host scratch for a second section of panda_env entries as well, and
 * m3_batch_command on such a batch accepts, besides everything else, an unsharded panda_env planner handle that needs the
 * run-time-scene instance (m3_set_panda_scene), the weighted family (m3_set_panda_cost_weights), both, or has a workspace per
 * sample (m3_set_panda_rollout_scenes).  Every other refusal above stays, in the same order -- among them the "forced off"
 * ones of m3_set_panda_scene_instance(h, 0) / m3_set_panda_weighted_cost_instance(h, 0) (M3_ERR_STATE) -- and so does the
 * contract: each handle's results are bit-identical to its own m3_command's, m3_panda_scene_instance_used and
 * m3_panda_weighted_cost_instance_used included, set as m3_rollout sets them.  Such handles group by family (literal, weighted
 * on the run-time scene, workspace per sample) ahead of the fields above; a handle with the default workspace and weights
 * runs the kernel it runs in any batch.  point_env handles with an arena per sample stay refused by the batches of this
 * header; m3p2i_hip_ext.h declares the call that makes a batch which takes them. */
#define M3_BATCH_PANDA_RUNTIME 1
typedef struct m3_batch m3_batch;
int m3_batch_create(int device, int max_handles, m3_batch** out);   /* all device + pinned workspace allocated here */
int m3_batch_create_ex(int device, int max_handles, int flags, m3_batch** out);
int m3_batch_flags(const m3_batch* b);   /* the flags it was created with; M3_ERR_BAD_ARG for NULL */
void m3_batch_destroy(m3_batch* b);
const char* m3_batch_last_error(const m3_batch* b);   /* b may be NULL: the last failed m3_batch_create on this thread */
int m3_batch_command(m3_batch* b, m3_handle* const* hs, int n, float* actions_host);
/* rollout-kernel and update launches of the last successful m3_batch_command (panda reach-cost launches not counted) */
int m3_batch_launches(const m3_batch* b, int* rollout_launches, int* update_launches);

/* ---- batched closed-loop episodes (point_env): N episodes of tools/closed_loop.run in lockstep --------------------------
 * One N-env "real world" (a sim_only point_env handle with K_local == n and bound views: the engine of an
 * IsaacGymWrapper(num_envs=n)), row e the 1-env world of episode e, planned by planners[e].  m3_episodes_tick runs one tick
 * of every episode: a pre-command kernel (dyn-obs walk with the episode's phase, success test, suction-gate snapshot), one
 * m3_batch_command of the planners whose episodes were still running after the last tick, a post-command kernel (trace
 * row, suction, step, collision count), one copy of the status words to pinned memory and ONE host synchronisation.
 * Before every batched command each planner is bound (m3_bind_sim_point) to its row of the world.  An episode ends at its
 * success tick (before its command, as closed_loop.run) or after the step of tick max_ticks - 1; an ended episode's
 * metrics are frozen and its planner leaves the next tick's batch (its world row keeps evolving, unrecorded).
 * A planner's first command (the fused / step probe) is the caller's: m3_episodes_begin (pre kernel + status, synchronises)
 * and m3_episodes_end (post kernel + status, synchronises) frame a tick whose commands the caller issues itself.
 * Each planner's m3_set_action_out destination is read at create and must stay the same at every tick.
 * m3_episodes_create refuses, before any launch and leaving every handle as it was: a world that is not a sim_only
 * point_env handle with bound views or whose K_local differs from n (M3_ERR_STATE), a panda_env planner (M3_ERR_UNSUPPORTED),
 * a planner m3_batch_command would refuse (its code), a handle on another stream than the world's, a handle listed twice,
 * a planner without an action-out destination, n <= 0, max_ticks <= 0, a bad spec (M3_ERR_BAD_ARG / M3_ERR_STATE).
 * All device and pinned memory is allocated by m3_episodes_create; a tick allocates nothing beyond what the planners' own
 * first commands allocate. */
typedef enum { M3_SUCTION_OFF = 0, M3_SUCTION_ON = 1, M3_SUCTION_PULL_PREFERENCE = 2 } m3_suction_mode;
typedef struct {
    int task;            /* M3_TASK_NAVIGATION .. M3_TASK_PUSH_PULL: what PLANNER_SIMPLE checks for success */
    float goal[2];
    int dyn_phase;       /* the dyn-obs walk of tick i is that of tick i + dyn_phase (>= 0) */
    int suction;         /* m3_suction_mode: push / navigation off, pull on, push_pull the previous pull preference */
    float kp_suction;
} m3_episode_spec;
typedef struct {
    int done_tick;       /* -1 while running; else the success tick or max_ticks - 1 */
    int success;
    int collision_ticks; /* ticks with |Fx| + |Fy| > 0.1 on the dyn-obs after the step */
    float final_pos[2];  /* box x, y (robot x, y for navigation) at the end, f32 */
} m3_episode_status;
typedef struct m3_episodes m3_episodes;
int m3_episodes_create(m3_handle* world, m3_handle* const* planners, const m3_episode_spec* specs, int n, int max_ticks,
                       int trace, m3_episodes** out);
int m3_episodes_tick(m3_episodes* eps, m3_batch* batch);
int m3_episodes_begin(m3_episodes* eps);
int m3_episodes_end(m3_episodes* eps);
/* status_out [n] (host); trace_out (host, may be NULL) [max_ticks][n][10] floats: robot x, y, box x, y, qz, qw, dyn-obs x,
 * y, action x, y -- rows of ticks an episode did not trace are undefined.  Synchronises. */
int m3_episodes_status(m3_episodes* eps, m3_episode_status* status_out, float* trace_out);
int m3_episodes_ticks_done(const m3_episodes* eps);
int m3_episodes_running(const m3_episodes* eps);   /* episodes not ended as of the last status copy (no synchronisation) */
void m3_episodes_destroy(m3_episodes* eps);
const char* m3_episodes_last_error(const m3_episodes* eps);   /* eps may be NULL: the last failed create on this thread */

/* ---- batched closed-loop episodes (panda_env): N reactive pick-and-place episodes in lockstep -----
 * world: a sim_only panda_env handle with K_local == n and bound views, row e the 1-env world of episode e, planned by
 * planners[e].  The task planner stays on the host and decides per tick, so a tick is TWO calls with the host in between:
 *   m3_panda_episodes_observe: the pre kernel -- per running episode, row e of the world's views advanced by one step of
 *     the planner's own simulator (under the targets that simulator kept since tick 0) into row e of the set's planning
 *     view (dof, root and rigid-body state) -- then ONE copy of the planning view's rigid-body rows to pinned host memory
 *     (*rb_host: [n][17][13] floats, valid until the next observe) and one synchronisation;
 *   the host: its n task planners on those rows, m3_set_objective on every planner that goes on, ended[e] != 0 for every
 *     episode whose task is done at this tick;
 *   m3_panda_episodes_act: every running, not-ended planner bound (m3_bind_sim_panda) to its row of the planning view, ONE
 *     m3_batch_command, the post kernel (running: trace row, step under row 0 of the planner's action-out; ended: up to
 *     settle_ticks steps under zero targets, one per tick, after which its row of the world is not stepped any more -- the
 *     cubeA / cubeB positions of the status are frozen from there on; an episode
 *     still running at tick max_ticks - 1 ends unsuccessful after that step).  No synchronisation.
 * Tick 0 is the caller's (each planner's first command is the fused / step probe on its own simulator):
 * m3_panda_episodes_act_first launches no command; sims[e] is planner e's K-env simulator handle, whose kept velocity
 * targets of row 0 become episode e's for every later observe.
 * m3_panda_episodes_create refuses, before any launch and leaving every handle as it was: a world that is not a sim_only
 * panda_env handle with bound views or whose K_local differs from n (M3_ERR_STATE), a point_env planner
 * (M3_ERR_UNSUPPORTED), a planner m3_batch_command would refuse (its code), a handle on another stream or device than the
 * world's, a handle listed twice, a planner without an action-out destination, n <= 0, max_ticks <= 0, settle_ticks < 0.
 * All device and pinned memory comes from create; observe / act allocate nothing. */
typedef struct {
    int phase;           /* 0 running, 1 ended and settling, 2 ended and settled: cubeA / cubeB are valid */
    int done_tick;       /* -1 while running; else the success tick or max_ticks - 1 */
    int success;
    int settle_left;     /* settle steps still to take */
    float cubeA[3];      /* rigid-body position of cubeA / cubeB in the episode's row of the world, f32: filled by */
    float cubeB[3];      /* m3_panda_episodes_status; with phase 2 the positions after the episode's last step, for good */
} m3_panda_episode_status;
#define M3_PANDA_EPISODE_TRACE_FLOATS 132   /* dof_state 18 | root_state 91 | action 9 | panda_hand pose 7 | cubeA body pose 7 */
typedef struct m3_panda_episodes m3_panda_episodes;
int m3_panda_episodes_create(m3_handle* world, m3_handle* const* planners, int n, int max_ticks, int settle_ticks, int trace,
                             m3_panda_episodes** out);
/* A set that also takes run-time workspaces, tuned weights and workspaces per row (M3_PANDA_EPISODES_RUNTIME) is made by the
 * _create_ex form of this call, declared in include/m3p2i_hip_ext.h; every call below serves both kinds of set. */
int m3_panda_episodes_observe(m3_panda_episodes* eps, const float** rb_host);
int m3_panda_episodes_act(m3_panda_episodes* eps, m3_batch* batch, const int* ended_host /* [n] */);
int m3_panda_episodes_act_first(m3_panda_episodes* eps, m3_handle* const* sims /* [n] */, const int* ended_host /* [n] */);
/* status_out [n] (host); trace_out (host, may be NULL) [max_ticks][n][M3_PANDA_EPISODE_TRACE_FLOATS], rows of ticks an
 * episode did not step while running are undefined.  Synchronises; not between observe and act (it reuses the pinned
 * host copy, which also ends the validity of the last observe's rows). */
int m3_panda_episodes_status(m3_panda_episodes* eps, m3_panda_episode_status* status_out, float* trace_out);
int m3_panda_episodes_ticks_done(const m3_panda_episodes* eps);
int m3_panda_episodes_running(const m3_panda_episodes* eps);   /* episodes the host has not ended (host mirror, no synchronisation) */
int m3_panda_episodes_active(const m3_panda_episodes* eps);    /* ... plus those still settling */
void m3_panda_episodes_destroy(m3_panda_episodes* eps);
const char* m3_panda_episodes_last_error(const m3_panda_episodes* eps);   /* eps may be NULL: the last failed create on this thread */

int m3_get_buffer(m3_handle* h, int which, void** dev_ptr, long long* nbytes);
int m3_reduce_len(const m3_handle* h);
int m3_record_len(const m3_handle* h);
int m3_get_info(m3_handle* h, m3_info* out);     /* synchronises the stream */
int m3_get_timing(m3_handle* h, m3_timing* out); /* synchronises the stream */

/* ---- step mode: the K rollout environments as an IsaacGymWrapper-like simulator ---- */
/* bind the wrapper's torch-owned views (device pointers, may be NULL to skip a view):
 * dof_state [Kl][2*ndof], root_state [Kl][nA][13], rigid_body_state [Kl][nB][13],
 * net_contact_force [Kl][nB][3] */
int m3_sim_bind_views(m3_handle* h, float* dof_state, float* root_state,
                      float* rigid_body_state, float* net_contact_force, int n_actors,
                      int n_bodies);
int m3_sim_pull_state(m3_handle* h); /* views -> internal state (set_*_state_tensor) */
/* update_dyn_obs (isaacgym_wrapper.py:205-220): root position of one actor of every environment shifted by
 * (dx, dy, dz) in the bound root_state view, followed by m3_sim_pull_state -- one launch (point_env) */
int m3_sim_shift_actor(m3_handle* h, int actor, float dx, float dy, float dz);
int m3_sim_push_state(m3_handle* h); /* internal state -> views (refresh_*) */
int m3_sim_set_velocity_target(m3_handle* h, const float* u_dev /* [Kl][nu] */);
int m3_sim_apply_body_forces(m3_handle* h, const float* f_dev /* [Kl][nB][3] */);
int m3_sim_step(m3_handle* h);       /* one step(): dt with substeps, then push views */
/* m3_sim_set_velocity_target(h, u) + m3_sim_step(h) in one launch: the targets are read from u (device,
 * [K_local][nu]) when the step runs and stay in force for later steps */
int m3_sim_step_with_target(m3_handle* h, const float* u);
int m3_cost(m3_handle* h, float* cost_dev /* [Kl] */); /* Objective.compute_cost */
/* the 1-env "real world" of scripts/sim.py:41-49 (point_env), evaluated on the device:
 * calculate_suction (utils/skill_utils.py:59-94): forces_dev f32 [Kl][nB][3] is overwritten with the
 * suction pair (box row, last body's row); threshold 1.5 for a 1-env handle, 1.8 otherwise. */
int m3_sim_suction_forces(m3_handle* h, float kp_suction, float* forces_dev);
/* check_suction_condition + check_and_apply_suction (utils/skill_utils.py:36-56): per environment, the
 * robot is within 0.6 of the box and action . (robot - box) > 0; where that holds and apply != 0 the
 * suction pair becomes the pending body force of the next m3_sim_step.  action_dev f32 [Kl][2];
 * applied_dev i32 [Kl] (optional) receives the condition.  enabled_dev (optional): one i32 on the device that
 * must be non-zero for the suction to act -- cfg.suction_active (sim.py:44-47) taken straight from the
 * planner's m3_info.pull_preference (M3_BUF_INFO) instead of through the host.  No host synchronisation. */
int m3_sim_check_and_apply_suction(m3_handle* h, const float* action_dev, float kp_suction, int apply,
                                   int* applied_dev, const int* enabled_dev);

/* Read-only: the wavefront order the LAST m3_rollout / m3_command of the handle went by -- order_dev[slot] = local index of
 * the sample that lane slot `slot` simulated (device memory, i32 [*n], *n = K_local; owned by the handle, valid until its
 * next rollout).  NULL and 0 when that rollout went by index: order off (m3_set_wave_order), samples relabelled
 * (m3_relabel_samples: index order IS wavefront order then), K_local < 128, random sampling, simple mode, noise uploaded
 * for almost every command, panda_env, or no rollout yet.  Synchronises the handle's stream.  For tests and tools. */
int m3_wave_order(m3_handle* h, const int** order_dev, int* n);

/* ---- sample groups (extension): one control sequence in M models, the costs aggregated ----
 * group_of [n], n == K_local: group_of[k] in 0 .. K-1 names the group of sample k (the ids are labels), -1 leaves it on its own.
 * A group has 2 .. 16 members.  After every m3_rollout (so inside m3_command, ahead of the update) each group's member costs in
 * M3_BUF_TRAJ_COST are replaced, in every member, by the mean of the group's j = max(1, ceil(worst_frac * M_g)) LARGEST member
 * costs: worst_frac = 1 the mean, <= 1/16 the maximum, in between a CVaR-style tail mean; a NaN member makes the aggregate NaN.
 * The arithmetic is a spec (csrc/sample_groups.hpp): descending sort, the fixed SUM16 tree, one binary32 division.  The update
 * then runs unchanged on K costs, so a group counts M_g times in the softmin and a sample on its own once.  That the members of
 * a group carry the same controls (the same noise rows) is the caller's arrangement.  NULL clears the groups: the handle runs
 * exactly the kernels of a handle that never had any.  Everything is validated before any state changes, all memory comes from
 * this call (none from a command), the groups survive m3_reset.
 * M3_ERR_BAD_ARG: n != K_local, an id outside -1 .. K-1, a group of 1 or of more than 16 members, sample K-1 (zero-noise /
 * null-action) or, multi-modal, samples 0 and K/2 (best trajectories) inside a group, a multi-modal group with members on both
 * sides of K/2, worst_frac outside (0, 1].  M3_ERR_UNSUPPORTED: a sharded or sim_only handle, mode_simple / sampling_random
 * (the noise is a function of the sample index), a handle with prior samples or a prior controller -- and the prior setters,
 * m3_batch_command and both lockstep episode sets refuse a handle that has groups. */
int m3_set_sample_groups(m3_handle* h, const int* group_of, int n, float worst_frac);
int m3_sample_groups_set(m3_handle* h);   /* the number of groups, 0: none */
/* sample k's group id as given (-1: on its own), the group's size (1) and its j (1); any pointer may be NULL */
int m3_get_sample_group(const m3_handle* h, int k, int* group, int* size, int* worst_j);
/* device, f32 [K_local], owned by the handle: the per-model costs of the last rollout, as they were before the aggregation
 * (samples on their own included).  M3_ERR_STATE before the first m3_set_sample_groups. */
int m3_sample_group_raw_costs(m3_handle* h, const float** dev);
/* the aggregation alone, on whatever M3_BUF_TRAJ_COST holds (for callers who write the costs themselves, and for tests);
 * M3_ERR_STATE without groups */
int m3_aggregate_sample_groups(m3_handle* h);


#ifdef __cplusplus
}
#endif
#endif
