// m3_internal.hpp -- structures shared by the kernels and the C-ABI host code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "../../include/m3p2i_hip.h"
#include "../../include/m3p2i_hip_ext.h"
#include "planar_dyn.hpp"
#include "point_cost.hpp"
#include "panda_dyn.hpp"
#include "panda_scene.hpp"
#include "owned_blocks.hpp"
#include "panda_variant.hpp"
#include "update_plan.hpp"

namespace m3 {

// ---- kernel argument blocks (passed by value; wave-uniform, live in SGPRs) -------------
struct RolloutArgs {
    int Kg, Kl, k0, T, nu;
    int multi_modal, mode_simple, sampling_random, sample_null_action;
    int gripper_cmd;
    float u_min[M3_MAX_NU], u_max[M3_MAX_NU], scale_tril[M3_MAX_NU], sigma_inv[M3_MAX_NU];
    float u_scale, gamma, lambda_;
    // the MPPIConfig switches no shipped config turns on (general kernel instance only)
    int noise_abs_cost, full_sigma;
    float noise_mu[M3_MAX_NU];
    const float* noise_mats;  // device [2][nu][nu]: Cholesky factor | inverse of noise_sigma (full_sigma)
    const float* scale_dev;   // device [nu] scale_tril when update_cov rewrites it every command, else null
    unsigned long long seed;
    unsigned call;
    CostParams cp;
    int lanes;                // active lanes (= samples) per 64-wide wavefront: 1..64
    float world0[18];         // rx ry rvx rvy | B: x y c s vx vy w | D: x y c s vx vy w
    // if sim_dof != null the initial world is read from env 0 of the wrapper's tensors
    // (dof_state [*,4], root_state [*,nA,13]) inside the kernel: no upload, no extra launch
    const float* sim_dof;
    const float* sim_root;
    int sim_box, sim_dyn;
    const float* delta;       // [T][Kl][nu], rows in lane-slot order when `order` is set
    const int* order;         // [Kl] lane -> local sample (null = identity)
    const float* mean;        // [T][nu] (U in simple mode)
    const float* mean1;
    const float* mean2;
    const float* best1;
    const float* best2;
    float* pend;              // [4][Kl]
    float* states;            // [T][Kl][4]
    float* actions;           // [T][Kl][nu]
    float* cost_h;            // [T][Kl]
    float* J;                 // [Kl]
    float* wave_min;          // [workgroups][3] minima of each workgroup's costs (wave_min.hpp), or null
};

struct SearchOut;
struct VI {  // (cost, global sample index) candidate of the top-k selection
    float v;
    int i;
};

struct UpdateArgs {
    VI* cand;         // [n_cand][M3_TOPK] per-workgroup top-k candidates (stage A -> stage B)
    float* part_min;  // [n_mins][3] per-workgroup minima (all, first half, second half)
    int n_mins;       // workgroups of k_mins
    int n_cand;       // top-k stage-A workgroups
    float* lad;       // [n_lad][96][3] per-workgroup eta sums on the beta ladders (k_ladder)
    int n_lad;        // workgroups of k_ladder
    struct SearchOut* srch;  // beta / eta / minima found by k_search (split path, K > 8192 multi-modal)
    float* apart;     // [apply_workgroups][8] partial half sums and argmax keys of k_apply_weights
    float* wpart;     // [n_chunk][3][T][nu] partial weighted sums of k_wsum (n_chunk > 1 only)
    int* wcount;      // [T] arrival counters of the k_wsum chunks + [T] the launch-wide one of the
                      // fused finalize (zero between launches)
    int fuse_finalize;  // k_wsum's last workgroup also does k_finalize's work (unsharded m3_command)
    int ladder_spins;   // k_update_small: bound of the wait for the other workgroups' ladder points
    int* lflag;         // [n_lad] k_ladder_search: epoch of the launch whose partial table the ladder workgroup has stored
    int epoch;
    int n_chunk;      // k_wsum workgroups per time step
    int lds_floats;   // costs staged in dynamic LDS by k_weights (set by launch_weights)
    int Kg, Kl, k0, T, nu;
    int multi_modal, mode_simple, env_type, filter_u, u_per_command;
    float lambda_, step_size_mean;
    const float* Jall;   // [Kg]
    float* w;            // [Kg]
    float* w1;           // [Kg/2]
    float* w2;           // [Kg - Kg/2]
    int* top_idx;        // [M3_TOPK]
    m3_info* info;       // device
    const float* actions;  // [T][Kl][nu]
    const float* states;   // [T][Kl][4]
    float* reduce;         // packed partial sums, see reduce_layout()
    float* mean;
    float* mean1;
    float* mean2;
    float* best;
    float* best1;
    float* best2;
    float* action_out;   // [T][nu]
    const int* p2p_err;  // device-side exchange attached: its sticky error word (a rank that never arrived: the records hold NaN)
    float* top_trajs;    // [M3_TOPK][T][2]
    // shard_mix (one-collective sharding; which launch sees which view: update_plan.hpp): k_weights / top-k see the LOCAL shard (Kg = Kl,
    // Jall = local costs, w = weights + k0); kbase maps their sample numbers to global indices
    int kbase;           // global index of sample 0 of the costs k_weights sees (0 unless shard_mix)
    int half_g;          // global K/2 (mode split, pull preference)
    float* record;       // this rank's record (null unless shard_mix)
    const float* records_all;  // [n_ranks][record_len]
    int n_ranks, rank;
    float* top_dst;      // where top-k stage B writes the rows: top_trajs (unsharded) or the
                         // reduce buffer's top section (sharded: summed over ranks first)
    float* rec_topj;     // where topk_finish leaves the sorted top-k costs / indices for the other
    float* rec_topi;     //   ranks (inside this rank's record; null: nowhere)
    // ---- "regen" one-collective sharding (multi-modal): after ONE all-gather of records
    // {J of the shard | its top-k} every rank runs the whole update on all K samples; the actions of
    // the other ranks' samples are RE-GENERATED from the replicated noise table and plan instead of
    // being communicated (a_k[t] is a function of the global sample index: mppi.py:381-416)
    int regen;           // 1: the launch covers all K_global samples (Kl == Kg, k0 == 0 in this struct; UPDATE_VIEW_ALL of update_plan.hpp)
    int fast;            // shard_mix = 2: the records carry per-rank minima + ladder tables; the search mixes them
                         // instead of re-evaluating all K costs, and ONE kernel does weights + sums + finalize
    float* rec_mins;     // this rank's record: minima [4] and ladder table [LAD_N][3] (pre-gather launch)
    float* rec_table;
    int Kls;             // samples per shard (= per rank)
    int rec_len;         // floats per gathered record
    const float* noise_all;  // [n_ranks][T][Kls][nu]: every shard's noise block
    float* Jout;             // regen: k_mins (the first reader of the gathered records) leaves the costs
                             // here as one [K_global] array (== Jall of the later launches)
    float u_min[M3_MAX_NU], u_max[M3_MAX_NU], scale_tril[M3_MAX_NU];
    float u_scale;
    int sample_null_action, gripper_cmd;
    // ---- shard_mix = 3 (two small exchanges, O(K_local) work after the first): the second record of this rank,
    // {-w, index of its best sample per weight set (3 pairs) | its half sums (2)} + its weighted sums and best rows
    float* rec_b;              // k_apply_weights' combine leaves the 8-float header here (null: not this protocol)
    const float* recb_all;     // [n_ranks][recb_len] after the second exchange
    int recb_len;
};
// record B (shard_mix = 3): header | [3][T][nu] weighted sums of the LOCAL shard (globally normalised weights) |
// [3][T][nu] action rows of the local best samples
constexpr int RECB_HDR = 8;
__host__ __device__ inline int recb_length(int T, int nu) { return (RECB_HDR + 6 * T * nu + 3) / 4 * 4; }

// REDUCE buffer: [3][T][nu] weighted sums (all, mode 1, mode 2) | [3][T][nu] best rows
// (best, best_1, best_2; zero unless this rank owns the row) | [TOPK][T][2] top trajectories
__host__ __device__ inline int reduce_off_psum(int which, int T, int nu) { return which * T * nu; }
__host__ __device__ inline int reduce_off_best(int which, int T, int nu) { return (3 + which) * T * nu; }
__host__ __device__ inline int reduce_off_top(int T, int nu) { return 6 * T * nu; }
__host__ __device__ inline int reduce_length(int T, int nu) { return 6 * T * nu + M3_TOPK * T * 2; }
// shard_mix record: header | REDUCE-shaped body
//   [0] min cost m_r  [1] eta_r  [2],[3] half sums of the local weights  [4] best index (int bits)
//   [8..28) top-k costs  [28..48) top-k global indices (int bits)
constexpr int REC_HDR = 48, REC_TOPJ = 8, REC_TOPI = 28;
__host__ __device__ inline int record_length(int T, int nu) { return REC_HDR + reduce_length(T, nu); }
constexpr int MIX_MAX_RANKS = 32;
// beta ladders of the multi-modal search: 0.9^j (j = 0..63) and 1.2^j (j = 1..32), see update.hip
constexpr int LAD_S = 64, LAD_G = 32, LAD_N = LAD_S + LAD_G;
// regen record: [Kls] trajectory costs of the shard | [TOPK] its smallest costs | [TOPK] their global
// indices (int bits) | [TOPK][T][2] their (x, y) trajectories | [4] the shard's minima (all / mode 1 /
// mode 2 / pad) | [LAD_N][3] its eta(beta) sums on the ladders relative to those minima (the last two only
// with shard_mix = 2); length padded to a multiple of 4 floats
__host__ __device__ inline int regen_off_topj(int Kls) { return Kls; }
__host__ __device__ inline int regen_off_topi(int Kls) { return Kls + M3_TOPK; }
__host__ __device__ inline int regen_off_trajs(int Kls) { return Kls + 2 * M3_TOPK; }
__host__ __device__ inline int regen_off_mins(int Kls, int T) { return Kls + 2 * M3_TOPK + M3_TOPK * T * 2; }
__host__ __device__ inline int regen_off_table(int Kls, int T) { return regen_off_mins(Kls, T) + 4; }
__host__ __device__ inline int regen_record_length(int Kls, int T) { return (regen_off_table(Kls, T) + LAD_N * 3 + 3) / 4 * 4; }

// ---- batched command (m3_batch_command): the per-handle entries of the device argument table ----------------------
// The variant of the point_env rollout kernels a handle runs, decided in one place (m3_api.hip: point_variant): the reference's
// arena and cost weights compiled in; the handle's cost weights a kernel argument (m3_set_point_cost_weights); the handle's
// arena a kernel argument as well (m3_set_point_scene -- always with the weights).  Also the order of the table's sections.
enum PointVariant { POINT_PLAIN = 0, POINT_WEIGHTED = 1, POINT_SCENE = 2, POINT_VARIANTS = 3 };
// one point_env handle's rollout: the arguments, the variant's scene (not read by the _ref build) and, for the variants that
// carry them, the handle's cost weights behind it
template <class SC, bool WEIGHTED>
struct BatchRolloutEntryT {
    static constexpr bool weighted = true;
    RolloutArgs a;
    SC sc;
    PointCostWeights wt;
};
template <class SC>
struct BatchRolloutEntryT<SC, false> {
    static constexpr bool weighted = false;
    RolloutArgs a;
    SC sc;
};
using BatchRolloutEntry = BatchRolloutEntryT<PointScene, false>;
using BatchRolloutEntryW = BatchRolloutEntryT<PointScene, true>;
using BatchRolloutEntryS = BatchRolloutEntryT<PointSceneRT, true>;
// (the kernels read the table by these offsets: they are what they were when the three were written out by hand)
static_assert(sizeof(RolloutArgs) == 528 && sizeof(BatchRolloutEntry) == 584 && offsetof(BatchRolloutEntry, sc) == 528, "");
static_assert(sizeof(BatchRolloutEntryW) == 616 && offsetof(BatchRolloutEntryW, sc) == 528 &&
              offsetof(BatchRolloutEntryW, wt) == 580, "");
static_assert(sizeof(BatchRolloutEntryS) == 760 && offsetof(BatchRolloutEntryS, sc) == 528 &&
              offsetof(BatchRolloutEntryS, wt) == 724, "");
// a point_env handle with an arena per sample (m3_set_point_rollout_scenes), in a batch created with the per-sample section:
// what BatchRolloutEntryS holds -- sc read for its uniform members only -- and the handle's OWN device table of rows
// [POINT_SCENE_ROW_WORDS][K_local] (point_scene_rows.hpp); the batch stores no rows
struct BatchRolloutEntrySV {
    RolloutArgs a;
    PointSceneRT sc;
    PointCostWeights wt;
    const float* rows;
};
static_assert(sizeof(BatchRolloutEntrySV) == 768 && offsetof(BatchRolloutEntrySV, sc) == 528 &&
              offsetof(BatchRolloutEntrySV, wt) == 724 && offsetof(BatchRolloutEntrySV, rows) == 760, "");
// the k_update_small instance (template arguments, workgroup width, top-k workgroups) an unsharded command takes:
// launch_update_small launches it, m3_batch_command groups the handles by it
struct SmallUpdateInstance {
    int nu, multi, jr, wt, n_cand;
};
SmallUpdateInstance update_small_instance(const UpdateArgs& a);
// blocks of the batched multi-modal update that are resident per CU (update_small.hip; DESIGN.md "Batched command")
int update_small_batch_blocks_per_cu(const SmallUpdateInstance& in);
// the same for the nu = 9 (panda_env) instances, kb_update_small9
int update_small9_batch_blocks_per_cu(const SmallUpdateInstance& in);
// one launch of k_update_small's body for n handles whose entries (tab[0 .. n-1], device) share `in` and T (and nu)
void launch_update_small_batch(const UpdateArgs* tab, int n, const SmallUpdateInstance& in, int T, hipStream_t s);
// the form a rollout launch takes (plan_rollout_point, plan_rollout_panda); launches nothing: m3_rollout launches it at once,
// m3_batch_command groups the handles by it
struct RolloutPlan {
    int instance, ref;   // point_env: -1 the general instance, 0..3 the per-task instance of that task; the reference's
                         // solver settings compiled in (panda_env: 0, 0)
    int lps, forces, general, shadows, rec;   // panda_env: lanes per sample, FORCES = pick / place, GENERAL = random sampler
                                              // or simple mode, quirk Q8's shadow slots, k_panda_reach_cost behind it
                                              // (point_env: all 0)
    int lanes, blocks;   // active lanes per wavefront, rollout workgroups
    int rows;            // rows of minima the launch leaves in a.wave_min (wave_min.hpp; 0: none)
    int weighted;        // point_env: the build of the general instance that takes the cost weights (POINT_WEIGHTED, POINT_SCENE;
                         // instance == -1)
    int form;            // point_env: 0 one wavefront per 64 samples, 1 dynamics + companion wavefront (rollout_point_kernel.hpp:
                         // rollout_point_body2); m3_rollout only -- the batched and episode paths plan with form_request 0
    int scene;           // point_env: the run-time-scene build of the general instance (POINT_SCENE; instance == -1,
                         // weighted == 1, ref == 0, form == 0); 2: its per-sample twin (m3_set_point_rollout_scenes) -- no
                         // variant of its own; in a batch created with the per-sample section, the table's fourth section
    int priors;          // point_env: the prior build of that instance (m3_set_prior_samples, rollout_point_priors.hip; scene 1 or 2,
                         // instance == -1, weighted == 1, ref == 0, form == 0); in a batch created with the priors section, the
                         // table's fifth section -- every other batch and episode set refuses such a handle
};
inline PointVariant point_variant(const RolloutPlan& p) { return p.scene ? POINT_SCENE : p.weighted ? POINT_WEIGHTED : POINT_PLAIN; }
// the section of the point_env batch table a plan's entry lies in: its variant's, the per-sample handles behind them
// (in a batch created with the priors section, the handles with prior samples behind those: the fifth section)
constexpr int POINT_SECTIONS = POINT_VARIANTS + 2, POINT_SECTION_SV = POINT_VARIANTS, POINT_SECTION_PR = POINT_VARIANTS + 1;
inline int point_section(const RolloutPlan& p) {
    return p.priors ? POINT_SECTION_PR : p.scene == 2 ? POINT_SECTION_SV : (int)point_variant(p);
}
// form_request: m3_set_point_rollout_form's value (0 one wavefront, 1 two wherever available, -1 by rollout_companion_pays)
// per_sample: the handle carries one arena per sample (variant POINT_SCENE then): RolloutPlan::scene = 2
// priors: the handle has prior samples set (variant POINT_SCENE then): RolloutPlan::priors = 1
RolloutPlan plan_rollout_point(const RolloutArgs& a, const PointScene& sc, PointVariant variant, int form_request = 0,
                               bool per_sample = false, bool priors = false);
// one launch of the plan's instance for n handles of K_local = a.Kl and the same plan (tab: device, n entries of the type of
// the plan's variant; p.scene == 2: of BatchRolloutEntrySV)
void launch_rollout_point_batch(const void* tab, int n, const RolloutPlan& p, hipStream_t s);
void launch_rollout_point_nav_batch(const BatchRolloutEntry* tab, int blocks, int n, bool ref, hipStream_t s);
void launch_rollout_point_push_batch(const BatchRolloutEntry* tab, int blocks, int n, bool ref, hipStream_t s);
void launch_rollout_point_pull_batch(const BatchRolloutEntry* tab, int blocks, int n, bool ref, hipStream_t s);
void launch_rollout_point_pushpull_batch(const BatchRolloutEntry* tab, int blocks, int n, bool ref, hipStream_t s);

// ---- launchers (defined in the .hip files) ---------------------------------------------
// one handle's launch of the plan; the plan's variant says which of sc / rt and whether wt is read
// scene_rows: p.scene == 2 only -- the handle's table of per-sample arenas (point_scene_rows.hpp), rt then its uniform members
void launch_rollout_point(const RolloutArgs& a, const PointScene& sc, const PointSceneRT& rt, const PointCostWeights& wt,
                          const RolloutPlan& p, hipStream_t s, int* err = nullptr /* p.form == 1: the hand-over's error word */,
                          const float* scene_rows = nullptr, const int* prior_slot = nullptr /* p.priors only: the handle's */,
                          const float* prior_tab = nullptr /* slot map and table of prior samples */);
// ... of a planner handle with prior samples (rollout_point_priors.hip; rows: null or the handle's per-sample arenas)
void launch_rollout_point_pr(const RolloutArgs& a, const PointSceneRT& uni, const float* rows, const PointCostWeights& wt,
                             const int* prior_slot, const float* prior_tab, int blocks, hipStream_t s);
// the ancillary controllers of a handle with a prior controller (m3_set_prior_controller; prior_controllers.hip): fills rows
// 0 .. c.pc.n - 1 of c.tab from the world, goal, u_max and T of a, the arguments of the rollout launched behind it
struct PriorControllerArgs {
    m3_prior_controller pc;
    float dt;      // the handle's
    float* tab;    // the handle's table of prior samples, device [M3_MAX_PRIOR_SAMPLES][T][2]
};
void launch_prior_controllers(const RolloutArgs& a, const PriorControllerArgs& c, hipStream_t s);
// a point_env handle with prior samples (m3_set_prior_samples, m3_set_prior_controller), in a batch created with the priors
// section: what BatchRolloutEntrySV holds (rows: null or the handle's per-sample table), the handle's OWN slot map and table of
// priors (ctl.tab, [M3_MAX_PRIOR_SAMPLES][T][2]) and its controller (ctl.pc.kind 0: the table is the caller's); the batch stores
// no priors
struct BatchRolloutEntryPR {
    RolloutArgs a;
    PointSceneRT sc;
    PointCostWeights wt;
    const float* rows;
    const int* prior_slot;
    PriorControllerArgs ctl;
};
static_assert(sizeof(BatchRolloutEntryPR) == 872 && offsetof(BatchRolloutEntryPR, sc) == 528 && offsetof(BatchRolloutEntryPR, wt) == 724 &&
              offsetof(BatchRolloutEntryPR, rows) == 760 && offsetof(BatchRolloutEntryPR, prior_slot) == 768 &&
              offsetof(BatchRolloutEntryPR, ctl) == 776 && alignof(BatchRolloutEntryPR) <= 16, "");
// ... of a group of n such handles of the same K, T and lanes (rollout_point_priors_batch.hip; tab: device; blocks: workgroups
// of one handle)
void launch_rollout_point_pr_batch(const BatchRolloutEntryPR* tab, int blocks, int n, hipStream_t s);
// the controllers of the n entries of a batch's priors section, one launch ahead of its rollout launches (an entry without a
// controller: nothing)
void launch_prior_controllers_batch(const BatchRolloutEntryPR* tab, int n, hipStream_t s);
// ... of a planner handle with an arena per sample (rollout_point_rollout_scenes.hip; uni, rows: point_scene_rows.hpp)
void launch_rollout_point_sv(const RolloutArgs& a, const PointSceneRT& uni, const float* rows, const PointCostWeights& wt,
                             int blocks, hipStream_t s);
// ... of a group of n such handles of the same K, T and lanes (tab: device; blocks: workgroups of one handle)
void launch_rollout_point_sv_batch(const BatchRolloutEntrySV* tab, int blocks, int n, hipStream_t s);
// the two-wavefront form of the navigation / push instances (p.form == 1)
void launch_rollout_point_nav2(const RolloutArgs& a, const PointScene& sc, int blocks, int* err, hipStream_t s);
void launch_rollout_point_push2(const RolloutArgs& a, const PointScene& sc, int blocks, int* err, hipStream_t s);
void launch_rollout_point_nav(const RolloutArgs& a, const PointScene& sc, int blocks, hipStream_t s);
void launch_rollout_point_push(const RolloutArgs& a, const PointScene& sc, int blocks, hipStream_t s);
void launch_rollout_point_pull(const RolloutArgs& a, const PointScene& sc, int blocks, hipStream_t s);
void launch_rollout_point_pushpull(const RolloutArgs& a, const PointScene& sc, int blocks, hipStream_t s);
void launch_transpose_noise(const float* src_ktn, float* dst_tkn, int K, int T, int nu,
                            hipStream_t s);
void launch_spline_noise(const float* knots, float* noise, int Kl, int nu, int n_knots, int T, int degree,
                         double smoothing, hipStream_t s);
void launch_sample_noise(const RolloutArgs& a, float* out, hipStream_t s);
void launch_halton_knots(float* knots, int k0, int n, int ncol, const int* primes_dev, const int* perm_dev,
                         const int* perm_off_dev, hipStream_t s);
struct OrderScene {   // where the scene's objects are when the wavefront order is computed
    const float* sim_root;  // != null: box / dyn-obs positions are read from the bound root_state tensor
    int sim_box, sim_dyn;
    float bx, by, dx, dy;   // otherwise these (host world)
    float ox, oy;           // obstacle
};
size_t wave_order_temp_bytes(int n);   // the radix sort's own storage for one range of n keys
hipError_t launch_wave_order(const float* noise, int Kl, int T, int nu, float s0, float s1, int half_local,
                             const OrderScene& os, void* scratch, size_t temp_bytes, int* order, float* noise_sorted,
                             const int* specials /* null, or 3 local indices (-1: none) */, hipStream_t s);
void launch_gather_rows(const float* src, const int* order, float* dst, int Kl, int rows, hipStream_t s);
void launch_weights(const UpdateArgs& a, hipStream_t s);
void launch_wsum(const UpdateArgs& a, hipStream_t s);
void launch_update_small(const UpdateArgs& a, hipStream_t s);   // (whether it applies: update_plan.hpp, update_small_applies)
void launch_finalize(const UpdateArgs& a, hipStream_t s);
void launch_mix(const UpdateArgs& a, hipStream_t s);
void launch_cov_update(const float* actions, const float* w, const float* mean, float* part, float* cov, int K, int T,
                       int nu, hipStream_t s);
void launch_local_topk(const UpdateArgs& a, hipStream_t s);
void launch_regen_fast(const UpdateArgs& a, hipStream_t s);
void launch_p3_search(const UpdateArgs& a, hipStream_t s);          // mixed-table search (+ top-k merge) of shard_mix = 3
void launch_p3_local_weights(const UpdateArgs& a, hipStream_t s);   // k_apply_weights<true> over the local costs
void launch_p3_done(const UpdateArgs& a, hipStream_t s);            // after the second exchange: sums, best rows, plan
int init_ladder_table();   // update.hip: the beta ladder into constant memory (per device context)
int regen_chunks(int Kg);   // workgroups per time step of k_regen_part
int rollout_lanes_for(int Kl);
// MI355X: 256 CUs x 4 SIMDs.  A rollout launch with more wavefronts than that is throughput-bound: the point_env
// kernels then run in their two-waves-per-SIMD build (rollout_point_kernel.hpp)
constexpr int M3_CUS = 256;
constexpr int M3_SIMDS = 1024;
inline bool rollout_two_waves(int wavefronts) { return wavefronts > M3_SIMDS; }
inline bool rollout_three_waves(int wavefronts) { return wavefronts > 4 * M3_SIMDS; }   // (measured: equal at 4 per SIMD, -11 % at 8)
// The two-wavefront form (dynamics + companion, rollout_point_kernel.hpp) puts two wavefronts of > 256 VGPRs on two SIMDs of
// one CU: up to M3_SIMDS / 2 workgroups every wavefront still has a SIMD of its own.  The automatic rule takes the form up to
// ROLLOUT_COMPANION_MAX_BLOCKS workgroups: the largest count at which it was not slower than the one-wavefront form in the
// K sweep of profiles/companion_wave/k_sweep_push.json ("Companion wavefront").
constexpr int ROLLOUT_COMPANION_MAX_BLOCKS = M3_SIMDS / 2;
inline bool rollout_companion_pays(int blocks) { return blocks <= ROLLOUT_COMPANION_MAX_BLOCKS; }
// its LDS: 16 bytes of progress words, then per step [8][64] floats (six of the record, the two scaled controls)
constexpr int R2_COMPS = 8;
constexpr size_t R2_LDS_MAX = 64 * 1024;   // what a launch gets without a function attribute
inline size_t rollout_point2_lds_bytes(int T) { return 16 + (size_t)T * R2_COMPS * 64 * sizeof(float); }
inline bool rollout_point2_fits(int T) { return T >= 1 && rollout_point2_lds_bytes(T) <= R2_LDS_MAX; }
int mins_workgroups(int Kg);
int topk_workgroups(int Kg);
int ladder_workgroups(int Kg);
int wsum_chunks(int Kl);
int apply_workgroups(int Kg);
void launch_mins(const UpdateArgs& a, hipStream_t s);
void launch_ladder(const UpdateArgs& a, hipStream_t s);
void launch_ladder_search(const UpdateArgs& a, hipStream_t s);
void launch_fused_large(const UpdateArgs& a, hipStream_t s);

// p2p.hip: device-side exchange of the records over peer-mapped memory
struct P2PArgs {
    const float* rec;                      // this rank's record
    int rec_len, rec_stride, n_ranks, rank, slot, seq;   // rec_stride: floats between two slots of a block (rec_len rounded up to 4)
    int plain_memory;                      // the block is ordinary (cached) device memory: system-scope fences needed
    unsigned long long timeout_ticks;      // of the 100 MHz wall clock
    int* err;                              // device word in the own block: 0, or 1 + the rank that never arrived
    float* peer_data[MIX_MAX_RANKS];       // data part of every rank's exchange block: [2][n_ranks][rec_stride]
    int* peer_flags[MIX_MAX_RANKS];        // flag part: [2][MIX_MAX_RANKS]
};
constexpr size_t P2P_HDR_BYTES = 1024;    // flags [2][32] ints + error word, then the data part
void launch_p2p_put(const P2PArgs& a, hipStream_t s);
void launch_p2p_wait(const P2PArgs& a, hipStream_t s);
void launch_p2p_exchange(const P2PArgs& a, hipStream_t s);   // both in one launch

// step mode
struct SimViews {
    float* dof_state;          // [Kl][2*ndof]
    float* root_state;         // [Kl][nA][13]
    float* rigid_body_state;   // [Kl][nB][13]
    float* net_contact_force;  // [Kl][nB][3]
    int n_actors, n_bodies;
    int box_actor, dyn_actor, robot_actor;  // panda_env: box = cubeA, dyn = cubeB
    int box_body, dyn_body, robot_body;     // point: robot_body = link_y (last body);
                                            // panda: robot_body = panda_link0 (first of 11)
    int table_body, shelf_body;             // panda_env only
    int obs_actor, obs_body;                // panda_env only: the dyn-obs plate
};
void launch_sim_pull(const SimViews& v, float* world /*[NW][Kl]*/, int Kl, hipStream_t s);
void launch_sim_shift_pull(const SimViews& v, float* world, int Kl, int actor, float dx, float dy, float dz, hipStream_t s);
void launch_sim_push(const SimViews& v, const float* world, int Kl, hipStream_t s);
void launch_sim_step(const PointScene& sc, const SimViews& v, float* world, const float* u /*[Kl][2]*/, float* u_keep,
                     int Kl, hipStream_t s);   // step + refresh of the views
void launch_sim_step_s(const PointSceneRT& sc, const SimViews& v, float* world, const float* u, float* u_keep, int Kl,
                       hipStream_t s);   // ... of a handle with a run-time scene
// ... of a sim_only handle with an arena per environment (m3_set_point_scene_rows; point_scene_rows.hpp: uni, rows)
void launch_sim_step_sv(const PointSceneRT& uni, const float* rows, const SimViews& v, float* world, const float* u,
                        float* u_keep, int Kl, hipStream_t s);
void launch_sim_forces(const SimViews& v, float* world, const float* f /*[Kl][nB][3]*/, int Kl,
                       hipStream_t s);
// wt: the handle's cost weights, or null for the reference's (compiled in)
void launch_sim_cost(const CostParams& cp, const PointCostWeights* wt, float* world, int Kl, int k0, float* cost, hipStream_t s);
void launch_sim_suction(const SimViews& v, float* world, int Kl, float kp, float thresh, float reach,
                        const float* action, int apply, float* forces, int* flags, const int* gate, hipStream_t s);

// batched closed-loop episodes (m3_episodes_*): one lane per episode of an N-env point_env world
struct EpisodeLane {          // per episode, uploaded once by m3_episodes_create
    int task, phase, suction; // M3_TASK_*, dyn-obs phase, EP_SUCTION_* (episode_lane.hpp)
    float gx, gy, kp;         // goal, kp_suction
    const int* pref;          // its planner's m3_info.pull_preference (device)
    const float* plan;        // its planner's action-out (device): row 0 is the velocity target
};
struct EpisodeArgs {
    SimViews v;               // the world's views, [n] rows
    float* world;             // the world's SoA state [NW][n]
    int n, last_tick;         // episodes, max_ticks - 1
    const EpisodeLane* lane;  // [n]
    m3_episode_status* st;    // [n]
    int* gate;                // [n] suction gate of the current tick
    float* trace;             // [max_ticks][n][10] or null
};
void launch_episodes_pre(const EpisodeArgs& a, int tick, hipStream_t s);
void launch_episodes_post(const PointScene& sc, const EpisodeArgs& a, int tick, hipStream_t s);
void launch_episodes_post_s(const PointSceneRT& sc, const EpisodeArgs& a, int tick, hipStream_t s);
void launch_episodes_post_sv(const PointSceneRT& uni, const float* rows, const EpisodeArgs& a, int tick, hipStream_t s);

constexpr int NW = 28;  // floats per env in the step-mode SoA world (PointWorld fields)
constexpr int NWP = 77; // same for the panda_env (PandaWorld fields, rollout_panda.hip)

// panda_env
constexpr int REACH_REC = 17;   // floats the reach cost reads of a (step, sample): rollout_panda.hip
struct PandaArgs {
    float world0[57];  // q9 qd9 | cubeA13 | cubeB13 | dyn-obs13 (pos3 quat4 vel3 angvel3)
    int cubeA_actor, cubeB_actor, obs_actor;
    PandaCostParams cp;
    int shadows;       // the last (two) sample slot(s) of every wavefront re-simulate sample 0 (and K / 2): quirk Q8
    int lps;           // lanes per sample of the rollout kernel: 0 = by size, 1, 8, 16 (m3_set_panda_lanes_per_sample)
    float* reach_rec;            // [T][REACH_REC][Kl] or null: the reach cost is formed after the rollout (k_panda_reach_cost), no shadow slots
    int* busy_hint;              // device address of the handle's hint word (host memory, mapped): 1 + the share, in 1/1000, of the
                                 // launch's (sample, substep) pairs with the gripper within reach of a box; written by the last wavefront
    unsigned long long* busy_count;   // device scratch of that: bits 0-23 wavefronts finished, bits 24-63 the sum so far
    int reach_busy;              // the host's reading of the last reports, with hysteresis: the reach command runs with 8 lanes per sample
};
// the plan of a panda rollout launch; pa becomes what the kernels receive (rows: the reach-cost kernel's workgroups with it)
RolloutPlan plan_rollout_panda(const RolloutArgs& a, PandaArgs& pa);
struct BatchPandaEntry {     // one panda_env handle's rollout in m3_batch_command's table (a.lanes: the plan's)
    RolloutArgs a;
    PandaArgs pa;
    PandaScene sc;
};
// one panda_env handle's rollout in the second section of m3_batch_command's table (a batch created with
// M3_BATCH_PANDA_RUNTIME; rollout_panda_batch_rt.hip): a handle that needs the run-time scene, the weighted cost or both, or has
// a workspace per sample (rows: the handle's device table [PANDA_SCENE_ROW_WORDS][K_local], else null)
struct BatchPandaEntryRT {
    RolloutArgs a;
    PandaArgs pa;
    PandaSceneRT sc;
    PandaCostWeights wt;
    const float* rows;
};
// What a launch is for: the family (panda_variant.hpp) and everything any family reads of the handle -- each takes what it
// needs: lit the literal kernels; rt every other family (with rows: its uniform members, panda_scene_rows.hpp); wt the weighted
// and the rows kernels; rows (per sample of a rollout, per environment of a step, the views or a cost) the rows kernels.
struct PandaLaunchScene {
    PandaVariant variant;
    const PandaScene* lit;
    const PandaSceneRT* rt;
    const PandaCostWeights* wt;
    const float* rows;
    // PANDA_PRIORS (m3_set_panda_prior_samples): the handle's slot map [Kl] and table of prior samples [rows][T][9]; its `rows`
    // are null unless the handle has a workspace per sample as well
    const int* prior_slot = nullptr;
    const float* prior_tab = nullptr;
};
// One launcher per operation (rollout_panda.hip; each forwards to the translation unit that holds the family's kernels).
// The rollout: pa, p as plan_rollout_panda left them -- the form is chosen alike for every family -- + the family's reach-cost
// kernel when the plan keeps the record buffer.
void launch_rollout_panda(const RolloutArgs& a, const PandaArgs& pa, const PandaLaunchScene& sc, const RolloutPlan& p, hipStream_t s);
// one launch of the plan's instance for n handles of K_local = Kl and the same plan and variant (a batch-side one; tab: device,
// n entries -- BatchPandaEntry for PANDA_LITERAL, else BatchPandaEntryRT), + one launch of the reach-cost kernel when the plan
// keeps the record buffer
void launch_rollout_panda_batch(const void* tab, int n, PandaVariant variant, const RolloutPlan& p, int Kl, hipStream_t s);
// step mode: step + refresh of the views, the views alone (no weighted form: they read no cost), the cost
void launch_psim_step(const PandaLaunchScene& sc, const SimViews& v, float* world, const float* u, float* u_keep, int Kl,
                      hipStream_t s);
void launch_psim_pull(const PandaLaunchScene& sc, const SimViews& v, float* world, int Kl, hipStream_t s);
void launch_psim_push(const PandaLaunchScene& sc, const SimViews& v, const float* world, int Kl, hipStream_t s);
void launch_psim_cost(const PandaLaunchScene& sc, const PandaCostParams& cp, const float* world, int Kl, int k0, bool env0_cube,
                      float* cost, hipStream_t s);

// batched closed-loop episodes of the panda_env (m3_panda_episodes_*): one lane per episode of an N-env world
struct PandaEpisodeArgs {
    SimViews v;                    // the world's views, [n] rows
    SimViews pv;                   // the set's planning view, [n] rows (no contact forces): what the planners and the host read
    float* world;                  // the world's SoA state [NWP][n]
    int n, last_tick, settle_ticks;
    const float* const* plan;      // [n] each planner's action-out (device): row 0 is the velocity target
    const float* kept;             // [n][9] the targets each planner's own simulator kept since tick 0
    const int* ended;              // [n] the host's word for the current tick
    m3_panda_episode_status* st;   // [n]
    float* trace;                  // [max_ticks][n][PE_TRACE_FLOATS] or null
};
// What a tick's two launches are for: the family (panda_variant.hpp: panda_episodes_variant -- PANDA_LITERAL, or PANDA_ROWS for a
// set created with M3_PANDA_EPISODES_RUNTIME) and what either reads: lit the literal kernels (the world's scene); the rows kernels
// uni (the members of the world's pscene_rt that depend on dt / substeps / iters alone) and the set's two device tables
// [PANDA_SCENE_ROW_WORDS][n] -- plan_rows the pre kernel (row e: planner e's workspace), world_rows the post kernel (row e: the
// workspace of row e of the world).
struct PandaEpisodesLaunchScene {
    PandaVariant variant;
    const PandaScene* lit;
    const PandaSceneRT* uni;
    const float* plan_rows;
    const float* world_rows;
};
void launch_panda_episodes_pre(const PandaEpisodesLaunchScene& sc, const PandaEpisodeArgs& a, hipStream_t s);
void launch_panda_episodes_post(const PandaEpisodesLaunchScene& sc, const PandaEpisodeArgs& a, int tick, hipStream_t s);

}  // namespace m3

namespace m3 {
// One scene per row of a handle (m3_handle::point_rows, ::panda_rows): per environment of a sim_only handle or per sample of a
// planner's fused rollout.  The three pointers are non-owning views of ledger blocks.
template <class Scene> struct SceneRows {
    bool env_on = false;      // sim_only: the step, the views, m3_cost and the episode tick take the per-row kernels
    bool sample_on = false;   // planner: m3_rollout / m3_command take the per-sample kernels
    Scene* set = nullptr;     // host [Kl]: what was set (m3_get_*_scene_row / m3_get_*_rollout_scene)
    float* host = nullptr;    // pinned host [row words][Kl]: the table as uploaded
    float* dev = nullptr;     // device, the same
};

// The prior samples of a planner handle (m3_set_prior_samples): samples whose controls are the caller's sequences.  The
// pointers are non-owning views of ledger blocks, allocated as one group by the first setter call on the handle.
struct PriorSampleState {
    int n = 0;                    // priors set (0: none -- the handle launches what it launched before the call existed)
    bool host_values = false;     // set by m3_set_prior_samples: `pinned` holds the values (m3_get_prior_sample)
    int idx[M3_MAX_PRIOR_SAMPLES] = {};   // global sample index of prior j ...
    int dev_n = 0;                // ... of the dev_n priors the device slot map was last built from (>= n: kept over a clear)
    float* tab_dev = nullptr;     // device [M3_MAX_PRIOR_SAMPLES][T][nu]
    int* slot_dev = nullptr;      // device [Kl]: local sample -> row of the table, -1: no prior
    float* pinned = nullptr;      // pinned host mirror of both: the table, behind it the slot map
    hipEvent_t uploaded = nullptr;   // recorded behind the last upload from `pinned`
    bool upload_pending = false;
    int used = -1;                // m3_prior_samples_used
    m3_prior_controller ctl = {}; // m3_set_prior_controller (kind 0: none -- the table is the caller's): the rows 0 .. n - 1 of
                                  // tab_dev are written by k_prior_controllers ahead of every rollout
};

// The sample groups of a planner handle (m3_set_sample_groups, sample_groups.hpp): the pointers are non-owning views of ledger
// blocks, allocated as one group by the first setter call on the handle and sized for any partition of its K samples.
struct SampleGroupState {
    int n = 0;                    // groups set (0: none -- the handle launches what it launched before the call existed)
    int n_ungrouped = 0;
    float worst_frac = 1.0f;
    int* tab_dev = nullptr;       // device: member[K/2][16] | worst_j[K/2] | ungrouped[K] (sample_group_table_ints)
    float* raw_dev = nullptr;     // device [K]: the per-model costs of the last rollout (m3_sample_group_raw_costs)
    int* pinned = nullptr;        // pinned host: the table as uploaded, behind it label[K] (the caller's ids) and dense[K] (rows)
};
// what k_sample_groups receives (sample_groups.hip): cap_groups = K/2 rows of the table, n_groups of them in use
struct SampleGroupArgs {
    const int* tab;
    int n_groups, n_ungrouped, cap_groups, K;
    float* J;      // M3_BUF_TRAJ_COST
    float* raw;
};
void launch_sample_groups(const SampleGroupArgs& a, hipStream_t s);
}  // namespace m3

// the ledger's release function bound to HIP (m3_api.hip): the one place that frees
void m3_release_block(m3::BlockKind kind, void* p);

struct m3_handle {
    m3_config cfg;
    // OWNERSHIP: every block of the handle is an entry of this ledger (owned_blocks.hpp), adopted by one own_* helper call of
    // m3_api.hip and freed by m3_destroy's release_all().  The named pointers below (buf[], sim_world, order, xb, point_rows.dev,
    // ...) are non-owning views the kernels' argument blocks and the getters read; a new buffer is one helper call, nothing else.
    m3::OwnedBlocks mem{&m3_release_block, 128};
    int* order = nullptr;          // [Kl] lane slot -> local sample (null: identity), sampler.hip
    void* order_scratch = nullptr;
    float* noise_sorted = nullptr; // [T][Kl][nu] noise rows in wavefront order
    size_t order_temp_bytes = 0;
    bool wave_order = true;        // m3_set_wave_order
    bool order_valid = false;
    bool order_dirty = true;       // recomputed by the next m3_rollout (needs the world)
    unsigned last_noise_call = 0;  // h->calls at the last m3_set_noise*
    int noise_churn = 0;           // consecutive noise uploads fewer than 16 commands apart
    bool relabel_pending = false;  // m3_relabel_samples: done by the next m3_rollout
    bool relabelled = false;       // the noise rows ARE in wavefront order (identity order from then on)
    m3::PointScene scene;
    m3::PandaScene pscene;             // ... with the masses of panda_scene (make_panda_scene; m3_create, m3_set_panda_scene)
    // m3_set_panda_scene (extension, panda_env): fixed members, written in place -- no allocation; survive m3_reset
    m3_panda_scene panda_scene = m3::PANDA_SCENE_DEFAULT;
    m3::PandaSceneRT pscene_rt = {};   // make_panda_scene_rt (m3_create, m3_set_panda_scene)
    int panda_scene_instance = -1;     // m3_set_panda_scene_instance: -1 by the values (geometry / friction not the defaults), 0 / 1 forced
    int panda_scene_used = 0;          // what the last rollout or step launched (m3_panda_scene_instance_used)
    float pworld0[57];
    hipStream_t stream = nullptr;
    std::string err;
    // objective
    int task = M3_TASK_PUSH;
    float goal[7] = {0, 0, 0, 0, 0, 0, 1};
    int gripper_cmd = 0;
    int avoid_dyn_obs = 0;             // m3_set_avoid_dyn_obs (extension; 0 = the reference's compute_cost)
    m3::PointCostWeights cost_weights = m3::POINT_COST_WEIGHTS_DEFAULT;   // m3_set_point_cost_weights (extension, point_env)
    int weighted_instance = -1;        // m3_set_weighted_cost_instance: -1 by the weights (not the defaults bit for bit), 0 / 1 forced
    // m3_set_panda_cost_weights (extension, panda_env): a fixed member, written in place -- no allocation; survives m3_reset
    m3::PandaCostWeights panda_cost_weights = m3::PANDA_COST_WEIGHTS_DEFAULT;
    int panda_weighted_instance = -1;  // m3_set_panda_weighted_cost_instance: -1 by the weights (not the defaults bit for bit), 0 / 1 forced
    int panda_weighted_used = 0;       // what the last rollout or m3_cost launched (m3_panda_weighted_cost_instance_used)
    m3_point_scene point_scene = m3::POINT_SCENE_DEFAULT;   // m3_set_point_scene (extension, point_env); survives m3_reset
    m3::PointSceneRT scene_rt = {};    // ... with the handle's dt / substeps / iterations (make_point_scene_rt; m3_create, m3_set_point_scene)
    int scene_instance = -1;           // m3_set_point_scene_instance: -1 by the values (not the defaults bit for bit), 0 / 1 forced
    // The rows of a handle, per kind of scene (SceneRows above): m3_set_*_scene_rows on a sim_only handle (one scene per
    // environment), m3_set_*_rollout_scenes on a planner handle (one per sample of the fused rollout); survive m3_reset.  A handle
    // is a planner or sim_only for life, so both features keep their rows in the same three blocks, allocated as one group by
    // the first setter call of that kind on the handle (upload_scene_rows, m3_api.hip); nothing else allocates them.
    m3::SceneRows<m3_point_scene> point_rows;   // table [POINT_SCENE_ROW_WORDS][Kl] (point_scene_rows.hpp)
    m3::SceneRows<m3_panda_scene> panda_rows;   // table [PANDA_SCENE_ROW_WORDS][Kl] (panda_scene_rows.hpp)
    m3::PriorSampleState priors;                // m3_set_prior_samples; survives m3_reset
    m3::PriorSampleState panda_priors;          // m3_set_panda_prior_samples (nu = 9; no controller); survives m3_reset
    m3::SampleGroupState groups;                // m3_set_sample_groups; survives m3_reset
    // world
    float world0[18];
    const float* world0_bound = nullptr;  // device, 18 floats (filled by world_from_sim)
    const float* bind_dof = nullptr;
    const float* bind_root = nullptr;
    int bind_nact = 0, bind_box = 0, bind_dyn = 0, bind_obs = 0;
    bool have_noise = false;
    bool cov_active = false;       // cfg.update_cov on a single-mode halton-spline planner (mppi.py:508-516)
    float* noise_mats = nullptr;   // device [2][nu][nu]: chol(noise_sigma) | noise_sigma^-1 (cfg.full_sigma)
    m3::UpdateProtocol protocol = m3::UPDATE_UNSHARDED;   // how the ranks reach one plan (update_plan.hpp; m3_create, from cfg alone)
    const float* recb_src = nullptr;   // second records as exchanged by m3_p2p_exchange(h, 1) (else M3_BUF_RECORDS_B_ALL)
    int recb_stride = 0;
    float* noise_all = nullptr;    // update_noise_of_all_ranks: [n_ranks][T][Kl][nu]; buf[M3_BUF_NOISE] aliases this rank's block
    int* local_top_idx = nullptr;  // ... and top_idx of the local pre-gather selection (scratch)
    unsigned calls = 0;
    int lanes_override = 0;  // 0 = automatic (rollout_lanes_for)
    int point_form = -1;          // m3_set_point_rollout_form: 0, 1, -1 = automatic
    int point_form_used = -1;     // the form of the last rollout launch (m3_point_rollout_form_used)
    int* rollout_err = nullptr;   // mapped host word (m3_create, point_env): a hand-over wait of the two-wavefront form ran out
    int* rollout_err_dev = nullptr;
    int* panda_busy_hint = nullptr;   // hipHostMalloc (m3_create, panda_env): see PandaArgs::busy_hint
    int* panda_busy_hint_dev = nullptr;   // the same word as the device sees it
    unsigned long long* panda_busy_count = nullptr;
    float* panda_reach_rec = nullptr;     // PandaArgs::reach_rec (m3_create: unsharded panda handles with K <= PANDA_REACH_REC_MAX_K)
    bool panda_reach_deferred = true;     // m3_set_panda_reach_cost_kernel
    int panda_reach_busy = 0;
    int panda_lps_used = 0;           // the form of the last panda rollout (m3_panda_lanes_per_sample_used)
    int panda_lps = 0;       // 0 = automatic (rollout_panda.hip: panda_lps_for), 1, 16
    // device buffers (views; the record protocols: three of buf[] alias other blocks and are no ledger entries)
    void* buf[M3_BUF_COUNT] = {};
    long long nbytes[M3_BUF_COUNT] = {};
    float* world0_dev = nullptr;
    float* action_out = nullptr;  // caller-owned destination of the plan (m3_set_action_out)
    m3::VI* topk_cand = nullptr;
    float* part_min = nullptr;
    float* lad = nullptr;
    float* wpart = nullptr;
    float* apart = nullptr;  // + 16 floats of SearchOut at the front
    int* wcount = nullptr;
    // the three-launch form of the unsharded multi-modal update (update_plan.hpp: update_large_range; update.hip: k_ladder_search)
    float* wave_min = nullptr;     // [rollout workgroups][3] minima left by the rollout (wave_min.hpp)
    int wave_min_rows = 0;         // rows the last rollout wrote
    int* lflag = nullptr;
    int lad_epoch = 0;
    bool five_launches = false;    // m3_set_update_launches(h, 5)
    int ladder_spins = 1 << 18;    // bounded wait of the in-launch ladder exchange (~20 ms); m3_set_ladder_spins
    float* sim_world = nullptr;  // step mode SoA [NW][Kl]
    float* sim_u = nullptr;      // [Kl][nu]
    float* noise_stage = nullptr;
    m3::SimViews views{};
    bool views_bound = false;
    // device-side exchange (p2p.hip)
    void* xb = nullptr;                 // view, own exchange block: header (flags, error word) + [2][n_ranks][rec_len]
    size_t xb_bytes = 0;
    int xb_kind = 0;                    // 1 uncached, 2 fine-grained, 3 plain device memory
    int xb_first_kind = 1;              // where the allocation's fallback chain starts (m3_p2p_set_memory_kind)
    void* peer_base[m3::MIX_MAX_RANKS] = {};   // every rank's block as mapped here (own: xb)
    bool peer_ipc[m3::MIX_MAX_RANKS] = {};     // opened with hipIpcOpenMemHandle: a ledger entry (m3_p2p_connect does not open it twice)
    bool p2p_ready = false;
    int p2p_seq[2] = {0, 0};           // per channel (0: records, 1: second records of shard_mix = 3)
    int p2p_first_ms = 30000, p2p_ms = 500;   // wait time-outs (m3_p2p_set_timeout_ms)
    int records_stride = 0;             // floats between two records of records_src
    const float* records_src = nullptr; // != null: the records of the exchange just enqueued (consumed by m3_finalize)
    // timing
    bool timing = false;
    hipEvent_t ev[4] = {};
};
