// m3_api.hip -- C-ABI of libm3p2i_hip.so (see include/m3p2i_hip.h for what each entry
// point replaces in the reference).  Host code only: argument checking, buffer ownership,
// launch sequencing on the handle's HIP stream.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <tuple>
#include <vector>
#include <new>

#include "m3_internal.hpp"
#include "batch_table_layout.hpp"
#include "point_views.hpp"
#include "panda_episode_lane.hpp"
#include "panda_episode_tables.hpp"
#include "point_scene_rows.hpp"
#include "panda_scene_rows.hpp"
#include "sample_groups.hpp"

using namespace m3;

static thread_local std::string g_create_err;

// on a HIP error: "<expr>: <error>" into (o)->err -- the error string of a handle, a batch (m3_batch) or an episode set
// (m3_episodes) -- and return M3_ERR_HIP
#define HIPCHK(o, expr)                                                                  \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            (o)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                \
            return M3_ERR_HIP;                                                           \
        }                                                                                \
    } while (0)

static int fail(m3_handle* h, int code, const char* msg) {
    if (h) h->err = msg; else g_create_err = msg;
    return code;
}

// what the update plans of a handle are decided from (update_plan.hpp)
static UpdatePlanInput update_plan_input(const m3_handle* h, bool fused, bool rollout_minima) {
    const m3_config& c = h->cfg;
    return {h->protocol, c.K_local, c.K_global, c.T, c.nu, c.multi_modal != 0, c.mode_simple != 0, fused, h->five_launches, rollout_minima};
}

// ---- ownership (owned_blocks.hpp): the ledger's release function bound to HIP -- the one place that frees -- and one helper
// per kind, the only places that allocate: allocate, adopt into the object's ledger, write the object's view ----
void m3_release_block(BlockKind kind, void* p) {
    switch (kind) {
        case BLOCK_DEVICE: (void)hipFree(p); break;
        case BLOCK_PINNED: (void)hipHostFree(p); break;
        case BLOCK_HOST: std::free(p); break;
        case BLOCK_EVENT: (void)hipEventDestroy(static_cast<hipEvent_t>(p)); break;
        case BLOCK_IPC: (void)hipIpcCloseMemHandle(p); break;
    }
}
extern "C" long long m3_owned_blocks_live(void) { return g_owned_blocks_live.load(); }

// alloc(void**) -> hipError_t; the answer: its error, or out-of-memory if the ledger could not take the block
template <class T, class F> static hipError_t own_hip(OwnedBlocks& l, BlockKind kind, T*& view, F alloc) {
    hipError_t e = hipSuccess;
    const bool ok = own_block(l, kind, view, [&]() -> void* { void* p = nullptr; e = alloc(&p); return e == hipSuccess ? p : nullptr; });
    return ok ? hipSuccess : e != hipSuccess ? e : hipErrorOutOfMemory;
}
// flags 0: hipMalloc; else hipExtMallocWithFlags
template <class T> static hipError_t own_device(OwnedBlocks& l, T*& view, size_t bytes, unsigned flags = 0) {
    return own_hip(l, BLOCK_DEVICE, view, [=](void** p) { return flags ? hipExtMallocWithFlags(p, bytes, flags) : hipMalloc(p, bytes); });
}
template <class T> static hipError_t own_pinned(OwnedBlocks& l, T*& view, size_t bytes, unsigned flags) {
    return own_hip(l, BLOCK_PINNED, view, [=](void** p) { return hipHostMalloc(p, bytes, flags); });
}
template <class T> static hipError_t own_host(OwnedBlocks& l, T*& view, size_t bytes) {
    return own_hip(l, BLOCK_HOST, view, [=](void** p) { return (*p = std::malloc(bytes)) ? hipSuccess : hipErrorOutOfMemory; });
}
// flags 0: hipEventCreate
static hipError_t own_event(OwnedBlocks& l, hipEvent_t& view, unsigned flags = 0) {
    return own_hip(l, BLOCK_EVENT, view, [=](void** p) {
        return flags ? hipEventCreateWithFlags(reinterpret_cast<hipEvent_t*>(p), flags) : hipEventCreate(reinterpret_cast<hipEvent_t*>(p));
    });
}
static hipError_t own_ipc(OwnedBlocks& l, void*& view, const hipIpcMemHandle_t& ih) {
    return own_hip(l, BLOCK_IPC, view, [&](void** p) { return hipIpcOpenMemHandle(p, ih, hipIpcMemLazyEnablePeerAccess); });
}

extern "C" int m3_abi_version(void) { return M3_ABI_VERSION; }

extern "C" const char* m3_last_error(const m3_handle* h) {
    return h ? h->err.c_str() : g_create_err.c_str();
}

extern "C" void m3_default_config(m3_config* c, int env_type) {
    std::memset(c, 0, sizeof(*c));
    c->abi_version = M3_ABI_VERSION;
    c->env_type = env_type;
    c->u_scale = 1.0f;
    c->gamma = 0.95f;         // MPPIConfig.rollout_var_discount, mppi.py:50
    c->step_size_mean = 0.98f;  // mppi.py:178
    c->sample_null_action = 1;
    c->filter_u = 1;
    c->substeps = 2;          // isaacgym_wrapper.py:10
    c->solver_iters = 6;      // isaacgym_wrapper.py:28
    if (env_type == M3_ENV_POINT) {  // config/mppi/point.yaml, config_point.yaml, isaacgym/point.yaml
        c->nu = 2; c->K_global = c->K_local = 200; c->T = 15; c->u_per_command = 15;
        c->lambda_ = 0.5f; c->kp_suction = 400.0f; c->dt = 0.05f;
        for (int j = 0; j < 2; ++j) { c->u_min[j] = -3.0f; c->u_max[j] = 3.0f; c->noise_sigma_diag[j] = 3.0f; }
    } else {  // config/mppi/panda.yaml, config_panda.yaml, isaacgym/panda.yaml
        c->nu = 9; c->K_global = c->K_local = 200; c->T = 12; c->u_per_command = 12;
        c->lambda_ = 0.05f; c->pre_height_diff = 0.05f; c->dt = 0.01f;
        for (int j = 0; j < 9; ++j) {
            c->u_min[j] = j < 7 ? -2.0f : -1.5f; c->u_max[j] = j < 7 ? 2.0f : 1.5f;
            c->noise_sigma_diag[j] = j < 7 ? 10.0f : 0.8f;
        }
    }
}

// "Planar contact dynamics spec v1" constants (sources: config/point_env/*.yaml,
// pointRobot.urdf, isaacgym_wrapper.py:18-37,341-344,462-469)
static void build_point_scene(const m3_config& c, PointScene& s) { make_point_scene(s, c.dt, c.substeps, c.solver_iters); }
// everything else of the scene is compile-time constant in PointScene (planar_dyn.hpp)

// "Panda chain spec" constants (sources: franka_panda.urdf limits, config/panda_env/*.yaml,
// isaacgym_wrapper.py:341-344)
// the handle's two panda scenes from its workspace (m3_create, m3_set_panda_scene): PandaScene takes the masses, PandaSceneRT
// everything
static void build_panda_scenes(const m3_config& c, const m3_panda_scene& ws, PandaScene& s, PandaSceneRT& rt) {
    make_panda_scene(s, c.dt, c.substeps, 6, ws.cube_m, ws.obs_m);
    rt = make_panda_scene_rt(ws, c.dt, c.substeps);
}

static void default_panda_world(float* w, int cube_on_shelf) {
    const float q0[9] = {0, 0, 0, -2.0f, 0, 1.8675f, 0, 0.02f, 0.02f};  // panda.yaml:10
    std::memset(w, 0, 57 * sizeof(float));      // q9 qd9 | cubeA13 | cubeB13 | dyn-obs13
    for (int i = 0; i < 9; ++i) w[i] = q0[i];
    if (cube_on_shelf) { w[18] = 0.425f; w[19] = 0.0f; w[20] = 1.35f; }     // 5_cubeA.yaml
    else { w[18] = 0.2f; w[19] = -0.2f; w[20] = 1.06f; }
    w[24] = 1.0f;
    w[31] = 0.2f; w[32] = 0.2f; w[33] = 1.06f; w[37] = 1.0f;                // 6_cubeB.yaml
    w[44] = 0.35f; w[45] = 0.0f; w[46] = 1.735f; w[50] = 1.0f;              // 4_obs.yaml
}

static void default_world(float* w) {
    const float init[18] = {0, 0, 0, 0, /*box 7_box.yaml*/ 0, 2, 1, 0, 0, 0, 0,
                            /*dyn-obs 6_dyn_obs.yaml*/ -2, 2, 1, 0, 0, 0, 0};
    std::memcpy(w, init, sizeof(init));
}

static int alloc_buf(m3_handle* h, int id, long long bytes) {
    if (bytes < 16) bytes = 16;
    const hipError_t e = own_device(h->mem, h->buf[id], (size_t)bytes);
    if (e != hipSuccess) { h->err = std::string("hipMalloc(&h->buf[id], (size_t)bytes): ") + hipGetErrorString(e); return M3_ERR_HIP; }
    HIPCHK(h, hipMemsetAsync(h->buf[id], 0, (size_t)bytes, h->stream));
    h->nbytes[id] = bytes;
    return M3_OK;
}

static constexpr int PANDA_BUSY_ON = 300, PANDA_BUSY_OFF = 220;
static constexpr int PANDA_REACH_REC_MAX_K = 8192, PANDA_BUSY_ON_REC = 260, PANDA_BUSY_OFF_REC = 190;   // (the forms tie between 116 and ~250 per mille; the arm's initial pose reads 148)

extern "C" int m3_create(const m3_config* c, m3_handle** out) {
    if (!c || !out) return fail(nullptr, M3_ERR_BAD_ARG, "m3_create: null argument");
    if (c->abi_version != M3_ABI_VERSION) return fail(nullptr, M3_ERR_BAD_ARG, "m3_create: abi_version mismatch");
    if (c->K_global < 1 || c->K_local < 1 || c->k_offset < 0 || c->k_offset + c->K_local > c->K_global)
        return fail(nullptr, M3_ERR_SHAPE, "m3_create: bad K_global/K_local/k_offset");
    if (c->T < 1 || c->T > 4096) return fail(nullptr, M3_ERR_SHAPE, "m3_create: bad horizon T");
    if (c->env_type == M3_ENV_POINT && c->nu != 2) return fail(nullptr, M3_ERR_SHAPE, "m3_create: point_env needs nu == 2");
    if (c->env_type == M3_ENV_PANDA && c->nu != 9) return fail(nullptr, M3_ERR_SHAPE, "m3_create: panda_env needs nu == 9");
    if (c->env_type != M3_ENV_POINT && c->env_type != M3_ENV_PANDA) return fail(nullptr, M3_ERR_BAD_ARG, "m3_create: bad env_type");
    if (!c->sim_only) {
        if (c->K_global < M3_TOPK) return fail(nullptr, M3_ERR_SHAPE, "m3_create: K must be >= 20 (torch.topk(weights, 20), mppi.py:248)");
        if (c->filter_u && (c->mode_simple ? c->u_per_command : c->T) < 9)
            return fail(nullptr, M3_ERR_SHAPE, "m3_create: filter_u needs >= 9 rows (savgol window, mppi.py:190)");
        if (c->mode_simple && (c->u_per_command < 1 || c->u_per_command > c->T))
            return fail(nullptr, M3_ERR_SHAPE, "m3_create: bad u_per_command");
    }
    if (c->substeps < 1 || c->solver_iters < 1 || !(c->dt > 0.0f)) return fail(nullptr, M3_ERR_BAD_ARG, "m3_create: bad dt/substeps/solver_iters");
    if (c->shard_mix && c->K_local != c->K_global) {
        if (c->multi_modal && !c->mode_simple && c->sampling_random)
            return fail(nullptr, M3_ERR_UNSUPPORTED, "m3_create: one-collective multi-modal sharding re-generates the other ranks' "
                                                     "actions from the noise TABLE: not with sampling_random");
        if (c->shard_mix >= 2 && !(c->multi_modal && !c->mode_simple))
            return fail(nullptr, M3_ERR_BAD_ARG, "m3_create: shard_mix = 2 / 3 (ladder tables in the records) are multi-modal protocols");
        if (c->shard_mix < 0 || c->shard_mix > 3) return fail(nullptr, M3_ERR_BAD_ARG, "m3_create: shard_mix must be 0, 1, 2 or 3");
        if (c->shard_mix == 3 && (long long)c->T * c->nu > 2048)
            return fail(nullptr, M3_ERR_UNSUPPORTED, "m3_create: shard_mix = 3 needs T * nu <= 2048");
        if (c->shard_mix == 3 && apply_workgroups(c->K_local) > 256)     // (m3_update_b's partial sums: one slot per workgroup)
            return fail(nullptr, M3_ERR_UNSUPPORTED, "m3_create: shard_mix = 3: K_local too large for the second exchange's partial sums");
        if (c->K_global % c->K_local != 0 || c->k_offset % c->K_local != 0 || c->K_global / c->K_local > MIX_MAX_RANKS)
            return fail(nullptr, M3_ERR_SHAPE, "m3_create: shard_mix needs equal shards (K_global = n * K_local, n <= 32)");
        if (c->K_local < M3_TOPK) return fail(nullptr, M3_ERR_SHAPE, "m3_create: shard_mix needs K_local >= 20");
        if (c->multi_modal && !c->mode_simple) {
            // the record of a one-collective multi-modal shard holds its top trajectories as float2 rows at
            // rec + K_local + 40 (regen_off_trajs): 8-byte aligned only for even K_local; shard_of() forms k / K_local
            // through a binary32 product that is exact only below 2^24
            if (c->K_local % 2) return fail(nullptr, M3_ERR_SHAPE, "m3_create: one-collective multi-modal sharding needs an even K_local");
            if (c->K_global >= (1 << 24)) return fail(nullptr, M3_ERR_SHAPE, "m3_create: one-collective multi-modal sharding needs K_global < 2^24");
        }
    }
    for (int j = 0; j < c->nu; ++j)
        if (!(c->noise_sigma_diag[j] > 0.0f) || !(c->u_max[j] >= c->u_min[j]))
            return fail(nullptr, M3_ERR_BAD_ARG, "m3_create: bad noise_sigma / bounds");
    if (!(c->gamma > 0.0f) || !(c->u_scale != 0.0f) || (c->mode_simple && !(c->lambda_ > 0.0f)))
        return fail(nullptr, M3_ERR_BAD_ARG, "m3_create: bad gamma / u_scale / lambda_");
    // noise_sigma with off-diagonal entries: Cholesky factor (MultivariateNormal, mppi.py:129-131) and inverse
    // (mppi.py:128) in binary64, rounded to f32 (for a diagonal matrix: sqrtf / 1.0f/x bit for bit)
    double chol[M3_MAX_NU * M3_MAX_NU] = {}, sinv[M3_MAX_NU * M3_MAX_NU] = {};
    if (c->full_sigma) {
        const int n = c->nu;
        for (int i = 0; i < n; ++i) {
            if (c->noise_sigma_full[i * n + i] != c->noise_sigma_diag[i])
                return fail(nullptr, M3_ERR_BAD_ARG, "m3_create: diagonal of noise_sigma_full != noise_sigma_diag");
            for (int j = 0; j < i; ++j)
                if (c->noise_sigma_full[i * n + j] != c->noise_sigma_full[j * n + i])
                    return fail(nullptr, M3_ERR_BAD_ARG, "m3_create: noise_sigma_full is not symmetric");
        }
        for (int i = 0; i < n; ++i)
            for (int j = 0; j <= i; ++j) {
                double s = (double)c->noise_sigma_full[i * n + j];
                for (int q = 0; q < j; ++q) s -= chol[i * n + q] * chol[j * n + q];
                if (i == j) {
                    if (!(s > 0.0)) return fail(nullptr, M3_ERR_BAD_ARG, "m3_create: noise_sigma_full is not positive definite");
                    chol[i * n + i] = std::sqrt(s);
                } else chol[i * n + j] = s / chol[j * n + j];
            }
        // Sigma^-1 = L^-T L^-1
        double li[M3_MAX_NU * M3_MAX_NU] = {};
        for (int j = 0; j < n; ++j) {
            li[j * n + j] = 1.0 / chol[j * n + j];
            for (int i = j + 1; i < n; ++i) {
                double s = 0.0;
                for (int q = j; q < i; ++q) s -= chol[i * n + q] * li[q * n + j];
                li[i * n + j] = s / chol[i * n + i];
            }
        }
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                double s = 0.0;
                for (int q = (i > j ? i : j); q < n; ++q) s += li[q * n + i] * li[q * n + j];
                sinv[i * n + j] = s;
            }
    }
    const bool single_halton = !c->multi_modal && !c->mode_simple;
    if (c->update_cov && single_halton && c->K_local != c->K_global)
        return fail(nullptr, M3_ERR_UNSUPPORTED, "m3_create: update_cov needs an unsharded handle");

    m3_handle* h = new (std::nothrow) m3_handle();
    if (!h) return fail(nullptr, M3_ERR_HIP, "m3_create: out of host memory");
    h->cfg = *c;
    h->cov_active = c->update_cov && single_halton && !c->sim_only;   // (elsewhere the reference ignores the flag)
    h->protocol = update_protocol(c->shard_mix, c->K_local, c->K_global, c->multi_modal, c->mode_simple);
    const UpdateAlloc ua = update_alloc(update_plan_input(h, false, false));   // what the handle's update plans need
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) {
        g_create_err = std::string("hipSetDevice: ") + hipGetErrorString(e);
        delete h;
        return M3_ERR_HIP;
    }
    if (!c->sim_only && init_ladder_table() != 0) {
        g_create_err = "m3_create: could not initialise the beta ladder table";
        delete h;
        return M3_ERR_HIP;
    }
    build_point_scene(*c, h->scene);
    h->scene_rt = make_point_scene_rt(h->point_scene, c->dt, c->substeps, c->solver_iters);
    default_world(h->world0);
    build_panda_scenes(*c, h->panda_scene, h->pscene, h->pscene_rt);
    default_panda_world(h->pworld0, c->cube_on_shelf);
    const long long Kl = c->K_local, Kg = c->K_global, T = c->T, nu = c->nu;
    const long long f = sizeof(float);
    int rc = M3_OK;
    auto A = [&](int id, long long bytes) { if (rc == M3_OK) rc = alloc_buf(h, id, bytes); };
    if (c->sim_only) {
        A(M3_BUF_INFO, sizeof(m3_info));
        if (rc != M3_OK) { g_create_err = h->err; m3_destroy(h); return rc; }
        (void)hipDeviceSynchronize();
        *out = h;
        return M3_OK;
    }
    A(M3_BUF_STATES, T * Kl * 4 * f);
    A(M3_BUF_ACTIONS, T * Kl * nu * f);
    A(M3_BUF_COST_HORIZON, T * Kl * f);
    if (!update_costs_head_record(h->protocol)) A(M3_BUF_TRAJ_COST, Kl * f);
    A(M3_BUF_TRAJ_COST_ALL, Kg * f);
    A(M3_BUF_WEIGHTS, Kg * f);
    A(M3_BUF_WEIGHTS_1, (Kg / 2) * f);
    A(M3_BUF_WEIGHTS_2, (Kg - Kg / 2) * f);
    for (int id = M3_BUF_MEAN; id <= M3_BUF_ACTION_OUT; ++id) A(id, T * nu * f);
    A(M3_BUF_TOP_IDX, M3_TOPK * sizeof(int));
    A(M3_BUF_TOP_TRAJS, M3_TOPK * T * 2 * f);
    A(M3_BUF_REDUCE, (long long)reduce_length((int)T, (int)nu) * f);
    if (!ua.noise_all) A(M3_BUF_NOISE, T * Kl * nu * f);
    A(M3_BUF_PENDING_FORCE, 4 * Kl * f);
    A(M3_BUF_INFO, sizeof(m3_info));
    A(M3_BUF_COV, 2 * nu * f);
    if (rc == M3_OK) {   // cov_action = diag(noise_sigma), scale_tril = sqrt(cov_action): mppi.py:175-176
        float cv[2 * M3_MAX_NU];
        for (int j = 0; j < nu; ++j) { cv[j] = c->noise_sigma_diag[j]; cv[nu + j] = std::sqrt(c->noise_sigma_diag[j]); }
        if (hipMemcpy(h->buf[M3_BUF_COV], cv, (size_t)(2 * nu * f), hipMemcpyHostToDevice) != hipSuccess) rc = M3_ERR_HIP;
    }
    if (rc == M3_OK && c->full_sigma) {
        float mats[2 * M3_MAX_NU * M3_MAX_NU];
        for (int i = 0; i < nu * nu; ++i) { mats[i] = (float)chol[i]; mats[nu * nu + i] = (float)sinv[i]; }
        if (own_device(h->mem, h->noise_mats, (size_t)(2 * nu * nu * f)) != hipSuccess ||
            hipMemcpy(h->noise_mats, mats, (size_t)(2 * nu * nu * f), hipMemcpyHostToDevice) != hipSuccess) rc = M3_ERR_HIP;
    }
    if (ua.noise_all) {   // (the record protocols)
        const long long rl = regen_record_length((int)Kl, (int)T);
        A(M3_BUF_RECORD, rl * f);
        A(M3_BUF_RECORDS_ALL, (Kg / Kl) * rl * f);
        if (rc == M3_OK && own_device(h->mem, h->noise_all, (size_t)(T * Kg * nu * f)) != hipSuccess) rc = M3_ERR_HIP;
        if (rc == M3_OK && hipMemsetAsync(h->noise_all, 0, (size_t)(T * Kg * nu * f), h->stream) != hipSuccess) rc = M3_ERR_HIP;
        if (rc == M3_OK && own_device(h->mem, h->local_top_idx, M3_TOPK * sizeof(int)) != hipSuccess) rc = M3_ERR_HIP;
        if (ua.record_b) {
            A(M3_BUF_RECORD_B, (long long)recb_length((int)T, (int)nu) * f);
            A(M3_BUF_RECORDS_B_ALL, (Kg / Kl) * (long long)recb_length((int)T, (int)nu) * f);
        }
        if (rc == M3_OK) {   // aliases: views of blocks adopted above, no ledger entries of their own
            h->buf[M3_BUF_TRAJ_COST] = h->buf[M3_BUF_RECORD]; h->nbytes[M3_BUF_TRAJ_COST] = Kl * f;
            h->buf[M3_BUF_NOISE] = h->noise_all + (size_t)(c->k_offset / Kl) * T * Kl * nu; h->nbytes[M3_BUF_NOISE] = T * Kl * nu * f;
            h->buf[M3_BUF_NOISE_ALL] = h->noise_all; h->nbytes[M3_BUF_NOISE_ALL] = T * Kg * nu * f;
        }
    } else if (ua.record) {
        A(M3_BUF_RECORD, (long long)record_length((int)T, (int)nu) * f);
        A(M3_BUF_RECORDS_ALL, (Kg / Kl) * (long long)record_length((int)T, (int)nu) * f);
    }
    if (rc == M3_OK && own_device(h->mem, h->world0_dev, 18 * f) != hipSuccess) rc = M3_ERR_HIP;
    if (rc == M3_OK && own_device(h->mem, h->topk_cand, (size_t)topk_workgroups((int)Kg) * M3_TOPK * sizeof(VI)) != hipSuccess) rc = M3_ERR_HIP;
    if (rc == M3_OK && own_device(h->mem, h->part_min, (size_t)mins_workgroups((int)Kg) * 3 * f) != hipSuccess) rc = M3_ERR_HIP;
    if (rc == M3_OK && own_device(h->mem, h->lad, (size_t)ladder_workgroups((int)Kg) * 96 * 3 * f) != hipSuccess) rc = M3_ERR_HIP;
    if (rc == M3_OK && own_device(h->mem, h->wpart, (size_t)(ua.partials_all ? std::max(wsum_chunks((int)Kg), regen_chunks((int)Kg)) : wsum_chunks((int)Kl)) * 3 * T * nu * f) != hipSuccess) rc = M3_ERR_HIP;
    if (rc == M3_OK && own_device(h->mem, h->apart, (size_t)(16 + std::max(apply_workgroups((int)Kg), ua.partials_all ? regen_chunks((int)Kg) : 0) * 8) * f) != hipSuccess) rc = M3_ERR_HIP;
    if (rc == M3_OK && ua.large_form) {   // the three-launch form (update.hip: k_ladder_search)
        const size_t nl = (size_t)ladder_workgroups((int)Kg);
        if (own_device(h->mem, h->wave_min, (size_t)Kl * 3 * f) != hipSuccess) rc = M3_ERR_HIP;      // (one row per rollout workgroup: <= K_local with one lane per wavefront)
        if (rc == M3_OK && own_device(h->mem, h->lflag, nl * sizeof(int)) != hipSuccess) rc = M3_ERR_HIP;
        if (rc == M3_OK && hipMemset(h->lflag, 0, nl * sizeof(int)) != hipSuccess) rc = M3_ERR_HIP;
    }
    if (rc == M3_OK && c->env_type == M3_ENV_PANDA) {
        // Everything a panda command may need is allocated HERE (no allocation in m3_command).  The word of
        // mapped host memory the rollout's last wavefront reports its near share into + its counter; and, for a handle
        // whose reach task takes quirk Q8's shadow slots (unsharded), the records between the rollout and
        // k_panda_reach_cost ([T][17][K] floats: 5.4 MB at C4).
        void* d = nullptr;
        if (own_pinned(h->mem, h->panda_busy_hint, sizeof(int), hipHostMallocMapped) != hipSuccess ||
            own_device(h->mem, h->panda_busy_count, sizeof(unsigned long long)) != hipSuccess ||
            hipMemset(h->panda_busy_count, 0, sizeof(unsigned long long)) != hipSuccess || hipHostGetDevicePointer(&d, h->panda_busy_hint, 0) != hipSuccess) {
            h->err = "m3_create: the panda rollout's report word (mapped host memory) could not be allocated";
            rc = M3_ERR_HIP;
        } else {
            h->panda_busy_hint_dev = (int*)d;
            *h->panda_busy_hint = 0;
        }
        if (rc == M3_OK && Kl == Kg && Kg >= 2 && Kl <= PANDA_REACH_REC_MAX_K &&
            own_device(h->mem, h->panda_reach_rec, (size_t)T * REACH_REC * (size_t)Kl * f) != hipSuccess) rc = M3_ERR_HIP;
    }
    if (rc == M3_OK && c->env_type == M3_ENV_POINT && !c->sim_only) {
        // the word the two-wavefront rollout form reports a hand-over wait that ran out into (mapped host memory: m3_rollout
        // reads it without a synchronisation, so it refuses the rollout AFTER the one that failed)
        void* d = nullptr;
        if (own_pinned(h->mem, h->rollout_err, sizeof(int), hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&d, h->rollout_err, 0) != hipSuccess) {
            h->err = "m3_create: the point rollout's error word (mapped host memory) could not be allocated";
            rc = M3_ERR_HIP;
        } else {
            h->rollout_err_dev = (int*)d;
            *h->rollout_err = 0;
        }
    }
    if (rc == M3_OK && own_device(h->mem, h->wcount, (size_t)(T + 2) * sizeof(int)) != hipSuccess) rc = M3_ERR_HIP;
    if (rc == M3_OK && hipMemset(h->wcount, 0, (size_t)(T + 2) * sizeof(int)) != hipSuccess) rc = M3_ERR_HIP;
    if (rc == M3_OK) {
        m3_info init;
        std::memset(&init, 0, sizeof(init));
        init.beta = init.beta_1 = init.beta_2 = 1.0f;  // mppi.py:184-187
        if (hipMemcpy(h->buf[M3_BUF_INFO], &init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess) rc = M3_ERR_HIP;
    }
    if (rc != M3_OK) {
        g_create_err = h->err.empty() ? "m3_create: device allocation failed" : h->err;
        m3_destroy(h);
        return rc;
    }
    (void)hipDeviceSynchronize();
    *out = h;
    return M3_OK;
}

extern "C" void m3_destroy(m3_handle* h) {
    if (!h) return;
    h->mem.release_all();
    delete h;
}

#ifndef M3_BUILD_ID
#define M3_BUILD_ID "unknown"
#endif
extern "C" const char* m3_build_id(void) { return M3_BUILD_ID; }

extern "C" int m3_set_stream(m3_handle* h, void* s) {
    if (!h) return M3_ERR_BAD_ARG;
    h->stream = (hipStream_t)s;
    return M3_OK;
}

extern "C" int m3_set_rollout_lanes(m3_handle* h, int lanes) {
    if (!h) return M3_ERR_BAD_ARG;
    if (lanes != 0 && (lanes < 1 || lanes > 64 || (lanes & (lanes - 1)) != 0))
        return fail(h, M3_ERR_BAD_ARG, "m3_set_rollout_lanes: lanes must be 0 (auto) or a power of two in 1..64");
    h->lanes_override = lanes;
    return M3_OK;
}

extern "C" int m3_set_point_rollout_form(m3_handle* h, int form) {
    if (!h) return M3_ERR_BAD_ARG;
    if (form < -1 || form > 1) return fail(h, M3_ERR_BAD_ARG, "m3_set_point_rollout_form: 0 (one wavefront), 1 (two) or -1 (automatic)");
    h->point_form = form;
    return M3_OK;
}

extern "C" int m3_point_rollout_form_used(m3_handle* h) {
    return h ? h->point_form_used : -1;
}

extern "C" int m3_wave_order(m3_handle* h, const int** order_dev, int* n) {
    if (!h || !order_dev || !n) return fail(h, M3_ERR_BAD_ARG, "m3_wave_order: null argument");
    *order_dev = nullptr;
    *n = 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->order_valid) {   // (set by the last rollout's refresh_wave_order; every refusal there leaves it false)
        *order_dev = h->order;
        *n = h->cfg.K_local;
    }
    return M3_OK;
}

extern "C" int m3_set_panda_lanes_per_sample(m3_handle* h, int lps) {
    if (!h) return M3_ERR_BAD_ARG;
    if (lps != 0 && lps != 1 && lps != 8 && lps != 16)
        return fail(h, M3_ERR_BAD_ARG, "m3_set_panda_lanes_per_sample: 0 (by size), 1, 8 or 16");
    h->panda_lps = lps;
    return M3_OK;
}

extern "C" int m3_set_panda_reach_cost_kernel(m3_handle* h, int on) {
    if (!h) return M3_ERR_BAD_ARG;
    h->panda_reach_deferred = on != 0;
    return M3_OK;
}

extern "C" int m3_panda_near_share(m3_handle* h) {
    return (h && h->panda_busy_hint) ? *(volatile const int*)h->panda_busy_hint - 1 : -1;
}

extern "C" int m3_panda_lanes_per_sample_used(m3_handle* h) {
    return h ? h->panda_lps_used : 0;
}

extern "C" int m3_set_update_launches(m3_handle* h, int launches) {
    if (!h) return M3_ERR_BAD_ARG;
    if (launches != 0 && launches != 3 && launches != 5) return fail(h, M3_ERR_BAD_ARG, "m3_set_update_launches: 0 (default), 3 or 5");
    h->five_launches = launches == 5;
    return M3_OK;
}

extern "C" int m3_set_ladder_spins(m3_handle* h, int spins) {
    if (!h) return M3_ERR_BAD_ARG;
    if (spins < -1) return fail(h, M3_ERR_BAD_ARG, "m3_set_ladder_spins: -1 (default), 0 (never wait) or a positive bound");
    h->ladder_spins = spins < 0 ? (1 << 18) : spins;
    return M3_OK;
}

extern "C" int m3_enable_timing(m3_handle* h, int on) {
    if (!h) return M3_ERR_BAD_ARG;
    if (on && !h->ev[0]) {
        BlockGroup g(h->mem);   // all four or none
        for (auto& ev : h->ev) HIPCHK(h, own_event(h->mem, ev));
        g.keep = true;
    }
    h->timing = on != 0;
    return M3_OK;
}

// (re)computes the wavefront order of the samples (sampler.hip) from the noise buffer and the
// current world; stream-ordered, no sync.  Called by m3_rollout when the noise changed and every
// ORDER_REFRESH commands (the objects move).
constexpr unsigned ORDER_REFRESH = 256;
// first local index of the second mode inside the block that starts at global sample k_offset (0 .. K_local)
static int block_half(const m3_config& c, int k_offset) {
    long long half_local = (long long)(c.K_global / 2) - k_offset;
    if (!c.multi_modal || half_local > c.K_local) half_local = c.K_local;
    if (half_local < 0) half_local = 0;
    return (int)half_local;
}

// one shard's block of noise rows [T][Kl][nu] (k_offset = global index of its first sample): sort into
// wavefront order; `relabel`: write the rows back in that order (and, for this rank's own block, let the
// pending suction forces follow their samples)
static int order_block(m3_handle* h, float* block, int k_offset, bool relabel, bool own) {
    const m3_config& c = h->cfg;
    const int half_local = block_half(c, k_offset);
    OrderScene os;
    std::memset(&os, 0, sizeof(os));
    if (h->bind_dof) { os.sim_root = h->bind_root; os.sim_box = h->bind_box; os.sim_dyn = h->bind_dyn; }
    os.bx = h->world0[4]; os.by = h->world0[5]; os.dx = h->world0[11]; os.dy = h->world0[12];
    os.ox = h->point_scene.obs_x; os.oy = h->point_scene.obs_y;   // (the handle's arena; the default: PointScene's constants)
    // relabelling keeps the samples with a role of their own at their index
    const int specials[3] = {0 - k_offset, c.K_global / 2 - k_offset, c.K_global - 1 - k_offset};
    hipError_t e = launch_wave_order(block, c.K_local, c.T, c.nu,
                                     std::sqrt(c.noise_sigma_diag[0]), std::sqrt(c.noise_sigma_diag[1]),
                                     half_local, os, h->order_scratch, h->order_temp_bytes, h->order, h->noise_sorted,
                                     relabel ? specials : nullptr, h->stream);
    if (e != hipSuccess) { h->err = std::string("wave order: ") + hipGetErrorString(e); return M3_ERR_HIP; }
    if (relabel) {
        // sample i := old sample order[i]: the noise rows (gathered above) and the per-sample state
        // that outlives a command (pending suction forces) move; everything else is rewritten by
        // the next rollout.  From here on the index order IS the wavefront order: coalesced stores.
        HIPCHK(h, hipMemcpyAsync(block, h->noise_sorted, sizeof(float) * (size_t)c.T * c.K_local * c.nu,
                                 hipMemcpyDeviceToDevice, h->stream));
        if (own) {
            launch_gather_rows((const float*)h->buf[M3_BUF_PENDING_FORCE], h->order, h->noise_sorted, c.K_local, 4, h->stream);
            HIPCHK(h, hipMemcpyAsync(h->buf[M3_BUF_PENDING_FORCE], h->noise_sorted, sizeof(float) * 4 * (size_t)c.K_local,
                                     hipMemcpyDeviceToDevice, h->stream));
        }
    }
    return M3_OK;
}

static int refresh_wave_order(m3_handle* h) {
    const m3_config& c = h->cfg;
    h->order_valid = false;
    h->order_dirty = false;
    const bool relabel = h->relabel_pending;
    h->relabel_pending = false;
    if (h->relabelled && !relabel) return M3_OK;   // rows already in wavefront order: by index
    // (a caller that uploads fresh noise for almost every command would pay the sort -- ~25 us --
    // more often than it pays back: by index then)
    if (!h->wave_order || c.env_type != M3_ENV_POINT || c.nu != 2 || c.K_local < 128 || c.sampling_random ||
        c.mode_simple || !h->have_noise || h->noise_churn >= 2)
        return M3_OK;
    if (!h->order) {
        // the sort's own storage: for the largest range any block of this handle is sorted in (each mode's part of its own
        // block; of every shard's block where the handle holds them all) -- the configuration fixes them, so sized once
        size_t temp = 0;
        const bool all = update_noise_of_all_ranks(h->protocol);
        const int nb = all ? c.K_global / c.K_local : 1;
        for (int r = 0; r < nb; ++r) {
            const int half = block_half(c, all ? r * c.K_local : c.k_offset);
            temp = std::max(temp, std::max(wave_order_temp_bytes(half), wave_order_temp_bytes(c.K_local - half)));
        }
        h->order_temp_bytes = temp;
        BlockGroup g(h->mem);   // all three or none: a failure leaves order null, the next rollout tries again
        HIPCHK(h, own_device(h->mem, h->order, sizeof(int) * (size_t)c.K_local));
        HIPCHK(h, own_device(h->mem, h->order_scratch, 3 * sizeof(float) * (size_t)c.K_local + h->order_temp_bytes));
        HIPCHK(h, own_device(h->mem, h->noise_sorted, sizeof(float) * (size_t)c.T * c.K_local * c.nu));
        g.keep = true;
    }
    if (relabel && update_noise_of_all_ranks(h->protocol)) {
        // every rank holds every shard's noise block (the other ranks' actions are re-generated from
        // them): relabel each block exactly as its owner does -- the same deterministic procedure on the
        // same inputs (noise table, world) -- this rank's own block LAST, so that h->order ends up as its
        // permutation
        const int n = c.K_global / c.K_local, me = c.k_offset / c.K_local;
        const size_t bl = (size_t)c.T * c.K_local * c.nu;
        for (int q = 0; q < n; ++q) {
            const int r = (q < me) ? q : (q + 1 < n ? q + 1 : me);   // 0..me-1, me+1..n-1, me
            const int rc = order_block(h, h->noise_all + (size_t)r * bl, r * c.K_local, true, r == me);
            if (rc != M3_OK) return rc;
        }
        h->relabelled = true;
        return M3_OK;
    }
    const int rc = order_block(h, (float*)h->buf[M3_BUF_NOISE], c.k_offset, relabel, true);
    if (rc != M3_OK) return rc;
    if (relabel) {
        h->relabelled = true;
        return M3_OK;
    }
    h->order_valid = true;
    return M3_OK;
}

extern "C" int m3_relabel_samples(m3_handle* h) {
    if (!h) return M3_ERR_BAD_ARG;
    if (!h->have_noise) return fail(h, M3_ERR_STATE, "m3_relabel_samples: no noise set");
    h->relabel_pending = true;
    h->order_dirty = true;
    return M3_OK;
}

static void note_noise_upload(m3_handle* h) {
    h->relabelled = false;
    h->relabel_pending = false;
    h->noise_churn = (h->have_noise && h->calls - h->last_noise_call < 16u) ? h->noise_churn + 1 : 0;
    h->last_noise_call = h->calls;
    h->have_noise = true;
    h->order_dirty = true;
}

extern "C" int m3_set_wave_order(m3_handle* h, int on) {
    if (!h) return M3_ERR_BAD_ARG;
    h->wave_order = on != 0;
    h->order_dirty = true;
    return M3_OK;
}

// rows [n_rows][T][nu] (reference layout) -> n_rows / K_local consecutive time-major blocks at dst
static int upload_noise(m3_handle* h, const float* delta, long long n_rows, float* dst, int on_device, const char* who) {
    if (!h || !delta) return fail(h, M3_ERR_BAD_ARG, "m3_set_noise: null argument");
    const m3_config& c = h->cfg;
    (void)who;
    const size_t bytes = (size_t)n_rows * c.T * c.nu * sizeof(float);
    const float* src = delta;
    ScopedBlock<float> tmp(h->mem);   // the staging block of a global upload: every exit frees it
    if (!on_device) {
        float* stage = nullptr;
        if (n_rows == c.K_local) {
            if (!h->noise_stage) HIPCHK(h, own_device(h->mem, h->noise_stage, bytes));
            stage = h->noise_stage;
        } else {
            HIPCHK(h, own_device(h->mem, tmp.p, bytes));
            stage = tmp.p;
        }
        HIPCHK(h, hipMemcpyAsync(stage, delta, bytes, hipMemcpyHostToDevice, h->stream));
        src = stage;
    }
    const size_t bl = (size_t)c.T * c.K_local * c.nu;
    for (long long r = 0; r < n_rows / c.K_local; ++r)
        launch_transpose_noise(src + r * bl, dst + r * bl, c.K_local, c.T, c.nu, h->stream);
    hipError_t e = hipGetLastError();
    if (!on_device) (void)hipStreamSynchronize(h->stream);  // host buffer may be released
    if (e != hipSuccess) { h->err = std::string("k_transpose_noise: ") + hipGetErrorString(e); return M3_ERR_HIP; }
    note_noise_upload(h);
    return M3_OK;
}

extern "C" int m3_set_noise(m3_handle* h, const float* delta, int on_device) {
    if (!h) return M3_ERR_BAD_ARG;
    if (h->cfg.sim_only) return fail(h, M3_ERR_STATE, "m3_set_noise: handle was created sim_only");
    if (update_noise_of_all_ranks(h->protocol)) return fail(h, M3_ERR_STATE, "m3_set_noise: a one-collective multi-modal shard needs the noise rows of ALL "
                                               "K_global samples (m3_set_noise_global)");
    return upload_noise(h, delta, h->cfg.K_local, (float*)h->buf[M3_BUF_NOISE], on_device, "m3_set_noise");
}

extern "C" int m3_set_noise_global(m3_handle* h, const float* delta_all, int on_device) {
    if (!h) return M3_ERR_BAD_ARG;
    if (!update_noise_of_all_ranks(h->protocol)) return fail(h, M3_ERR_STATE, "m3_set_noise_global: only for one-collective multi-modal shards "
                                                "(cfg.shard_mix with multi_modal, K_local < K_global)");
    return upload_noise(h, delta_all, h->cfg.K_global, h->noise_all, on_device, "m3_set_noise_global");
}

static int upload_knots(m3_handle* h, const float* knots, long long n_rows, float* dst, int n_knots, int degree,
                        float smoothing, int on_device) {
    if (!h || !knots) return fail(h, M3_ERR_BAD_ARG, "m3_set_noise_knots: null argument");
    const m3_config& c = h->cfg;
    if (c.sim_only) return fail(h, M3_ERR_STATE, "m3_set_noise_knots: handle was created sim_only");
    if (degree < 1 || degree > 3) return fail(h, M3_ERR_BAD_ARG, "m3_set_noise_knots: degree must be 1..3");
    if (n_knots <= degree || n_knots > 64)
        return fail(h, M3_ERR_SHAPE, "m3_set_noise_knots: needs degree < n_knots <= 64 (splrep: m > k must hold)");
    if (!(smoothing >= 0.0f)) return fail(h, M3_ERR_BAD_ARG, "m3_set_noise_knots: smoothing must be >= 0");
    const size_t bytes = (size_t)n_rows * c.nu * n_knots * sizeof(float);
    const float* src = knots;
    ScopedBlock<float> stage(h->mem);
    if (!on_device) {
        HIPCHK(h, own_device(h->mem, stage.p, bytes));
        HIPCHK(h, hipMemcpyAsync(stage.p, knots, bytes, hipMemcpyHostToDevice, h->stream));
        src = stage.p;
    }
    const size_t bl = (size_t)c.T * c.K_local * c.nu, kl = (size_t)c.K_local * c.nu * n_knots;
    for (long long r = 0; r < n_rows / c.K_local; ++r)
        launch_spline_noise(src + r * kl, dst + r * bl, c.K_local, c.nu, n_knots, c.T, degree, (double)smoothing, h->stream);
    hipError_t e = hipGetLastError();
    if (stage.p) (void)hipStreamSynchronize(h->stream);   // (before the block goes)
    if (e != hipSuccess) { h->err = std::string("k_spline_noise: ") + hipGetErrorString(e); return M3_ERR_HIP; }
    note_noise_upload(h);
    return M3_OK;
}

extern "C" int m3_set_noise_knots(m3_handle* h, const float* knots, int n_knots, int degree, float smoothing,
                                  int on_device) {
    if (!h) return M3_ERR_BAD_ARG;
    if (update_noise_of_all_ranks(h->protocol)) return fail(h, M3_ERR_STATE, "m3_set_noise_knots: a one-collective multi-modal shard needs the knots of ALL "
                                               "K_global samples (m3_set_noise_knots_global)");
    return upload_knots(h, knots, h->cfg.K_local, (float*)h->buf[M3_BUF_NOISE], n_knots, degree, smoothing, on_device);
}

extern "C" int m3_set_noise_knots_global(m3_handle* h, const float* knots_all, int n_knots, int degree, float smoothing,
                                         int on_device) {
    if (!h) return M3_ERR_BAD_ARG;
    if (!update_noise_of_all_ranks(h->protocol)) return fail(h, M3_ERR_STATE, "m3_set_noise_knots_global: only for one-collective multi-modal shards");
    return upload_knots(h, knots_all, h->cfg.K_global, h->noise_all, n_knots, degree, smoothing, on_device);
}

// the whole reference sampler on the device: Halton -> erfinv -> smoothing spline (no host values at all)
// Faure's permutations (H. Faure, "Good permutations for extreme discrepancy", J. Number Theory 42 (1992) 47-56),
// defined recursively: pi_2 = (0 1); for even b = 2k, pi_b = (2 pi_k, 2 pi_k + 1); for odd b = 2k + 1, pi_b is
// pi_2k with every value >= k increased by one and the value k inserted in the middle.  pi_b(0) = 0 for every b.
static std::vector<int> faure_permutation(int b) {
    if (b == 2) return {0, 1};
    std::vector<int> r;
    if (b % 2 == 0) {
        const std::vector<int> hlf = faure_permutation(b / 2);
        for (int x : hlf) r.push_back(2 * x);
        for (int x : hlf) r.push_back(2 * x + 1);
    } else {
        const int k = (b - 1) / 2;
        r = faure_permutation(b - 1);
        for (int& x : r) if (x >= k) x += 1;
        r.insert(r.begin() + k, k);
    }
    return r;
}

extern "C" int m3_set_noise_halton_scrambled(m3_handle* h, int n_knots, int degree, float smoothing, int scramble) {
    if (!h) return M3_ERR_BAD_ARG;
    const m3_config& c = h->cfg;
    if (c.sim_only) return fail(h, M3_ERR_STATE, "m3_set_noise_halton: handle was created sim_only");
    if (scramble != M3_HALTON_PLAIN && scramble != M3_HALTON_FAURE)
        return fail(h, M3_ERR_BAD_ARG, "m3_set_noise_halton_scrambled: scramble must be M3_HALTON_PLAIN or M3_HALTON_FAURE");
    const int ncol = c.nu * n_knots;
    if (n_knots < 1 || ncol > 100) return fail(h, M3_ERR_SHAPE, "m3_set_noise_halton: nu * n_knots must be <= 100 (mppi_utils.py:81)");
    int primes[100], np_ = 0;
    for (int cand = 2; np_ < ncol; ++cand) {
        bool is_p = true;
        for (int q = 0; q < np_ && primes[q] * primes[q] <= cand; ++q)
            if (cand % primes[q] == 0) { is_p = false; break; }
        if (is_p) primes[np_++] = cand;
    }
    std::vector<int> perm, perm_off;
    if (scramble == M3_HALTON_FAURE)
        for (int j = 0; j < ncol; ++j) {
            perm_off.push_back((int)perm.size());
            const std::vector<int> pj = faure_permutation(primes[j]);
            perm.insert(perm.end(), pj.begin(), pj.end());
        }
    const bool all = update_noise_of_all_ranks(h->protocol);
    const long long rows = all ? c.K_global : c.K_local;
    const int k0 = all ? 0 : c.k_offset;
    ScopedBlock<float> knots_blk(h->mem);
    ScopedBlock<int> tab_blk(h->mem);   // primes | perm offsets | permutations
    const size_t ntab = (size_t)ncol + perm_off.size() + perm.size();
    HIPCHK(h, own_device(h->mem, knots_blk.p, (size_t)rows * ncol * sizeof(float)));
    if (own_device(h->mem, tab_blk.p, ntab * sizeof(int)) != hipSuccess) return fail(h, M3_ERR_HIP, "m3_set_noise_halton: hipMalloc");
    float* const knots = knots_blk.p;
    int* const tab = tab_blk.p;
    std::vector<int> host(primes, primes + ncol);
    host.insert(host.end(), perm_off.begin(), perm_off.end());
    host.insert(host.end(), perm.begin(), perm.end());
    int rc = M3_OK;
    if (hipMemcpyAsync(tab, host.data(), ntab * sizeof(int), hipMemcpyHostToDevice, h->stream) != hipSuccess) rc = M3_ERR_HIP;
    if (rc == M3_OK) {
        const bool sc = scramble != M3_HALTON_PLAIN;
        launch_halton_knots(knots, k0, (int)rows, ncol, tab, sc ? tab + 2 * ncol : nullptr, sc ? tab + ncol : nullptr, h->stream);
        // knots [rows][nu][n_knots] == [rows][ncol]: column j * n_knots + q is knot q of control dimension j
        rc = upload_knots(h, knots, rows, all ? h->noise_all : (float*)h->buf[M3_BUF_NOISE], n_knots, degree, smoothing, 1);
    }
    (void)hipStreamSynchronize(h->stream);     // (also keeps `host` alive until the copy is done; then the two blocks go)
    if (rc != M3_OK && h->err.empty()) h->err = "m3_set_noise_halton failed";
    return rc;
}

extern "C" int m3_set_noise_halton(m3_handle* h, int n_knots, int degree, float smoothing) {
    return m3_set_noise_halton_scrambled(h, n_knots, degree, smoothing, M3_HALTON_PLAIN);
}

extern "C" int m3_sample_noise(m3_handle* h) {
    if (!h) return M3_ERR_BAD_ARG;
    const m3_config& c = h->cfg;
    if (c.sim_only || !(c.sampling_random || c.mode_simple))
        return fail(h, M3_ERR_STATE, "m3_sample_noise: the handle has a noise table (sampling_random == 0)");
    if (update_noise_of_all_ranks(h->protocol)) return fail(h, M3_ERR_STATE, "m3_sample_noise: not on a one-collective multi-modal shard");
    RolloutArgs a;
    std::memset(&a, 0, sizeof(a));
    a.Kg = c.K_global; a.Kl = c.K_local; a.k0 = c.k_offset; a.T = c.T; a.nu = c.nu;
    a.full_sigma = c.full_sigma; a.noise_mats = h->noise_mats;
    for (int j = 0; j < c.nu; ++j) { a.noise_mu[j] = c.noise_mu[j]; a.scale_tril[j] = std::sqrt(c.noise_sigma_diag[j]); }
    a.seed = c.seed; a.call = h->calls;
    launch_sample_noise(a, (float*)h->buf[M3_BUF_NOISE], h->stream);
    HIPCHK(h, hipGetLastError());
    return M3_OK;
}

extern "C" int m3_set_objective(m3_handle* h, int task, const float* goal, int goal_len, int gripper_cmd) {
    if (!h) return M3_ERR_BAD_ARG;
    if (task < 0 || task > M3_TASK_IDLE) return fail(h, M3_ERR_BAD_ARG, "m3_set_objective: unknown task");
    if (goal_len < 0 || goal_len > 7 || (goal_len > 0 && !goal)) return fail(h, M3_ERR_SHAPE, "m3_set_objective: bad goal");
    if (h->cfg.env_type == M3_ENV_POINT && task > M3_TASK_PUSH_PULL)
        return fail(h, M3_ERR_UNSUPPORTED, "m3_set_objective: task not defined for point_env");
    if (h->cfg.env_type == M3_ENV_POINT && goal_len < 2) return fail(h, M3_ERR_SHAPE, "m3_set_objective: point_env goal needs 2 values");
    if (h->cfg.env_type == M3_ENV_PANDA && task <= M3_TASK_PUSH_PULL)
        return fail(h, M3_ERR_UNSUPPORTED, "m3_set_objective: task not defined for panda_env");
    if (h->cfg.env_type == M3_ENV_PANDA && task == M3_TASK_PICK && goal_len < 7)
        return fail(h, M3_ERR_SHAPE, "m3_set_objective: pick needs a 7-value goal pose (cost_functions.py:116-123)");
    if (task == M3_TASK_PUSH_PULL && !h->cfg.multi_modal)
        return fail(h, M3_ERR_STATE, "m3_set_objective: push_pull needs multi_modal (cost_functions.py:27-29)");
    h->task = task;
    for (int i = 0; i < goal_len; ++i) h->goal[i] = goal[i];
    h->gripper_cmd = gripper_cmd;
    return M3_OK;
}

extern "C" int m3_set_avoid_dyn_obs(m3_handle* h, int on) {
    if (!h) return M3_ERR_BAD_ARG;
    if (h->cfg.env_type != M3_ENV_POINT) return fail(h, M3_ERR_UNSUPPORTED, "m3_set_avoid_dyn_obs: point_env only");
    h->avoid_dyn_obs = on != 0;
    return M3_OK;
}

static const char* env_only_text(int env) { return env == M3_ENV_POINT ? ": point_env only" : ": panda_env only"; }

// ---- the tri-state instance switches of both environments (m3_set_weighted_cost_instance, m3_set_point_scene_instance and
// their panda twins): -1 by `by` (the handle's weights or values), 0 / 1 forced ----
static int set_instance(m3_handle* h, int env, int m3_handle::*member, int on, const char* who, const char* by) {
    if (!h) return M3_ERR_BAD_ARG;
    if (h->cfg.env_type != env) return fail(h, M3_ERR_UNSUPPORTED, (std::string(who) + env_only_text(env)).c_str());
    if (on < -1 || on > 1) return fail(h, M3_ERR_BAD_ARG, (std::string(who) + ": -1 (by the " + by + "), 0 or 1").c_str());
    h->*member = on;
    return M3_OK;
}

// ---- the cost weights of both environments (extension; per-handle state like the objective: a fixed member, written in place --
// no allocation, no synchronisation).  The public struct is n floats in the layout of the member ----
static const char* const COST_WEIGHT_NAMES[9] = {"nav_dist", "collision", "robot_box", "box_goal", "push_dist",
                                                 "push_align", "pull_dist", "pull_vel", "pull_align"};
static_assert(sizeof(m3_point_cost_weights) == 9 * sizeof(float) && sizeof(PointCostWeights) == sizeof(m3_point_cost_weights),
              "m3_point_cost_weights: nine floats, the layout of PointCostWeights");
static const char* const PANDA_COST_WEIGHT_NAMES[7] = {"reach_dist", "reach_tilt", "pick_goal", "pick_ori", "collision",
                                                       "shelf_force", "place_grip"};
static_assert(sizeof(m3_panda_cost_weights) == 7 * sizeof(float) && sizeof(PandaCostWeights) == sizeof(m3_panda_cost_weights),
              "m3_panda_cost_weights: seven floats, the layout of PandaCostWeights");

// w: the public struct (null: the defaults); names[n]: its fields
template <class W>
static int set_cost_weights(m3_handle* h, int env, W m3_handle::*member, const W& defaults, const void* w, const char* const* names,
                            int n, const char* who) {
    if (!h) return M3_ERR_BAD_ARG;
    if (h->cfg.env_type != env) return fail(h, M3_ERR_UNSUPPORTED, (std::string(who) + env_only_text(env)).c_str());
    if (!w) { h->*member = defaults; return M3_OK; }
    const float* f = static_cast<const float*>(w);
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(f[i])) return fail(h, M3_ERR_BAD_ARG, (std::string(who) + ": " + names[i] + " is not finite").c_str());
    std::memcpy(&(h->*member), w, sizeof(W));
    return M3_OK;
}
template <class W> static int get_cost_weights(const m3_handle* h, int env, W m3_handle::*member, void* out) {
    if (!h || !out) return M3_ERR_BAD_ARG;
    if (h->cfg.env_type != env) return M3_ERR_UNSUPPORTED;
    std::memcpy(out, &(h->*member), sizeof(W));
    return M3_OK;
}

extern "C" void m3_default_point_cost_weights(m3_point_cost_weights* w) { if (w) std::memcpy(w, &POINT_COST_WEIGHTS_DEFAULT, sizeof(*w)); }
extern "C" int m3_set_point_cost_weights(m3_handle* h, const m3_point_cost_weights* w) {
    return set_cost_weights(h, M3_ENV_POINT, &m3_handle::cost_weights, POINT_COST_WEIGHTS_DEFAULT, w, COST_WEIGHT_NAMES, 9, "m3_set_point_cost_weights");
}
extern "C" int m3_get_point_cost_weights(const m3_handle* h, m3_point_cost_weights* out) { return get_cost_weights(h, M3_ENV_POINT, &m3_handle::cost_weights, out); }
extern "C" int m3_set_weighted_cost_instance(m3_handle* h, int on) {
    return set_instance(h, M3_ENV_POINT, &m3_handle::weighted_instance, on, "m3_set_weighted_cost_instance", "weights");
}

extern "C" void m3_default_panda_cost_weights(m3_panda_cost_weights* w) { if (w) std::memcpy(w, &PANDA_COST_WEIGHTS_DEFAULT, sizeof(*w)); }
extern "C" int m3_set_panda_cost_weights(m3_handle* h, const m3_panda_cost_weights* w) {
    return set_cost_weights(h, M3_ENV_PANDA, &m3_handle::panda_cost_weights, PANDA_COST_WEIGHTS_DEFAULT, w, PANDA_COST_WEIGHT_NAMES, 7, "m3_set_panda_cost_weights");
}
extern "C" int m3_get_panda_cost_weights(const m3_handle* h, m3_panda_cost_weights* out) { return get_cost_weights(h, M3_ENV_PANDA, &m3_handle::panda_cost_weights, out); }
extern "C" int m3_set_panda_weighted_cost_instance(m3_handle* h, int on) {
    return set_instance(h, M3_ENV_PANDA, &m3_handle::panda_weighted_instance, on, "m3_set_panda_weighted_cost_instance", "weights");
}

// the handle's weights are the defaults bit for bit (-0.0f is not 0.0f here: the kernels multiply by them)
static bool default_cost_weights(const m3_handle* h) {
    return std::memcmp(&h->cost_weights, &POINT_COST_WEIGHTS_DEFAULT, sizeof(PointCostWeights)) == 0;
}

// ---- the point_env arena (extension; per-handle state like the cost weights: no allocation, no synchronisation) ----
static const char* const SCENE_FIELD_NAMES[28] = {
    "robot_r", "robot_m", "box_hx", "box_hy", "box_m", "box_I", "box_mu_g", "box_req", "dyn_hx", "dyn_hy", "dyn_m", "dyn_I",
    "dyn_mu_g", "dyn_req", "obs_x", "obs_y", "obs_hx", "obs_hy", "wall", "mu_rb", "mu_rd", "mu_ro", "mu_rw", "mu_bw", "mu_dw",
    "mu_bd", "mu_bo", "mu_do"};
// what a field must satisfy: 0 any finite value (a position), 1 > 0 (size, mass, inertia, lever arm), 2 >= 0 (friction)
static const int SCENE_FIELD_RULE[28] = {1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1, 1, 2, 1, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2};
static_assert(sizeof(m3_point_scene) == 28 * sizeof(float), "m3_point_scene: twenty-eight floats");

// the per-field checks of an arena, shared by m3_set_point_scene and every row of m3_set_point_scene_rows: empty if it passes,
// else "<field> <what is wrong>"
static std::string point_scene_fault(const m3_point_scene& src) {
    const float* f = reinterpret_cast<const float*>(&src);
    for (int i = 0; i < 28; ++i) {
        const char* what = !std::isfinite(f[i]) ? " is not finite"
                           : (SCENE_FIELD_RULE[i] == 1 && !(f[i] > 0.0f)) ? " must be > 0"
                           : (SCENE_FIELD_RULE[i] == 2 && f[i] < 0.0f) ? " must be >= 0" : nullptr;
        if (what) return std::string(SCENE_FIELD_NAMES[i]) + what;
    }
    if (!(src.wall > src.robot_r)) return "wall must be > robot_r";
    return std::string();
}

// ---- the two kinds of run-time scene, the point_env arena and the panda_env workspace: what differs between them, once.  The
// single scene (m3_set_*_scene), the rows per environment of a sim_only handle (m3_set_*_scene_rows) and per sample of a
// planner's rollout (m3_set_*_rollout_scenes) are the templates below over a kind.  Per-handle state like the cost weights:
// the single scene is a fixed member, written in place -- no allocation, no synchronisation ----
struct PointSceneKind {
    using Scene = m3_point_scene;
    static constexpr int ENV = M3_ENV_POINT;
    static constexpr const Scene& DEFAULT = POINT_SCENE_DEFAULT;
    static constexpr int ROW_WORDS = POINT_SCENE_ROW_WORDS;
    static constexpr Scene m3_handle::*SINGLE = &m3_handle::point_scene;
    static constexpr SceneRows<Scene> m3_handle::*ROWS = &m3_handle::point_rows;
    static constexpr const char* SET_SCENE = "m3_set_point_scene";
    static constexpr const char* SET_ENV_ROWS = "m3_set_point_scene_rows";
    static constexpr const char* SET_SAMPLE_ROWS = "m3_set_point_rollout_scenes";
    // (what a planner handle is told by m3_set_point_scene_rows; out of date since m3_set_point_rollout_scenes exists, kept as it is)
    static constexpr const char* PLANNER_HINT = "a planner's rollouts share one model: m3_set_point_scene";
    static std::string fault(const Scene& sc) { return point_scene_fault(sc); }
    // the handle's derived copy of its single scene
    static void rebuild(m3_handle* h) { h->scene_rt = make_point_scene_rt(h->point_scene, h->cfg.dt, h->cfg.substeps, h->cfg.solver_iters); }
    static void pack_row(const m3_config& c, const Scene& sc, float* table, int Kl, int i) {
        point_scene_row_pack(make_point_scene_rt(sc, c.dt, c.substeps, c.solver_iters), table, Kl, i);
    }
};
struct PandaSceneKind {
    using Scene = m3_panda_scene;
    static constexpr int ENV = M3_ENV_PANDA;
    static constexpr const Scene& DEFAULT = PANDA_SCENE_DEFAULT;
    static constexpr int ROW_WORDS = PANDA_SCENE_ROW_WORDS;
    static constexpr Scene m3_handle::*SINGLE = &m3_handle::panda_scene;
    static constexpr SceneRows<Scene> m3_handle::*ROWS = &m3_handle::panda_rows;
    static constexpr const char* SET_SCENE = "m3_set_panda_scene";
    static constexpr const char* SET_ENV_ROWS = "m3_set_panda_scene_rows";
    static constexpr const char* SET_SAMPLE_ROWS = "m3_set_panda_rollout_scenes";
    static constexpr const char* PLANNER_HINT = "the samples of a planner's rollout: m3_set_panda_rollout_scenes";
    static std::string fault(const Scene& sc) { return panda_scene_fault(sc); }
    static void rebuild(m3_handle* h) { build_panda_scenes(h->cfg, h->panda_scene, h->pscene, h->pscene_rt); }
    static void pack_row(const m3_config& c, const Scene& sc, float* table, int Kl, int i) {
        panda_scene_row_pack(make_panda_scene_rt(sc, c.dt, c.substeps), table, Kl, i);
    }
};

template <class Kind> static void default_scene(typename Kind::Scene* sc) {
    if (sc) std::memcpy(sc, &Kind::DEFAULT, sizeof(*sc));
}

template <class Kind> static int set_scene(m3_handle* h, const typename Kind::Scene* sc) {
    if (!h) return M3_ERR_BAD_ARG;
    const std::string who = Kind::SET_SCENE;
    if (h->cfg.env_type != Kind::ENV) return fail(h, M3_ERR_UNSUPPORTED, (who + env_only_text(Kind::ENV)).c_str());
    const typename Kind::Scene& src = sc ? *sc : Kind::DEFAULT;
    const std::string fault = Kind::fault(src);
    if (!fault.empty()) return fail(h, M3_ERR_BAD_ARG, (who + ": " + fault).c_str());
    std::memcpy(&(h->*Kind::SINGLE), &src, sizeof(src));
    Kind::rebuild(h);
    // the last call wins: the handle is on its single scene (the rows' memory is kept for a later call)
    (h->*Kind::ROWS).env_on = (h->*Kind::ROWS).sample_on = false;
    return M3_OK;
}

template <class Kind> static int get_scene(const m3_handle* h, typename Kind::Scene* out) {
    if (!h || !out) return M3_ERR_BAD_ARG;
    if (h->cfg.env_type != Kind::ENV) return M3_ERR_UNSUPPORTED;
    std::memcpy(out, &(h->*Kind::SINGLE), sizeof(*out));
    return M3_OK;
}

// The rows of a handle -- per environment (sim_only) or per sample (planner) -- into its host copy, pinned mirror and device
// table: scenes are Kl checked rows.  THE allocation of both features: the first call of the kind on a handle; later calls
// reuse the three blocks (K_local is fixed at m3_create).  m3_sim_step*, m3_cost, m3_episodes_tick / _begin / _end, m3_rollout
// and m3_command allocate nothing because of the rows -- they read the device table and the handle's scene_rt / pscene_rt,
// nothing else.
template <class Kind>
static int upload_scene_rows(m3_handle* h, const typename Kind::Scene* scenes, const char* who) {
    using Scene = typename Kind::Scene;
    SceneRows<Scene>& r = h->*Kind::ROWS;
    const int Kl = h->cfg.K_local;
    const size_t table_bytes = (size_t)Kind::ROW_WORDS * Kl * sizeof(float);
    if (!r.dev) {
        BlockGroup g(h->mem);   // all three or none
        hipError_t e = own_host(h->mem, r.set, (size_t)Kl * sizeof(Scene));
        if (e == hipSuccess) e = own_pinned(h->mem, r.host, table_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = own_device(h->mem, r.dev, table_bytes);
        if (e != hipSuccess) return fail(h, M3_ERR_HIP, (std::string(who) + ": " + hipGetErrorString(e)).c_str());
        g.keep = true;
    } else {
        // the pinned mirror is the source of the previous call's asynchronous upload: that copy is over before it is rewritten
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    std::memcpy(r.set, scenes, (size_t)Kl * sizeof(Scene));
    for (int i = 0; i < Kl; ++i) Kind::pack_row(h->cfg, scenes[i], r.host, Kl, i);
    HIPCHK(h, hipMemcpyAsync(r.dev, r.host, table_bytes, hipMemcpyHostToDevice, h->stream));
    return M3_OK;
}

// m3_set_*_scene_rows (sim_only handles: one scene per environment) and, per_sample, m3_set_*_rollout_scenes (planner handles:
// one scene per sample of the fused rollout).  Every check before any state changes.
template <class Kind> static int set_scene_rows(m3_handle* h, const typename Kind::Scene* scenes, int n, bool per_sample) {
    if (!h) return M3_ERR_BAD_ARG;
    const std::string who = per_sample ? Kind::SET_SAMPLE_ROWS : Kind::SET_ENV_ROWS;
    bool& on = per_sample ? (h->*Kind::ROWS).sample_on : (h->*Kind::ROWS).env_on;
    if (h->cfg.env_type != Kind::ENV) return fail(h, M3_ERR_UNSUPPORTED, (who + env_only_text(Kind::ENV)).c_str());
    if ((h->cfg.sim_only != 0) == per_sample)
        return fail(h, M3_ERR_STATE, (who + (per_sample ? std::string(": planner handles only (the environments of a sim_only handle: ") + Kind::SET_ENV_ROWS
                                                        : std::string(": sim_only handles only (") + Kind::PLANNER_HINT) + ")").c_str());
    if (!scenes) {   // back on the single scene: exactly the kernels of a handle that never had rows (n is not read)
        on = false;
        return M3_OK;
    }
    const int Kl = h->cfg.K_local;
    if (n != Kl)
        return fail(h, M3_ERR_SHAPE, (who + ": n is " + std::to_string(n) + ", the handle's K_local " + std::to_string(Kl)).c_str());
    for (int i = 0; i < n; ++i) {
        const std::string fault = Kind::fault(scenes[i]);
        if (!fault.empty()) return fail(h, M3_ERR_BAD_ARG, (who + ": row " + std::to_string(i) + ": " + fault).c_str());
    }
    const int rc = upload_scene_rows<Kind>(h, scenes, who.c_str());
    if (rc != M3_OK) return rc;
    on = true;
    return M3_OK;
}
// row `row` as it was set, while the feature (per_sample: which of the two) is on
template <class Kind> static int get_scene_row(const m3_handle* h, int row, typename Kind::Scene* out, bool per_sample) {
    if (!h || !out) return M3_ERR_BAD_ARG;
    if (h->cfg.env_type != Kind::ENV) return M3_ERR_UNSUPPORTED;
    const SceneRows<typename Kind::Scene>& r = h->*Kind::ROWS;
    if (!(per_sample ? r.sample_on : r.env_on)) return M3_ERR_STATE;
    if (row < 0 || row >= h->cfg.K_local) return M3_ERR_BAD_ARG;
    std::memcpy(out, &r.set[row], sizeof(*out));
    return M3_OK;
}

extern "C" void m3_default_point_scene(m3_point_scene* sc) { default_scene<PointSceneKind>(sc); }
extern "C" int m3_set_point_scene(m3_handle* h, const m3_point_scene* sc) { return set_scene<PointSceneKind>(h, sc); }
extern "C" int m3_get_point_scene(const m3_handle* h, m3_point_scene* out) { return get_scene<PointSceneKind>(h, out); }
extern "C" int m3_set_point_scene_rows(m3_handle* h, const m3_point_scene* scenes, int n) { return set_scene_rows<PointSceneKind>(h, scenes, n, false); }
extern "C" int m3_get_point_scene_row(const m3_handle* h, int row, m3_point_scene* out) { return get_scene_row<PointSceneKind>(h, row, out, false); }
extern "C" int m3_point_scene_rows_set(const m3_handle* h) { return h ? (h->point_rows.env_on ? 1 : 0) : M3_ERR_BAD_ARG; }
extern "C" int m3_set_point_rollout_scenes(m3_handle* h, const m3_point_scene* scenes, int n) { return set_scene_rows<PointSceneKind>(h, scenes, n, true); }
extern "C" int m3_get_point_rollout_scene(const m3_handle* h, int row, m3_point_scene* out) { return get_scene_row<PointSceneKind>(h, row, out, true); }
extern "C" int m3_point_rollout_scenes_set(const m3_handle* h) { return h ? (h->point_rows.sample_on ? 1 : 0) : M3_ERR_BAD_ARG; }
extern "C" int m3_set_point_scene_instance(m3_handle* h, int on) {
    return set_instance(h, M3_ENV_POINT, &m3_handle::scene_instance, on, "m3_set_point_scene_instance", "values");
}

extern "C" void m3_default_panda_scene(m3_panda_scene* sc) { default_scene<PandaSceneKind>(sc); }
extern "C" int m3_set_panda_scene(m3_handle* h, const m3_panda_scene* sc) { return set_scene<PandaSceneKind>(h, sc); }
extern "C" int m3_get_panda_scene(const m3_handle* h, m3_panda_scene* out) { return get_scene<PandaSceneKind>(h, out); }
extern "C" int m3_set_panda_scene_rows(m3_handle* h, const m3_panda_scene* scenes, int n) { return set_scene_rows<PandaSceneKind>(h, scenes, n, false); }
extern "C" int m3_get_panda_scene_row(const m3_handle* h, int row, m3_panda_scene* out) { return get_scene_row<PandaSceneKind>(h, row, out, false); }
extern "C" int m3_panda_scene_rows_set(const m3_handle* h) { return h ? (h->panda_rows.env_on ? 1 : 0) : M3_ERR_BAD_ARG; }
extern "C" int m3_set_panda_rollout_scenes(m3_handle* h, const m3_panda_scene* scenes, int n) { return set_scene_rows<PandaSceneKind>(h, scenes, n, true); }
extern "C" int m3_get_panda_rollout_scene(const m3_handle* h, int row, m3_panda_scene* out) { return get_scene_row<PandaSceneKind>(h, row, out, true); }
extern "C" int m3_panda_rollout_scenes_set(const m3_handle* h) { return h ? (h->panda_rows.sample_on ? 1 : 0) : M3_ERR_BAD_ARG; }
extern "C" int m3_set_panda_scene_instance(m3_handle* h, int on) {
    return set_instance(h, M3_ENV_PANDA, &m3_handle::panda_scene_instance, on, "m3_set_panda_scene_instance", "values");
}

// ---- prior samples (extension, planner handles, unsharded): samples of the fused rollout that take the caller's control
// sequences.  THE allocation of the feature is the first setter call on a handle; m3_rollout and m3_command read the two
// device blocks, nothing else.  Every check before any state changes.  One implementation for both environments (point_env:
// m3_set_prior_samples, nu = 2; panda_env: m3_set_panda_prior_samples, nu = 9): a PriorKind names the environment, the
// handle's state of that kind and the entry points' names; nu is the handle's ----
struct PriorKind {
    int env;
    PriorSampleState m3_handle::*state;
    const char* setter;          // the host entry point; the device one is setter + "_device"
};
static const PriorKind PRIOR_KIND_POINT = {M3_ENV_POINT, &m3_handle::priors, "m3_set_prior_samples"};
static const PriorKind PRIOR_KIND_PANDA = {M3_ENV_PANDA, &m3_handle::panda_priors, "m3_set_panda_prior_samples"};
// the checks on the handle ...
static int prior_handle_check(m3_handle* h, const std::string& who, int env = M3_ENV_POINT) {
    const m3_config& c = h->cfg;
    if (c.env_type != env) return fail(h, M3_ERR_UNSUPPORTED, (who + env_only_text(env)).c_str());
    if (c.sim_only) return fail(h, M3_ERR_STATE, (who + ": planner handles only (the handle was created sim_only)").c_str());
    if (c.K_local != c.K_global) return fail(h, M3_ERR_UNSUPPORTED, (who + ": sharded handle (K_local != K_global)").c_str());
    return M3_OK;
}
// ... and on the n sample indices
static int prior_index_check(m3_handle* h, const std::string& who, const int* sample_idx, int n) {
    const m3_config& c = h->cfg;
    if (!sample_idx) return fail(h, M3_ERR_BAD_ARG, (who + ": null sample_idx").c_str());
    const int K = c.K_global;
    for (int j = 0; j < n; ++j) {
        const int k = sample_idx[j];
        const std::string at = who + ": prior " + std::to_string(j) + ": sample " + std::to_string(k);
        if (k < 0 || k >= K) return fail(h, M3_ERR_BAD_ARG, (at + " is outside 0 .. K_global - 1 = " + std::to_string(K - 1)).c_str());
        if (k == K - 1) return fail(h, M3_ERR_BAD_ARG, (at + " is the zero-noise / null-action sample K_global - 1").c_str());
        if (c.multi_modal && (k == 0 || k == K / 2))
            return fail(h, M3_ERR_BAD_ARG, (at + " is a best-trajectory sample of the multi-modal planner (0 and K/2)").c_str());
        for (int q = 0; q < j; ++q)
            if (sample_idx[q] == k) return fail(h, M3_ERR_BAD_ARG, (at + " listed twice").c_str());
    }
    return M3_OK;
}
// The blocks of the feature (allocated by the first call on the handle, as one group) and the slot map of these n indices on
// the device.  Leaves the pinned mirror free to be rewritten: the previous call's uploads from it are over.
static int prior_blocks_and_slots(m3_handle* h, const std::string& who, const int* sample_idx, int n,
                                  const PriorKind& kind = PRIOR_KIND_POINT) {
    const m3_config& c = h->cfg;
    PriorSampleState& ps = h->*kind.state;
    const int Kl = c.K_local, T = c.T, nu = c.nu;
    const size_t tab_bytes = (size_t)M3_MAX_PRIOR_SAMPLES * T * nu * sizeof(float), slot_bytes = (size_t)Kl * sizeof(int);
    bool slots_stale = false;
    if (!ps.tab_dev) {
        BlockGroup g(h->mem);   // all or none
        hipError_t e = own_device(h->mem, ps.tab_dev, tab_bytes);
        if (e == hipSuccess) e = own_device(h->mem, ps.slot_dev, slot_bytes);
        if (e == hipSuccess) e = own_pinned(h->mem, ps.pinned, tab_bytes + slot_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = own_event(h->mem, ps.uploaded, hipEventDisableTiming);
        if (e != hipSuccess) return fail(h, M3_ERR_HIP, (who + ": " + hipGetErrorString(e)).c_str());
        g.keep = true;
        int* slot = reinterpret_cast<int*>(ps.pinned + (size_t)M3_MAX_PRIOR_SAMPLES * T * nu);
        for (int i = 0; i < Kl; ++i) slot[i] = -1;
        ps.dev_n = 0;
        slots_stale = true;
    } else if (ps.upload_pending) {
        // the pinned mirror is the source of the previous call's asynchronous uploads: those copies, and only those, are over
        // before it is rewritten
        HIPCHK(h, hipEventSynchronize(ps.uploaded));
        ps.upload_pending = false;
    }
    int* slot = reinterpret_cast<int*>(ps.pinned + (size_t)M3_MAX_PRIOR_SAMPLES * T * nu);
    if (slots_stale || ps.dev_n != n || std::memcmp(ps.idx, sample_idx, (size_t)n * sizeof(int)) != 0) {
        for (int j = 0; j < ps.dev_n; ++j) slot[ps.idx[j] - c.k_offset] = -1;
        for (int j = 0; j < n; ++j) slot[sample_idx[j] - c.k_offset] = j;
        std::memcpy(ps.idx, sample_idx, (size_t)n * sizeof(int));
        ps.dev_n = n;
        HIPCHK(h, hipMemcpyAsync(ps.slot_dev, slot, slot_bytes, hipMemcpyHostToDevice, h->stream));
    }
    return M3_OK;
}
static int set_prior_samples(m3_handle* h, const PriorKind& kind, const float* seqs, const int* sample_idx, int n, bool device) {
    if (!h) return M3_ERR_BAD_ARG;
    const std::string who = std::string(kind.setter) + (device ? "_device" : "");
    const m3_config& c = h->cfg;
    int rc = prior_handle_check(h, who, kind.env);
    if (rc != M3_OK) return rc;
    if (n < 0 || n > M3_MAX_PRIOR_SAMPLES)
        return fail(h, M3_ERR_BAD_ARG, (who + ": n is " + std::to_string(n) + ", must be in 0 .. " + std::to_string(M3_MAX_PRIOR_SAMPLES)).c_str());
    PriorSampleState& ps = h->*kind.state;
    if (!seqs || n == 0) {   // exactly the kernels of a handle that never had priors (the blocks are kept for a later call)
        ps.n = 0;
        ps.ctl.kind = 0;
        return M3_OK;
    }
    if (h->groups.n > 0) return fail(h, M3_ERR_UNSUPPORTED, (who + SAMPLE_GROUPS_REFUSE_PRIORS).c_str());
    if ((rc = prior_index_check(h, who, sample_idx, n)) != M3_OK) return rc;
    const int T = c.T, nu = c.nu;
    if (!device)
        for (int j = 0; j < n; ++j)
            for (int t = 0; t < T; ++t)
                for (int u = 0; u < nu; ++u)
                    if (!std::isfinite(seqs[((size_t)j * T + t) * nu + u]))
                        return fail(h, M3_ERR_BAD_ARG, (who + ": prior " + std::to_string(j) + ": step " + std::to_string(t) + " control " +
                                                        std::to_string(u) + " is not finite").c_str());
    if ((rc = prior_blocks_and_slots(h, who, sample_idx, n, kind)) != M3_OK) return rc;
    const size_t bytes = (size_t)n * T * nu * sizeof(float);
    if (device) {
        HIPCHK(h, hipMemcpyAsync(ps.tab_dev, seqs, bytes, hipMemcpyDeviceToDevice, h->stream));
    } else {
        std::memcpy(ps.pinned, seqs, bytes);
        HIPCHK(h, hipMemcpyAsync(ps.tab_dev, ps.pinned, bytes, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipEventRecord(ps.uploaded, h->stream));
    ps.upload_pending = true;
    ps.host_values = !device;
    ps.n = n;
    ps.ctl.kind = 0;   // (against m3_set_prior_controller the last call wins: the table is the caller's again)
    return M3_OK;
}
static int get_prior_sample(const m3_handle* h, const PriorKind& kind, int j, int* sample_idx, float* seq) {
    if (!h) return M3_ERR_BAD_ARG;
    if (h->cfg.env_type != kind.env) return M3_ERR_UNSUPPORTED;
    const PriorSampleState& ps = h->*kind.state;
    if (j < 0 || j >= ps.n) return M3_ERR_BAD_ARG;
    if (seq && !ps.host_values) return M3_ERR_STATE;
    if (sample_idx) *sample_idx = ps.idx[j];
    const size_t row = (size_t)h->cfg.T * h->cfg.nu;
    if (seq) std::memcpy(seq, ps.pinned + (size_t)j * row, row * sizeof(float));
    return M3_OK;
}
extern "C" int m3_set_prior_samples(m3_handle* h, const float* seqs, const int* sample_idx, int n) {
    return set_prior_samples(h, PRIOR_KIND_POINT, seqs, sample_idx, n, false);
}
extern "C" int m3_set_prior_samples_device(m3_handle* h, const float* seqs_dev, const int* sample_idx, int n) {
    return set_prior_samples(h, PRIOR_KIND_POINT, seqs_dev, sample_idx, n, true);
}
extern "C" int m3_prior_samples_set(const m3_handle* h) { return h ? h->priors.n : M3_ERR_BAD_ARG; }
extern "C" int m3_get_prior_sample(const m3_handle* h, int j, int* sample_idx, float* seq) {
    return get_prior_sample(h, PRIOR_KIND_POINT, j, sample_idx, seq);
}
extern "C" int m3_prior_samples_used(m3_handle* h) { return h ? h->priors.used : M3_ERR_BAD_ARG; }
// (panda_env: the same five)
extern "C" int m3_set_panda_prior_samples(m3_handle* h, const float* seqs, const int* sample_idx, int n) {
    return set_prior_samples(h, PRIOR_KIND_PANDA, seqs, sample_idx, n, false);
}
extern "C" int m3_set_panda_prior_samples_device(m3_handle* h, const float* seqs_dev, const int* sample_idx, int n) {
    return set_prior_samples(h, PRIOR_KIND_PANDA, seqs_dev, sample_idx, n, true);
}
extern "C" int m3_panda_prior_samples_set(const m3_handle* h) { return h ? h->panda_priors.n : M3_ERR_BAD_ARG; }
extern "C" int m3_get_panda_prior_sample(const m3_handle* h, int j, int* sample_idx, float* seq) {
    return get_prior_sample(h, PRIOR_KIND_PANDA, j, sample_idx, seq);
}
extern "C" int m3_panda_prior_samples_used(m3_handle* h) { return h ? h->panda_priors.used : M3_ERR_BAD_ARG; }

// ---- a prior controller (extension, m3p2i_hip_ext.h): the library fills the table, on the device, ahead of every rollout ----
extern "C" void m3_default_prior_controller(m3_prior_controller* pc, int kind, int n) {
    if (!pc) return;
    std::memset(pc, 0, sizeof(*pc));
    n = std::min(std::max(n, 1), M3_MAX_PRIOR_CONTROLLER_SEQS);
    pc->kind = kind;
    pc->n = n;
    for (int j = 0; j < n; ++j) pc->speed[j] = 1.0f - (float)j / (float)n;
    pc->standoff = 0.45f;
    pc->reach = 0.05f;
}
extern "C" int m3_set_prior_controller(m3_handle* h, const m3_prior_controller* pc, const int* sample_idx) {
    if (!h) return M3_ERR_BAD_ARG;
    const std::string who = "m3_set_prior_controller";
    int rc = prior_handle_check(h, who);
    if (rc != M3_OK) return rc;
    PriorSampleState& ps = h->priors;
    if (!pc) {   // exactly the kernels of a handle that never had priors (the blocks are kept for a later call)
        ps.n = 0;
        ps.ctl.kind = 0;
        return M3_OK;
    }
    if (h->groups.n > 0) return fail(h, M3_ERR_UNSUPPORTED, (who + SAMPLE_GROUPS_REFUSE_PRIORS).c_str());
    if (pc->kind != M3_PRIOR_CONTROLLER_GO_TO && pc->kind != M3_PRIOR_CONTROLLER_PUSH_BEHIND)
        return fail(h, M3_ERR_BAD_ARG, (who + ": unknown kind " + std::to_string(pc->kind) + " (M3_PRIOR_CONTROLLER_GO_TO = 1, _PUSH_BEHIND = 2)").c_str());
    if (pc->n < 1 || pc->n > M3_MAX_PRIOR_CONTROLLER_SEQS)
        return fail(h, M3_ERR_BAD_ARG, (who + ": n is " + std::to_string(pc->n) + ", must be in 1 .. " + std::to_string(M3_MAX_PRIOR_CONTROLLER_SEQS)).c_str());
    const auto positive = [](float v) { return std::isfinite(v) && v > 0.0f; };
    for (int j = 0; j < pc->n; ++j)
        if (!positive(pc->speed[j]))
            return fail(h, M3_ERR_BAD_ARG, (who + ": speed factor " + std::to_string(j) + " is not a finite positive number").c_str());
    if (!positive(pc->standoff)) return fail(h, M3_ERR_BAD_ARG, (who + ": standoff is not a finite positive number").c_str());
    if (!positive(pc->reach)) return fail(h, M3_ERR_BAD_ARG, (who + ": reach is not a finite positive number").c_str());
    if ((rc = prior_index_check(h, who, sample_idx, pc->n)) != M3_OK) return rc;
    if ((rc = prior_blocks_and_slots(h, who, sample_idx, pc->n)) != M3_OK) return rc;
    HIPCHK(h, hipEventRecord(ps.uploaded, h->stream));   // (behind the slot map's copy, if there was one)
    ps.upload_pending = true;
    ps.host_values = false;
    ps.n = pc->n;
    ps.ctl = *pc;
    for (int j = pc->n; j < M3_MAX_PRIOR_CONTROLLER_SEQS; ++j) ps.ctl.speed[j] = 0.0f;   // (what the getter returns is defined)
    return M3_OK;
}
extern "C" int m3_get_prior_controller(const m3_handle* h, m3_prior_controller* out) {
    if (!h || !out) return M3_ERR_BAD_ARG;
    if (h->cfg.env_type != M3_ENV_POINT) return M3_ERR_UNSUPPORTED;
    std::memset(out, 0, sizeof(*out));
    if (h->priors.n > 0 && h->priors.ctl.kind != 0) *out = h->priors.ctl;
    return M3_OK;
}
extern "C" int m3_prior_table(const m3_handle* h, const float** tab_dev, int* n) {
    if (!h) return M3_ERR_BAD_ARG;
    if (h->cfg.env_type != M3_ENV_POINT) return M3_ERR_UNSUPPORTED;
    if (!h->priors.tab_dev) return M3_ERR_STATE;
    if (tab_dev) *tab_dev = h->priors.tab_dev;
    if (n) *n = h->priors.n;
    return M3_OK;
}
// the handle has a controller that the next rollout runs
static bool prior_controller_on(const m3_handle* h) { return h->priors.n > 0 && h->priors.ctl.kind != 0; }
static PriorControllerArgs prior_controller_args(const m3_handle* h) { return {h->priors.ctl, h->cfg.dt, h->priors.tab_dev}; }

// ---- sample groups (m3_set_sample_groups): sample_groups.hpp validates, builds the table and owns the
// refusals; here: the reading of the handle, the blocks, the upload and the launch ----
static SampleGroupsInput sample_groups_input(const m3_handle* h) {
    const m3_config& c = h->cfg;
    return {c.K_local, c.K_global, c.multi_modal != 0, c.mode_simple != 0, c.sampling_random != 0, c.sim_only != 0,
            h->priors.n > 0 || h->panda_priors.n > 0};
}
extern "C" int m3_set_sample_groups(m3_handle* h, const int* group_of, int n, float worst_frac) {
    if (!h) return M3_ERR_BAD_ARG;
    SampleGroupState& sg = h->groups;
    if (!group_of) {   // exactly the kernels of a handle that never had groups (the blocks are kept for a later call)
        sg.n = 0;
        sg.n_ungrouped = 0;
        return M3_OK;
    }
    // ---- every check, and the table, before any state changes ----
    const SampleGroupsInput in = sample_groups_input(h);
    SampleGroupTable t;
    try {
        const SampleGroupFault f = sample_groups_build(in, group_of, n, worst_frac, t);
        if (f.r != SAMPLE_GROUPS_OK)
            return fail(h, sample_groups_refusal_is_unsupported(f.r) ? M3_ERR_UNSUPPORTED : M3_ERR_BAD_ARG, sample_groups_refusal_text(f, in).c_str());
    } catch (const std::bad_alloc&) {
        return fail(h, M3_ERR_HIP, "m3_set_sample_groups: out of host memory");
    }
    const int K = in.K_local, cap = K / 2;
    const size_t tab_ints = sample_group_table_ints(K);
    if (!sg.tab_dev) {
        BlockGroup g(h->mem);   // all or none
        hipError_t e = own_device(h->mem, sg.tab_dev, tab_ints * sizeof(int));
        if (e == hipSuccess) e = own_device(h->mem, sg.raw_dev, (size_t)K * sizeof(float));
        if (e == hipSuccess) e = own_pinned(h->mem, sg.pinned, (tab_ints + 2 * (size_t)K) * sizeof(int), hipHostMallocDefault);
        if (e == hipSuccess) e = hipMemsetAsync(sg.raw_dev, 0, (size_t)K * sizeof(float), h->stream);
        if (e != hipSuccess) return fail(h, M3_ERR_HIP, (std::string("m3_set_sample_groups: ") + hipGetErrorString(e)).c_str());
        g.keep = true;
    }
    // (the pinned mirror is free to be rewritten: every call that uploads from it ends with a synchronisation)
    int* p = sg.pinned;
    for (size_t i = 0; i < tab_ints; ++i) p[i] = -1;
    std::memcpy(p, t.member.data(), t.member.size() * sizeof(int));
    std::memcpy(p + (size_t)cap * SAMPLE_GROUP_LANES, t.worst_j.data(), t.worst_j.size() * sizeof(int));
    if (t.n_ungrouped) std::memcpy(p + (size_t)cap * (SAMPLE_GROUP_LANES + 1), t.ungrouped.data(), t.ungrouped.size() * sizeof(int));
    std::memcpy(p + tab_ints, group_of, (size_t)K * sizeof(int));
    std::memcpy(p + tab_ints + K, t.dense.data(), (size_t)K * sizeof(int));
    sg.n = 0;   // (a failed upload leaves the handle without groups, not with half a table)
    HIPCHK(h, hipMemcpyAsync(sg.tab_dev, p, tab_ints * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    sg.n = t.n_groups;
    sg.n_ungrouped = t.n_ungrouped;
    sg.worst_frac = worst_frac;
    return M3_OK;
}
extern "C" int m3_sample_groups_set(m3_handle* h) { return h ? h->groups.n : M3_ERR_BAD_ARG; }
extern "C" int m3_get_sample_group(const m3_handle* h, int k, int* group, int* size, int* worst_j) {
    if (!h) return M3_ERR_BAD_ARG;
    const int K = h->cfg.K_local;
    if (k < 0 || k >= K) return M3_ERR_BAD_ARG;
    const SampleGroupState& sg = h->groups;
    int id = -1, m = 1, j = 1;
    if (sg.n > 0) {
        const size_t tab_ints = sample_group_table_ints(K);
        const int row = sg.pinned[tab_ints + K + k];
        if (row >= 0) {
            id = sg.pinned[tab_ints + k];
            m = 0;
            for (int l = 0; l < SAMPLE_GROUP_LANES; ++l) m += sg.pinned[(size_t)row * SAMPLE_GROUP_LANES + l] >= 0;
            j = sg.pinned[(size_t)(K / 2) * SAMPLE_GROUP_LANES + row];
        }
    }
    if (group) *group = id;
    if (size) *size = m;
    if (worst_j) *worst_j = j;
    return M3_OK;
}
extern "C" int m3_sample_group_raw_costs(m3_handle* h, const float** dev) {
    if (!h || !dev) return M3_ERR_BAD_ARG;
    if (!h->groups.raw_dev) return fail(h, M3_ERR_STATE, "m3_sample_group_raw_costs: the handle never had sample groups (m3_set_sample_groups)");
    *dev = h->groups.raw_dev;
    return M3_OK;
}
// the launch at the tail of a rollout (and m3_aggregate_sample_groups'): behind the last writer of M3_BUF_TRAJ_COST on the stream
static void aggregate_sample_groups(m3_handle* h) {
    const SampleGroupState& sg = h->groups;
    launch_sample_groups({sg.tab_dev, sg.n, sg.n_ungrouped, h->cfg.K_local / 2, h->cfg.K_local, (float*)h->buf[M3_BUF_TRAJ_COST], sg.raw_dev},
                         h->stream);
}
extern "C" int m3_aggregate_sample_groups(m3_handle* h) {
    if (!h) return M3_ERR_BAD_ARG;
    if (h->groups.n <= 0) return fail(h, M3_ERR_STATE, "m3_aggregate_sample_groups: the handle has no sample groups (m3_set_sample_groups)");
    aggregate_sample_groups(h);
    HIPCHK(h, hipGetLastError());
    return M3_OK;
}

// the handle's arena is the default bit for bit (-0.0f is not 0.0f here)
static bool default_point_scene(const m3_handle* h) {
    return std::memcmp(&h->point_scene, &POINT_SCENE_DEFAULT, sizeof(m3_point_scene)) == 0;
}

// ---- which point_env kernels a handle runs: decided here and nowhere else ----
// what a caller is about to launch: the step-mode cost reads the weights only, the step and the episode tick the arena only,
// a rollout both
enum PointSide { SIDE_COST = 1, SIDE_STEP = 2, SIDE_ROLLOUT = SIDE_COST | SIDE_STEP };
// the variant of the rollout kernels (SIDE_ROLLOUT: m3_rollout, m3_batch_command) or of the step-mode cost (SIDE_COST: the
// arena is no input of the cost, so never POINT_SCENE)
static PointVariant point_variant(const m3_handle* h, PointSide side) {
    if (h->cfg.env_type != M3_ENV_POINT) return POINT_PLAIN;
    // (per-sample arenas are the run-time-scene variant of the rollout; a planner handle's own step keeps its single scene)
    // (... and so is the prior build, m3_set_prior_samples)
    const bool rows = side == SIDE_ROLLOUT && (h->point_rows.sample_on || h->priors.n > 0);
    if ((side & SIDE_STEP) && (h->scene_instance < 0 ? (rows || !default_point_scene(h)) : h->scene_instance != 0)) return POINT_SCENE;
    return (h->weighted_instance < 0 ? !default_cost_weights(h) : h->weighted_instance != 0) ? POINT_WEIGHTED : POINT_PLAIN;
}
// the variant of the step-mode kernels (m3_sim_step, the episode tick): the arena compiled in, the handle's arena a kernel
// argument (m3_set_point_scene), or one arena per environment (m3_set_point_scene_rows)
enum PointStepVariant { STEP_COMPILED, STEP_RUNTIME, STEP_ROWS };
static PointStepVariant point_step_variant(const m3_handle* h) {
    if (h->point_rows.env_on) return STEP_ROWS;
    return point_variant(h, SIDE_STEP) == POINT_SCENE ? STEP_RUNTIME : STEP_COMPILED;
}
// why the handle cannot run that side's kernels (M3_ERR_STATE; nullptr: it can)
static const char* point_variant_refusal(const m3_handle* h, PointSide side) {
    if (h->cfg.env_type != M3_ENV_POINT) return nullptr;
    if ((side & SIDE_COST) && h->weighted_instance == 0 && !default_cost_weights(h))
        return "the weighted cost instance is forced off (m3_set_weighted_cost_instance 0) but the handle's cost weights are not the defaults";
    if ((side & SIDE_STEP) && h->scene_instance == 0 && h->point_rows.env_on)
        return "the run-time-scene instance is forced off (m3_set_point_scene_instance 0) but the handle has an arena per environment (m3_set_point_scene_rows)";
    if (side == SIDE_ROLLOUT && h->scene_instance == 0 && h->point_rows.sample_on)
        return "the run-time-scene instance is forced off (m3_set_point_scene_instance 0) but the handle has an arena per sample (m3_set_point_rollout_scenes)";
    if (side == SIDE_ROLLOUT && h->scene_instance == 0 && h->priors.n > 0)
        return "the run-time-scene instance is forced off (m3_set_point_scene_instance 0) but the handle has prior samples (m3_set_prior_samples)";
    if ((side & SIDE_STEP) && h->scene_instance == 0 && !default_point_scene(h))
        return "the run-time-scene instance is forced off (m3_set_point_scene_instance 0) but the handle's scene is not the default";
    return nullptr;
}

extern "C" int m3_panda_scene_instance_used(m3_handle* h) { return h ? h->panda_scene_used : M3_ERR_BAD_ARG; }

extern "C" int m3_panda_weighted_cost_instance_used(m3_handle* h) { return h ? h->panda_weighted_used : M3_ERR_BAD_ARG; }

// ---- which panda_env kernels a handle runs, what the launch records, why a path refuses the handle: panda_variant.hpp decides,
// from this reading of the handle.  Here: the reading, the texts and what a launcher receives ----
static PandaVariantInput panda_input(const m3_handle* h) {
    PandaVariantInput in;
    in.scene_instance = h->panda_scene_instance;
    in.weighted_instance = h->panda_weighted_instance;
    in.geometry_default = panda_scene_geometry_is_default(h->panda_scene);   // (anything but the two masses off the defaults)
    // (bit for bit: -0.0f is not 0.0f here, the kernels multiply by them)
    in.weights_default = std::memcmp(&h->panda_cost_weights, &PANDA_COST_WEIGHTS_DEFAULT, sizeof(PandaCostWeights)) == 0;
    in.rollout_scenes_on = h->panda_rows.sample_on;
    in.scene_rows_on = h->panda_rows.env_on;
    in.sim_only = h->cfg.sim_only != 0;
    in.priors_on = h->panda_priors.n > 0;
    return in;
}
static const char* panda_refusal_text(PandaRefusal r) {
    switch (r) {
        case PANDA_REFUSAL_NONE: return nullptr;
        case PANDA_SCENE_OFF_ENV_ROWS:
            return "the run-time-scene instance is forced off (m3_set_panda_scene_instance 0) but the handle has a workspace per environment (m3_set_panda_scene_rows)";
        case PANDA_SCENE_OFF_SAMPLE_ROWS:
            return "the run-time-scene instance is forced off (m3_set_panda_scene_instance 0) but the handle has a workspace per sample (m3_set_panda_rollout_scenes)";
        case PANDA_SCENE_OFF_GEOMETRY:
            return "the run-time-scene instance is forced off (m3_set_panda_scene_instance 0) but the handle's workspace (m3_set_panda_scene) is not the default";
        case PANDA_WEIGHTS_OFF_TUNED:
            return "the weighted cost instance is forced off (m3_set_panda_weighted_cost_instance 0) but the handle's cost weights (m3_set_panda_cost_weights) are not the defaults";
        case PANDA_UNBATCHED_SCENE:
            return "its workspace (m3_set_panda_scene) needs the run-time-scene instance, which only m3_rollout / "
                   "m3_command and the handle's own step, cost and views run";
        case PANDA_UNBATCHED_SAMPLE_ROWS:
            return "it has a workspace per sample (m3_set_panda_rollout_scenes), which only m3_rollout / m3_command run";
        case PANDA_UNBATCHED_ENV_ROWS:
            return "it has a workspace per environment (m3_set_panda_scene_rows), which only the handle's own step, cost and views run";
        case PANDA_UNBATCHED_WEIGHTS:
            return "its cost weights (m3_set_panda_cost_weights) need the weighted cost instance, which only m3_rollout / "
                   "m3_command and the handle's own m3_cost run";
        case PANDA_SCENE_OFF_PRIORS:
            return "the run-time-scene instance is forced off (m3_set_panda_scene_instance 0) but the handle has prior samples (m3_set_panda_prior_samples)";
        case PANDA_WEIGHTS_OFF_PRIORS:
            return "the weighted cost instance is forced off (m3_set_panda_weighted_cost_instance 0) but the handle has prior samples (m3_set_panda_prior_samples)";
        case PANDA_UNBATCHED_PRIORS:
            return "it has prior samples (m3_set_panda_prior_samples), which only m3_rollout / m3_command run";
    }
    return nullptr;
}
// why the handle cannot run its own kernels on a side (M3_ERR_STATE; nullptr: it can, or it is no panda_env handle)
static const char* panda_refusal(const m3_handle* h, PandaSide side) {
    return h->cfg.env_type == M3_ENV_PANDA ? panda_refusal_text(panda_refusal(panda_input(h), side)) : nullptr;
}
// why a path that carries a PandaScene and forms the literal cost only (a batch table without the run-time section, the lockstep
// episodes' kernels) cannot take the handle (M3_ERR_UNSUPPORTED; nullptr as above)
static const char* panda_unbatched(const m3_handle* h, PandaUnbatchedOrder order) {
    return h->cfg.env_type == M3_ENV_PANDA ? panda_refusal_text(panda_unbatched(panda_input(h), order)) : nullptr;
}
// why a lockstep episode set of that mode cannot take the handle, the world or a planner (code: M3_ERR_STATE for what the
// handle's own kernels refuse, M3_ERR_UNSUPPORTED for what only the literal mode cannot carry; nullptr as above)
static const char* panda_episodes_refusal(const m3_handle* h, PandaEpisodesMode mode, PandaUnbatchedOrder order, int& code) {
    if (h->cfg.env_type != M3_ENV_PANDA) return nullptr;
    const PandaRefusal r = panda_episodes_refusal(panda_input(h), mode, order);
    code = panda_refusal_is_state(r) ? M3_ERR_STATE : M3_ERR_UNSUPPORTED;
    return panda_refusal_text(r);
}
// a launcher's view of the handle for a variant, and the record of what an accepted call launches
static PandaLaunchScene panda_launch_scene(const m3_handle* h, PandaVariant v) {
    PandaLaunchScene sc = {v, &h->pscene, &h->pscene_rt, &h->panda_cost_weights, h->panda_rows.dev};
    if (v == PANDA_PRIORS) {   // (one family with and without a workspace per sample: null rows say "the handle's scene")
        if (!h->panda_rows.sample_on) sc.rows = nullptr;
        sc.prior_slot = h->panda_priors.slot_dev;
        sc.prior_tab = h->panda_priors.tab_dev;
    }
    return sc;
}
static void panda_record_used(m3_handle* h, const PandaDecision& d) {
    if (d.scene_used != PANDA_USED_UNCHANGED) h->panda_scene_used = d.scene_used;
    if (d.weighted_used != PANDA_USED_UNCHANGED) h->panda_weighted_used = d.weighted_used;
}

extern "C" int m3_set_multi_modal(m3_handle* h, int mm) {
    if (!h) return M3_ERR_BAD_ARG;
    if (!h->cfg.sim_only && (mm != 0) != (h->cfg.multi_modal != 0))
        return fail(h, M3_ERR_STATE, "m3_set_multi_modal: fixed at m3_create for planner handles");
    h->cfg.multi_modal = mm != 0;
    return M3_OK;
}

extern "C" int m3_set_plan(m3_handle* h, int which, const float* v) {
    if (!h || !v) return M3_ERR_BAD_ARG;
    if (which < M3_BUF_MEAN || which > M3_BUF_BEST_2) return fail(h, M3_ERR_BAD_ARG, "m3_set_plan: not a plan buffer");
    HIPCHK(h, hipMemcpyAsync(h->buf[which], v, (size_t)h->cfg.T * h->cfg.nu * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return M3_OK;
}

extern "C" int m3_set_beta(m3_handle* h, float beta) {
    if (!h) return M3_ERR_BAD_ARG;
    if (!(beta > 0.0f)) return fail(h, M3_ERR_BAD_ARG, "m3_set_beta: beta must be > 0");
    HIPCHK(h, hipMemcpyAsync((char*)h->buf[M3_BUF_INFO] + offsetof(m3_info, beta), &beta, sizeof(float),
                             hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // `beta` is a stack value
    return M3_OK;
}

extern "C" int m3_set_call_count(m3_handle* h, unsigned calls) {
    if (!h) return M3_ERR_BAD_ARG;
    h->calls = calls;
    // (a rollout still in flight may be about to report into the word zeroed below)
    if (h->panda_busy_hint) HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->panda_busy_hint) { *h->panda_busy_hint = 0; h->panda_reach_busy = 0; }
    return M3_OK;
}

extern "C" int m3_set_action_out(m3_handle* h, float* dev_ptr) {
    if (!h) return M3_ERR_BAD_ARG;
    if (h->cfg.sim_only) return fail(h, M3_ERR_STATE, "m3_set_action_out: handle was created sim_only");
    h->action_out = dev_ptr;
    return M3_OK;
}

extern "C" int m3_reset(m3_handle* h) {
    if (!h) return M3_ERR_BAD_ARG;
    for (int id = M3_BUF_MEAN; id <= M3_BUF_ACTION_OUT; ++id)
        HIPCHK(h, hipMemsetAsync(h->buf[id], 0, (size_t)h->nbytes[id], h->stream));
    HIPCHK(h, hipMemsetAsync(h->buf[M3_BUF_PENDING_FORCE], 0, (size_t)h->nbytes[M3_BUF_PENDING_FORCE], h->stream));
    m3_info init;
    std::memset(&init, 0, sizeof(init));
    init.beta = init.beta_1 = init.beta_2 = 1.0f;
    HIPCHK(h, hipMemcpyAsync(h->buf[M3_BUF_INFO], &init, sizeof(init), hipMemcpyHostToDevice, h->stream));
    // update_cov adapts cov_action / scale_tril (mppi.py:508-516): a reset planner starts from the configured
    // diag(noise_sigma) again, like a freshly built one (mppi.py:175-176)
    float cv[2 * M3_MAX_NU];
    const int nu = h->cfg.nu;
    for (int j = 0; j < nu; ++j) { cv[j] = h->cfg.noise_sigma_diag[j]; cv[nu + j] = std::sqrt(h->cfg.noise_sigma_diag[j]); }
    HIPCHK(h, hipMemcpyAsync(h->buf[M3_BUF_COV], cv, (size_t)(2 * nu) * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->calls = 0;
    if (h->panda_busy_hint) { *h->panda_busy_hint = 0; h->panda_reach_busy = 0; }
    return M3_OK;
}

extern "C" int m3_set_world_point(m3_handle* h, const m3_point_world* w) {
    if (!h || !w) return M3_ERR_BAD_ARG;
    float* o = h->world0;
    o[0] = w->robot[0]; o[1] = w->robot[1]; o[2] = w->robot[2]; o[3] = w->robot[3];
    const float* src[2] = {w->box, w->dyn_obs};
    for (int b = 0; b < 2; ++b) {
        const float* r = src[b];
        float* p = o + 4 + b * 7;
        p[0] = r[0]; p[1] = r[1];
        yaw_from_quat(r[2], r[3], &p[2], &p[3]);  // yaw from the (0,0,qz,qw) quaternion
        p[4] = r[4]; p[5] = r[5]; p[6] = r[6];
    }
    h->world0_bound = nullptr;
    h->bind_dof = nullptr;
    return M3_OK;
}

// internal-format variant used by the parity tests: 18 floats, boxes as (x, y, cos, sin, ...)
extern "C" int m3_set_world_point_raw(m3_handle* h, const float* w18) {
    if (!h || !w18) return M3_ERR_BAD_ARG;
    std::memcpy(h->world0, w18, 18 * sizeof(float));
    h->world0_bound = nullptr;
    h->bind_dof = nullptr;
    return M3_OK;
}

extern "C" int m3_bind_sim_point(m3_handle* h, const float* dof, const float* root, int n_actors, int box_actor, int dyn_actor) {
    if (!h || !dof || !root) return M3_ERR_BAD_ARG;
    if (n_actors < 1 || box_actor < 0 || box_actor >= n_actors || dyn_actor < 0 || dyn_actor >= n_actors)
        return fail(h, M3_ERR_SHAPE, "m3_bind_sim_point: actor index out of range");
    h->bind_dof = dof; h->bind_root = root; h->bind_nact = n_actors; h->bind_box = box_actor; h->bind_dyn = dyn_actor;
    return M3_OK;
}

static void fill_cost_params(const m3_handle* h, CostParams& cp) {
    cp.task = h->task;
    cp.multi_modal = h->cfg.multi_modal;
    cp.half_K = h->cfg.K_global / 2;
    for (int i = 0; i < 7; ++i) cp.goal[i] = h->goal[i];
    cp.kp_suction = h->cfg.kp_suction;
    cp.suction_thresh = (h->cfg.K_global == 1) ? 1.5f : 1.8f;  // skill_utils.py:75-82
    cp.avoid_dyn_obs = h->avoid_dyn_obs;
}

static void fill_panda_cost_params(const m3_handle* h, PandaCostParams& cp) {
    cp.task = h->task;
    cp.multi_modal = h->cfg.multi_modal;
    cp.half_K = h->cfg.K_global / 2;
    for (int i = 0; i < 7; ++i) cp.goal[i] = h->goal[i];
    cp.pre_height_diff = h->cfg.pre_height_diff;
    cp.tilt_cos_theta = 0.5f;  // cost_functions.py:13
}

// panda_env initial state, 57 floats: q[9] qd[9] | cubeA | cubeB | dyn-obs, each pos3 quat4(xyzw) linvel3 angvel3
extern "C" int m3_set_world_panda_raw(m3_handle* h, const float* w57) {
    const float* w31 = w57;
    if (!h || !w31) return M3_ERR_BAD_ARG;
    if (h->cfg.env_type != M3_ENV_PANDA) return fail(h, M3_ERR_STATE, "m3_set_world_panda_raw: not a panda_env handle");
    std::memcpy(h->pworld0, w31, 57 * sizeof(float));
    h->bind_dof = nullptr;
    return M3_OK;
}

extern "C" int m3_bind_sim_panda(m3_handle* h, const float* dof, const float* root, int n_actors, int cubeA_actor, int cubeB_actor,
                                 int obs_actor) {
    if (!h || !dof || !root) return M3_ERR_BAD_ARG;
    if (h->cfg.env_type != M3_ENV_PANDA) return fail(h, M3_ERR_STATE, "m3_bind_sim_panda: not a panda_env handle");
    if (n_actors < 1 || cubeA_actor < 0 || cubeA_actor >= n_actors || cubeB_actor < 0 || cubeB_actor >= n_actors ||
        obs_actor < 0 || obs_actor >= n_actors)
        return fail(h, M3_ERR_SHAPE, "m3_bind_sim_panda: actor index out of range");
    h->bind_dof = dof; h->bind_root = root; h->bind_nact = n_actors; h->bind_box = cubeA_actor; h->bind_dyn = cubeB_actor;
    h->bind_obs = obs_actor;
    return M3_OK;
}

// m3_rollout's choice of the reach command's kernel form: share (1/1000) of the last finished command's (sample, substep) pairs with
// the gripper within reach of a box from which eight lanes per sample take over / below which one lane does again
// (tools/panda_reach_mid_bench.py, profiles/r05/panda_reach_mid_bench.json; K = 4000, T = 20, rollout ms with 1 / 8 lanes: the arm at
// its initial pose 148 per mille 0.166 / 0.210, 20 ticks into an episode 116: 0.179 / 0.206, 30 ticks 442: 0.383 / 0.287, 40 ticks
// 842: 0.784 / 0.450, 60 ticks 993: 1.530 / 0.831 -- the forms cross near 240; the eight-lane form's own count runs ~10 % higher,
// its shadow slots included)

// the conditions under which m3_rollout refuses (M3_ERR_STATE; nullptr: none) -- batch_refusal checks them too
static const char* rollout_refusal(const m3_handle* h) {
    const m3_config& c = h->cfg;
    if (c.sim_only) return "m3_rollout: handle was created sim_only";
    if (!c.sampling_random && !c.mode_simple && !h->have_noise)
        return "m3_rollout: no noise set (m3_set_noise) and sampling_random == 0";
    if (c.mode_simple && !c.sampling_random && !h->have_noise)
        return "m3_rollout: simple mode needs m3_set_noise or sampling_random";
    if (h->task == M3_TASK_PUSH_PULL && !c.multi_modal) return "m3_rollout: push_pull needs multi_modal";
    if (const char* why = panda_refusal(h, PANDA_SIDE_ROLLOUT)) return why;
    if (prior_controller_on(h) && h->priors.ctl.kind == M3_PRIOR_CONTROLLER_PUSH_BEHIND && h->task == M3_TASK_NAVIGATION)
        return "m3_rollout: the prior controller is PUSH_BEHIND (m3_set_prior_controller) but the task is navigation, which has no box to go behind";
    return point_variant_refusal(h, SIDE_ROLLOUT);
}

// the rollout's arguments; refreshes the wavefront order when it is due (a stream-ordered launch)
static int prepare_rollout(m3_handle* h, RolloutArgs& a) {
    const m3_config& c = h->cfg;
    std::memset(&a, 0, sizeof(a));
    a.Kg = c.K_global; a.Kl = c.K_local; a.k0 = c.k_offset; a.T = c.T; a.nu = c.nu;
    a.multi_modal = c.multi_modal; a.mode_simple = c.mode_simple;
    a.sampling_random = c.sampling_random; a.sample_null_action = c.sample_null_action;
    a.gripper_cmd = h->gripper_cmd;
    for (int j = 0; j < c.nu; ++j) {
        a.u_min[j] = c.u_min[j]; a.u_max[j] = c.u_max[j];
        a.scale_tril[j] = std::sqrt(c.noise_sigma_diag[j]);  // mppi.py:175-176
        a.sigma_inv[j] = 1.0f / c.noise_sigma_diag[j];       // mppi.py:128 (diagonal)
    }
    a.u_scale = c.u_scale; a.gamma = c.gamma; a.lambda_ = c.lambda_;
    a.noise_abs_cost = c.noise_abs_cost; a.full_sigma = c.full_sigma;
    for (int j = 0; j < c.nu; ++j) a.noise_mu[j] = c.noise_mu[j];
    a.noise_mats = h->noise_mats;
    a.scale_dev = h->cov_active ? (const float*)h->buf[M3_BUF_COV] + c.nu : nullptr;
    a.seed = c.seed; a.call = h->calls;
    fill_cost_params(h, a.cp);
    std::memcpy(a.world0, h->world0, sizeof(a.world0));
    if (h->bind_dof) {
        a.sim_dof = h->bind_dof; a.sim_root = h->bind_root;
        a.sim_box = h->bind_box; a.sim_dyn = h->bind_dyn;
    }
    a.lanes = h->lanes_override > 0 ? h->lanes_override : rollout_lanes_for(c.K_local);
    a.delta = (const float*)h->buf[M3_BUF_NOISE];
    if (h->relabelled && h->wave_order && h->calls % ORDER_REFRESH == 0 && h->calls != h->last_noise_call)
        h->relabel_pending = true;   // the objects move: relabel again now and then (labels carry no meaning)
    if (h->order_dirty || h->relabel_pending || (h->wave_order && h->calls % ORDER_REFRESH == 0)) {
        const int rc = refresh_wave_order(h);
        if (rc != M3_OK) return rc;
    }
    a.order = h->order_valid ? h->order : nullptr;
    if (a.order) a.delta = h->noise_sorted;
    a.mean = (const float*)h->buf[M3_BUF_MEAN];
    a.mean1 = (const float*)h->buf[M3_BUF_MEAN_1];
    a.mean2 = (const float*)h->buf[M3_BUF_MEAN_2];
    a.best1 = (const float*)h->buf[M3_BUF_BEST_1];
    a.best2 = (const float*)h->buf[M3_BUF_BEST_2];
    a.pend = (float*)h->buf[M3_BUF_PENDING_FORCE];
    a.states = (float*)h->buf[M3_BUF_STATES];
    a.actions = (float*)h->buf[M3_BUF_ACTIONS];
    a.cost_h = (float*)h->buf[M3_BUF_COST_HORIZON];
    a.J = (float*)h->buf[M3_BUF_TRAJ_COST];
    a.wave_min = h->wave_min;   // (null unless the handle's update is the three-launch one)
    return M3_OK;
}

// the panda part of a rollout's arguments (plan_rollout): world, objective, quirk Q8's shadow slots, the
// record buffer of k_panda_reach_cost, and the handle's reading of its last busy report (hysteresis: updates h->panda_reach_busy)
static void fill_panda_args(m3_handle* h, const RolloutArgs& a, PandaArgs& pa) {
    std::memcpy(pa.world0, h->pworld0, sizeof(pa.world0));
    pa.cubeA_actor = h->bind_box; pa.cubeB_actor = h->bind_dyn; pa.obs_actor = h->bind_obs;
    fill_panda_cost_params(h, pa.cp);
    // quirk Q8: the reach cost is measured against environment 0's cube (shadow lanes, rollout_panda.hip); a rank of
    // a sharded command does not hold sample 0's noise row and uses each sample's own cube
    pa.shadows = (pa.cp.task == 4 && a.k0 == 0 && a.Kl == a.Kg && a.Kg >= 2) ? (pa.cp.multi_modal ? 2 : 1) : 0;
    pa.lps = h->panda_lps;
    // reach on a handle that would need shadow slots: with room for one round of wavefronts in a many-lane form (K <= 8192)
    // the cost moves into a kernel of its own behind the rollout (rollout_panda.hip: k_panda_reach_cost) -- 17 floats per
    // (step, sample) in between
    pa.reach_rec = (pa.shadows != 0 && a.Kl <= PANDA_REACH_REC_MAX_K && h->panda_reach_deferred) ? h->panda_reach_rec : nullptr;
    // the reach command's kernel form follows what the last command's rollouts met (rollout_panda.hip: panda_lps_for): the
    // kernel's last wavefront reports the share of (sample, substep) pairs with the gripper within reach of a box or an awake
    // cube into a word of mapped host memory (m3_create), read here without a synchronisation (so it is the report of the
    // last FINISHED command); a many-lane form from PANDA_BUSY_ON(_REC) per mille, one lane again below PANDA_BUSY_OFF(_REC).
    pa.busy_hint = h->panda_busy_hint_dev; pa.busy_count = h->panda_busy_count; pa.reach_busy = 0;
    if (h->panda_busy_hint) {
        const int share = *(volatile const int*)h->panda_busy_hint - 1;    // (-1: nothing reported yet)
        // (with the cost kernel available the many-lane form has no shadow slots and takes over earlier)
        const int on = pa.reach_rec ? PANDA_BUSY_ON_REC : PANDA_BUSY_ON, off = pa.reach_rec ? PANDA_BUSY_OFF_REC : PANDA_BUSY_OFF;
        if (share >= on) h->panda_reach_busy = 1;
        else if (share >= 0 && share < off) h->panda_reach_busy = 0;
        pa.reach_busy = h->panda_reach_busy;
    }
}

// a handle's rollout, as m3_rollout launches it and m3_batch_command groups it: the arguments (prepare_rollout), for panda_env
// the panda part (fill_panda_args), and the form (p; a and pa become what the kernels receive).  Keeps the handle's record of
// what the launch leaves: the rows of minima (wave_min_rows), the panda form (panda_lps_used)
static int plan_rollout(m3_handle* h, RolloutArgs& a, PandaArgs& pa, RolloutPlan& p, bool own_launch = false) {
    const int rc = prepare_rollout(h, a);
    if (rc != M3_OK) return rc;
    if (h->cfg.env_type == M3_ENV_POINT) {
        // (the two-wavefront form: m3_rollout's own launch only, and only with the error word to report into)
        p = plan_rollout_point(a, h->scene, point_variant(h, SIDE_ROLLOUT), (own_launch && h->rollout_err_dev) ? h->point_form : 0,
                               h->point_rows.sample_on, h->priors.n > 0);
    } else {
        fill_panda_args(h, a, pa);
        p = plan_rollout_panda(a, pa);
        h->panda_lps_used = p.lps;
    }
    a.lanes = p.lanes;
    h->wave_min_rows = p.rows;
    return M3_OK;
}

extern "C" int m3_rollout(m3_handle* h) {
    if (!h) return M3_ERR_BAD_ARG;
    if (const char* why = rollout_refusal(h)) return fail(h, M3_ERR_STATE, why);
    RolloutArgs a;
    PandaArgs pa;
    RolloutPlan p;
    if (h->rollout_err && *(volatile const int*)h->rollout_err != 0)
        return fail(h, M3_ERR_HIP, "m3_rollout: a hand-over wait between the two wavefronts of an earlier rollout launch ran out "
                                   "(its results are invalid); m3_set_point_rollout_form(h, 0) avoids the form");
    const int rc = plan_rollout(h, a, pa, p, true);
    if (rc != M3_OK) return rc;
    if (h->cfg.env_type == M3_ENV_POINT) { h->point_form_used = p.form; h->priors.used = p.priors; }
    if (h->timing) HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    // the handle's ancillary controllers fill its table of priors from the world this rollout starts from, directly ahead of it
    if (prior_controller_on(h)) launch_prior_controllers(a, prior_controller_args(h), h->stream);
    if (h->cfg.env_type == M3_ENV_POINT) launch_rollout_point(a, h->scene, h->scene_rt, h->cost_weights, p, h->stream, h->rollout_err_dev, h->point_rows.dev,
                                                              h->priors.slot_dev, h->priors.tab_dev);
    else {
        const PandaDecision d = panda_decision(panda_input(h), PANDA_SIDE_ROLLOUT);
        launch_rollout_panda(a, pa, panda_launch_scene(h, d.variant), p, h->stream);
        panda_record_used(h, d);
        h->panda_priors.used = d.variant == PANDA_PRIORS ? 1 : 0;
    }
    // the handle's sample groups: each group's costs become one aggregate, behind the last writer of M3_BUF_TRAJ_COST
    if (h->groups.n > 0) aggregate_sample_groups(h);
    HIPCHK(h, hipGetLastError());
    if (h->timing) HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    return M3_OK;
}

// the controller alone, for the world currently set or bound: what the next rollout's launch of it would write
extern "C" int m3_prior_controller_fill(m3_handle* h) {
    if (!h) return M3_ERR_BAD_ARG;
    if (h->cfg.env_type != M3_ENV_POINT) return fail(h, M3_ERR_UNSUPPORTED, (std::string("m3_prior_controller_fill") + env_only_text(M3_ENV_POINT)).c_str());
    if (!prior_controller_on(h)) return fail(h, M3_ERR_STATE, "m3_prior_controller_fill: the handle has no prior controller (m3_set_prior_controller)");
    if (const char* why = rollout_refusal(h)) return fail(h, M3_ERR_STATE, why);
    // (of the rollout's arguments the kernel reads the world, the goal, u_max and T: no wavefront order is refreshed here)
    const m3_config& c = h->cfg;
    RolloutArgs a;
    std::memset(&a, 0, sizeof(a));
    a.Kg = c.K_global; a.Kl = c.K_local; a.k0 = c.k_offset; a.T = c.T; a.nu = c.nu;
    for (int j = 0; j < c.nu; ++j) { a.u_min[j] = c.u_min[j]; a.u_max[j] = c.u_max[j]; }
    fill_cost_params(h, a.cp);
    std::memcpy(a.world0, h->world0, sizeof(a.world0));
    if (h->bind_dof) {
        a.sim_dof = h->bind_dof; a.sim_root = h->bind_root;
        a.sim_box = h->bind_box; a.sim_dyn = h->bind_dyn;
    }
    launch_prior_controllers(a, prior_controller_args(h), h->stream);
    HIPCHK(h, hipGetLastError());
    return M3_OK;
}

// where a command leaves its plan: the caller's destination (m3_set_action_out) or M3_BUF_ACTION_OUT
static float* plan_dst(const m3_handle* h) { return h->action_out ? h->action_out : (float*)h->buf[M3_BUF_ACTION_OUT]; }
// floats of that plan: [u_per_command][nu] in simple mode, else [T][nu]
static size_t plan_floats(const m3_config& c) { return (size_t)(c.mode_simple ? c.u_per_command : c.T) * c.nu; }

static void fill_update_args(m3_handle* h, UpdateArgs& a) {
    const m3_config& c = h->cfg;
    std::memset(&a, 0, sizeof(a));
    a.Kg = c.K_global; a.Kl = c.K_local; a.k0 = c.k_offset; a.T = c.T; a.nu = c.nu;
    a.multi_modal = c.multi_modal; a.mode_simple = c.mode_simple; a.env_type = c.env_type;
    a.filter_u = c.filter_u; a.u_per_command = c.u_per_command;
    a.lambda_ = c.lambda_; a.step_size_mean = c.step_size_mean;
    a.cand = h->topk_cand;
    a.ladder_spins = h->ladder_spins;
    a.p2p_err = (h->p2p_ready && h->xb) ? (const int*)((const char*)h->xb + 2 * MIX_MAX_RANKS * sizeof(int)) : nullptr;
    a.part_min = h->part_min;
    a.n_cand = topk_workgroups(c.K_global);
    a.n_mins = mins_workgroups(c.K_global);
    a.lad = h->lad;
    a.wpart = h->wpart;
    a.srch = (SearchOut*)h->apart;
    a.apart = h->apart + 16;
    a.wcount = h->wcount;
    a.lflag = h->lflag;
    a.n_chunk = wsum_chunks(c.K_local);
    a.n_lad = ladder_workgroups(c.K_global);
    // (unsharded: the local costs ARE the global costs, no copy)
    a.Jall = (const float*)h->buf[c.K_local == c.K_global ? M3_BUF_TRAJ_COST : M3_BUF_TRAJ_COST_ALL];
    a.w = (float*)h->buf[M3_BUF_WEIGHTS];
    a.w1 = (float*)h->buf[M3_BUF_WEIGHTS_1];
    a.w2 = (float*)h->buf[M3_BUF_WEIGHTS_2];
    a.top_idx = (int*)h->buf[M3_BUF_TOP_IDX];
    a.info = (m3_info*)h->buf[M3_BUF_INFO];
    a.actions = (const float*)h->buf[M3_BUF_ACTIONS];
    a.states = (const float*)h->buf[M3_BUF_STATES];
    a.reduce = (float*)h->buf[M3_BUF_REDUCE];
    a.mean = (float*)h->buf[M3_BUF_MEAN];
    a.mean1 = (float*)h->buf[M3_BUF_MEAN_1];
    a.mean2 = (float*)h->buf[M3_BUF_MEAN_2];
    a.best = (float*)h->buf[M3_BUF_BEST];
    a.best1 = (float*)h->buf[M3_BUF_BEST_1];
    a.best2 = (float*)h->buf[M3_BUF_BEST_2];
    a.action_out = plan_dst(h);
    a.top_trajs = (float*)h->buf[M3_BUF_TOP_TRAJS];
    a.top_dst = (c.K_local == c.K_global) ? a.top_trajs : a.reduce + reduce_off_top(c.T, c.nu);
    a.kbase = 0;
    a.half_g = c.K_global / 2;
    a.n_ranks = c.K_global / c.K_local;
    a.rank = c.k_offset / c.K_local;
    a.records_all = h->records_src ? h->records_src : (const float*)h->buf[M3_BUF_RECORDS_ALL];
    a.rec_topj = a.rec_topi = nullptr;
    a.rec_mins = a.rec_table = nullptr;
    a.rec_b = nullptr;
    a.recb_all = h->recb_src ? h->recb_src : (const float*)h->buf[M3_BUF_RECORDS_B_ALL];
    a.recb_len = h->recb_src ? h->recb_stride : recb_length(c.T, c.nu);
    a.fast = 0;
    a.regen = 0;
    a.Jout = nullptr;
    a.Kls = c.K_local;
    a.rec_len = m3_record_len(h);
    if (h->records_src) a.rec_len = h->records_stride;   // (the p2p block's slots are padded to 16 bytes; rec_len is only ever a stride)
    a.noise_all = h->noise_all;
    for (int j = 0; j < c.nu; ++j) {
        a.u_min[j] = c.u_min[j]; a.u_max[j] = c.u_max[j];
        a.scale_tril[j] = std::sqrt(c.noise_sigma_diag[j]);   // as m3_rollout
    }
    a.u_scale = c.u_scale;
    a.sample_null_action = c.sample_null_action;
    a.gripper_cmd = h->gripper_cmd;
}

// the arguments of a command's update, the finalize fused in or not (also what m3_batch_command launches for every handle)
static void fill_update_impl_args(m3_handle* h, UpdateArgs& a, bool fuse) {
    fill_update_args(h, a);
    a.fuse_finalize = fuse ? 1 : 0;
}

// MPPIConfig.update_cov: the covariance update that follows the mean update (mppi.py:508-516)
static int after_finalize(m3_handle* h) {
    if (!h->cov_active) return M3_OK;
    const m3_config& c = h->cfg;
    launch_cov_update((const float*)h->buf[M3_BUF_ACTIONS], (const float*)h->buf[M3_BUF_WEIGHTS],
                      (const float*)h->buf[M3_BUF_MEAN], h->wpart, (float*)h->buf[M3_BUF_COV], c.K_local, c.T, c.nu,
                      h->stream);
    HIPCHK(h, hipGetLastError());
    return M3_OK;
}

// the end of a command whose finalize has been enqueued (m3_finalize, m3_update_finalize, m3_batch_command): the covariance
// step, the end-of-command timing event (timed: not in a batch), the call count
static int finish_command(m3_handle* h, bool timed, bool covariance = true) {
    const int rc = covariance ? after_finalize(h) : M3_OK;
    if (rc != M3_OK) return rc;
    if (timed && h->timing) HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
    h->calls += 1;
    return M3_OK;
}

// ---- what a step of an update plan sees and where it writes (update_plan.hpp: UpdateView, UpdateDest) ----
// the launch sees the local shard as if it were all there is, and reports global indices
static void view_local_shard(const m3_handle* h, UpdateArgs& a) {
    const m3_config& c = h->cfg;
    a.Kg = c.K_local;
    a.kbase = c.k_offset;
    a.Jall = (const float*)h->buf[M3_BUF_TRAJ_COST];   // (the record protocols: the head of the record)
    a.w += c.k_offset; a.w1 += c.k_offset;
}
// the launch covers every sample of every rank
static void view_all_samples(const m3_handle* h, UpdateArgs& a) {
    a.Kl = h->cfg.K_global; a.k0 = 0;
    a.n_chunk = wsum_chunks(h->cfg.K_global);
    a.top_dst = a.top_trajs;               // rows come from the gathered records (topk_finish)
}
// the step writes into this rank's record (in its protocol's layout) or second record
static void dest_record(const m3_handle* h, const UpdateStep& st, UpdateArgs& a) {
    const m3_config& c = h->cfg;
    float* rec = (float*)h->buf[M3_BUF_RECORD];
    if (st.dest == UPDATE_DEST_RECORD_B) {
        float* recb = (float*)h->buf[M3_BUF_RECORD_B];
        if (st.launch == UPDATE_LAUNCH_WSUM) { a.reduce = recb + RECB_HDR; a.n_cand = 0; }   // the sums + the rows of the local best samples
        else a.rec_b = recb;                                                                  // the header
    } else if (update_mix_record(h->protocol)) {
        a.record = rec;
        a.rec_topj = rec + REC_TOPJ;
        a.rec_topi = rec + REC_TOPI;
        a.reduce = rec + REC_HDR;
        a.top_dst = a.reduce + reduce_off_top(c.T, c.nu);
        a.n_cand = topk_workgroups(c.K_local);
    } else {   // the shard's own top-k (costs, global indices, trajectories) behind its costs
        a.n_cand = c.K_local <= 8192 ? 1 : topk_workgroups(c.K_local);
        a.top_idx = h->local_top_idx;
        a.rec_topj = rec + regen_off_topj(c.K_local);
        a.rec_topi = rec + regen_off_topi(c.K_local);
        a.top_dst = rec + regen_off_trajs(c.K_local);
        if (st.fast) {   // ... and its minima + ladder table
            a.rec_mins = rec + regen_off_mins(c.K_local, c.T);
            a.rec_table = rec + regen_off_table(c.K_local, c.T);
        }
    }
}

// The one executor of the update plans: every step launches with freshly filled arguments, its view and its flags.
static int run_update_plan(m3_handle* h, const UpdatePlan& p) {
    bool checked = false;
    for (int i = 0; i < p.n; ++i) {
        const UpdateStep& st = p.step[i];
        UpdateArgs a;
        fill_update_impl_args(h, a, st.fuse_finalize);
        a.regen = st.regen ? 1 : 0;
        a.fast = st.fast ? 1 : 0;
        if (st.view == UPDATE_VIEW_LOCAL) view_local_shard(h, a);
        else if (st.view == UPDATE_VIEW_ALL) view_all_samples(h, a);
        if (st.dest != UPDATE_DEST_BUFFERS) dest_record(h, st, a);
        if (st.regen && !st.fast) a.Jout = (float*)h->buf[M3_BUF_TRAJ_COST_ALL];   // k_mins, the first reader of the gathered records, compacts their costs into it
        if (st.rollout_minima) { a.part_min = h->wave_min; a.n_mins = h->wave_min_rows; }
        switch (st.launch) {
            case UPDATE_LAUNCH_MINS: launch_mins(a, h->stream); break;
            case UPDATE_LAUNCH_LADDER: launch_ladder(a, h->stream); break;
            case UPDATE_LAUNCH_WEIGHTS: launch_weights(a, h->stream); break;
            case UPDATE_LAUNCH_WSUM: launch_wsum(a, h->stream); break;
            case UPDATE_LAUNCH_FINALIZE: launch_finalize(a, h->stream); break;
            case UPDATE_LAUNCH_SMALL: launch_update_small(a, h->stream); break;
            case UPDATE_LAUNCH_LADDER_SEARCH: a.epoch = ++h->lad_epoch; launch_ladder_search(a, h->stream); break;
            case UPDATE_LAUNCH_FUSED_LARGE: a.epoch = h->lad_epoch; launch_fused_large(a, h->stream); break;   // (the search's epoch)
            case UPDATE_LAUNCH_LOCAL_TOPK: launch_local_topk(a, h->stream); break;
            case UPDATE_LAUNCH_MIX: launch_mix(a, h->stream); break;
            case UPDATE_LAUNCH_REGEN_FAST: launch_regen_fast(a, h->stream); break;
            case UPDATE_LAUNCH_P3_SEARCH: launch_p3_search(a, h->stream); break;
            case UPDATE_LAUNCH_P3_LOCAL_WEIGHTS: launch_p3_local_weights(a, h->stream); break;
            case UPDATE_LAUNCH_P3_DONE: launch_p3_done(a, h->stream); break;
        }
        checked = st.ends_update;
        if (st.ends_update) {
            HIPCHK(h, hipGetLastError());
            if (h->timing) HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
        }
    }
    if (!checked) HIPCHK(h, hipGetLastError());
    return p.ends_command ? finish_command(h, true, p.covariance) : M3_OK;
}

static int update_refused(m3_handle* h, UpdateRefusal r, bool from_command) {
    return fail(h, update_refusal_is_state(r) ? M3_ERR_STATE : M3_ERR_UNSUPPORTED, update_refusal_text(r, from_command));
}
static int run_update_entry(m3_handle* h, UpdateEntry entry, bool rollout_minima) {
    const UpdatePlan p = update_plan(update_plan_input(h, false, rollout_minima), entry);
    if (p.refusal != UPDATE_REFUSAL_NONE) return update_refused(h, p.refusal, false);
    if (h->cfg.sim_only && (entry == UPDATE_ENTRY_UPDATE || entry == UPDATE_ENTRY_UPDATE_FINALIZE))
        return fail(h, M3_ERR_STATE, "m3_update: handle was created sim_only");
    return run_update_plan(h, p);
}

extern "C" int m3_update(m3_handle* h) {
    if (!h) return M3_ERR_BAD_ARG;
    return run_update_entry(h, UPDATE_ENTRY_UPDATE, false);
}

// shard_mix = 3, between the two exchanges (update_sharded.hip: k_p3_done's comment)
extern "C" int m3_update_b(m3_handle* h) {
    if (!h) return M3_ERR_BAD_ARG;
    return run_update_entry(h, UPDATE_ENTRY_UPDATE_B, false);
}

// ---- device-side exchange of the records (p2p.hip) -------------------------------------------------------------
static int p2p_ranks(const m3_handle* h) { return h->cfg.K_global / h->cfg.K_local; }
static int p2p_rank(const m3_handle* h) { return h->cfg.k_offset / h->cfg.K_local; }
// the device a pointer lives on (-1: unknown)
static int ptr_device(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return at.device;
}
static int p2p_alloc(m3_handle* h) {
    if (h->xb) return M3_OK;
    const m3_config& c = h->cfg;
    // the block belongs on the HANDLE's device, whatever device is current on the calling thread (a process that
    // drives several GPUs, torch's current device): set it for the allocation and put the caller's back
    struct DeviceGuard {
        int prev = -1;
        explicit DeviceGuard(int d) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; (void)hipSetDevice(d); }
        ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    } guard(c.device);
    if (!update_has_record(h->protocol) || !h->buf[M3_BUF_RECORD])
        return fail(h, M3_ERR_STATE, "m3_p2p: the handle has no record to exchange (needs cfg.shard_mix on a sharded handle)");
    const size_t rl = (size_t)m3_record_len(h), rlb = (size_t)m3_record_b_len(h);
    h->xb_bytes = P2P_HDR_BYTES + 2 * (size_t)p2p_ranks(h) * (((rl + 3) & ~(size_t)3) + ((rlb + 3) & ~(size_t)3)) * sizeof(float);
    // uncached: neither the peers' stores nor the owner's loads may be served from a stale L2 line
    // (m3_p2p_set_memory_kind: start further down the fallback chain -- the tests of the fenced paths)
    const int first = h->xb_first_kind;
    // (the ledger holds whichever attempt succeeded, as device memory)
    if (first <= 1 && own_device(h->mem, h->xb, h->xb_bytes, hipDeviceMallocUncached) == hipSuccess) h->xb_kind = 1;
    else if ((void)hipGetLastError(), first <= 2 && own_device(h->mem, h->xb, h->xb_bytes, hipDeviceMallocFinegrained) == hipSuccess) h->xb_kind = 2;
    else if ((void)hipGetLastError(), own_device(h->mem, h->xb, h->xb_bytes) == hipSuccess) h->xb_kind = 3;
    else return fail(h, M3_ERR_HIP, "m3_p2p: allocation of the exchange block failed");
    HIPCHK(h, hipMemset(h->xb, 0, h->xb_bytes));
    HIPCHK(h, hipDeviceSynchronize());
    const int on = ptr_device(h->xb);
    if (on >= 0 && on != c.device) return fail(h, M3_ERR_HIP, "m3_p2p: the exchange block did not land on the handle's device");
    return M3_OK;
}

extern "C" int m3_p2p_export(m3_handle* h, m3_ipc_handle* out) {
    if (!h || !out) return M3_ERR_BAD_ARG;
    const int rc = p2p_alloc(h);
    if (rc != M3_OK) return rc;
    static_assert(sizeof(hipIpcMemHandle_t) <= sizeof(m3_ipc_handle), "m3_ipc_handle too small");
    hipIpcMemHandle_t ih;
    HIPCHK(h, hipIpcGetMemHandle(&ih, h->xb));
    std::memset(out, 0, sizeof(*out));
    std::memcpy(out->bytes, &ih, sizeof(ih));
    return M3_OK;
}

static int p2p_finish_connect(m3_handle* h) {
    for (int p = 0; p < p2p_ranks(h); ++p)
        if (!h->peer_base[p]) return fail(h, M3_ERR_STATE, "m3_p2p_connect: a peer's block is missing");
    // (re-)arm: own flags, error word and sequence numbers start from zero.  Collective by nature -- no peer may put
    // between this and the barrier every caller of connect holds before its first exchange (distributed.attach_p2p).
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemset(h->xb, 0, P2P_HDR_BYTES));
    HIPCHK(h, hipDeviceSynchronize());
    h->p2p_ready = true;
    h->p2p_seq[0] = h->p2p_seq[1] = 0;
    h->records_src = nullptr; h->recb_src = nullptr;
    return M3_OK;
}

extern "C" int m3_p2p_clear_error(m3_handle* h) {
    if (!h) return M3_ERR_BAD_ARG;
    if (!h->xb || !h->p2p_ready) return fail(h, M3_ERR_STATE, "m3_p2p_clear_error: no connected exchange block");
    return p2p_finish_connect(h);
}

extern "C" int m3_p2p_detach(m3_handle* h) {
    if (!h) return M3_ERR_BAD_ARG;
    // the blocks stay mapped (m3_p2p_connect* re-arms them); the finalize kernels no longer read the error word, so a
    // handle whose exchange gave up hands out plans again once its records come from another transport
    if (h->xb) HIPCHK(h, hipStreamSynchronize(h->stream));
    h->p2p_ready = false;
    h->records_src = nullptr; h->recb_src = nullptr;
    return M3_OK;
}

extern "C" int m3_p2p_set_memory_kind(m3_handle* h, int first_kind) {
    if (!h) return M3_ERR_BAD_ARG;
    if (first_kind < 1 || first_kind > 3) return fail(h, M3_ERR_BAD_ARG, "m3_p2p_set_memory_kind: 1 uncached, 2 fine-grained, 3 plain");
    if (h->xb) return fail(h, M3_ERR_STATE, "m3_p2p_set_memory_kind: the exchange block exists already (call before m3_p2p_export / connect)");
    h->xb_first_kind = first_kind;
    return M3_OK;
}

extern "C" int m3_p2p_connect(m3_handle* h, const m3_ipc_handle* all, int n) {
    if (!h || !all) return M3_ERR_BAD_ARG;
    int rc = p2p_alloc(h);
    if (rc != M3_OK) return rc;
    if (n != p2p_ranks(h)) return fail(h, M3_ERR_SHAPE, "m3_p2p_connect: need one handle per rank");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    for (int p = 0; p < n; ++p) {
        if (p == p2p_rank(h)) { h->peer_base[p] = h->xb; continue; }
        if (h->peer_ipc[p] && h->peer_base[p]) continue;
        hipIpcMemHandle_t ih;
        std::memcpy(&ih, all[p].bytes, sizeof(ih));
        if (own_ipc(h->mem, h->peer_base[p], ih) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, M3_ERR_HIP, "m3_p2p_connect: hipIpcOpenMemHandle failed (peer block of another process)");
        }
        h->peer_ipc[p] = true;
    }
    return p2p_finish_connect(h);
}

extern "C" int m3_p2p_connect_local(m3_handle* h, m3_handle* const* peers, int n) {
    if (!h || !peers) return M3_ERR_BAD_ARG;
    int rc = p2p_alloc(h);
    if (rc != M3_OK) return rc;
    if (n != p2p_ranks(h)) return fail(h, M3_ERR_SHAPE, "m3_p2p_connect_local: need one handle per rank");
    for (int p = 0; p < n; ++p) {
        m3_handle* q = peers[p];
        if (!q || p2p_rank(q) != p || m3_record_len(q) != m3_record_len(h) || p2p_ranks(q) != n ||
            m3_record_b_len(q) != m3_record_b_len(h) || q->cfg.shard_mix != h->cfg.shard_mix)
            return fail(h, M3_ERR_SHAPE, "m3_p2p_connect_local: peers[p] must be the handle of rank p of the same sharding and protocol");
        rc = p2p_alloc(q);
        if (rc != M3_OK) return fail(h, rc, "m3_p2p_connect_local: a peer could not allocate its block");
        const int on = ptr_device(q->xb);
        if (on >= 0 && on != q->cfg.device) return fail(h, M3_ERR_HIP, "m3_p2p_connect_local: a peer's block is not on that peer's device");
        if (q->cfg.device != h->cfg.device) {
            int can = 0, prev = -1;
            (void)hipDeviceCanAccessPeer(&can, h->cfg.device, q->cfg.device);
            if (!can) return fail(h, M3_ERR_UNSUPPORTED, "m3_p2p_connect_local: no peer access between the two devices");
            if (hipGetDevice(&prev) != hipSuccess) prev = -1;
            (void)hipSetDevice(h->cfg.device);
            const hipError_t e = hipDeviceEnablePeerAccess(q->cfg.device, 0);
            if (prev >= 0) (void)hipSetDevice(prev);       // (the caller's current device is the caller's)
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); return fail(h, M3_ERR_HIP, "m3_p2p_connect_local: hipDeviceEnablePeerAccess"); }
            (void)hipGetLastError();
        }
        h->peer_base[p] = q->xb;
    }
    return p2p_finish_connect(h);
}

// channel 0: the records (M3_BUF_RECORD); channel 1: the second records of shard_mix = 3 (M3_BUF_RECORD_B)
static void p2p_args(m3_handle* h, P2PArgs& a, int ch) {
    std::memset(&a, 0, sizeof(a));
    const int lenA = m3_record_len(h), strideA = (lenA + 3) & ~3;
    a.rec = (const float*)h->buf[ch == 0 ? M3_BUF_RECORD : M3_BUF_RECORD_B];
    a.rec_len = ch == 0 ? lenA : m3_record_b_len(h);
    a.rec_stride = (a.rec_len + 3) & ~3;
    a.n_ranks = p2p_ranks(h);
    a.rank = p2p_rank(h);
    a.seq = h->p2p_seq[ch];
    a.slot = a.seq & 1;
    a.timeout_ticks = 100000ull * (unsigned long long)(a.seq <= 1 ? h->p2p_first_ms : h->p2p_ms);   // 100 MHz wall clock
    a.plain_memory = h->xb_kind != 1;     // only the uncached block skips both GPUs' L2 for certain: the fine-grained fallback gets the fences too
    a.err = (int*)((char*)h->xb + 2 * MIX_MAX_RANKS * sizeof(int));
    for (int p = 0; p < a.n_ranks; ++p) {
        a.peer_flags[p] = (int*)((char*)h->peer_base[p] + (ch == 0 ? 0 : 512));
        a.peer_data[p] = (float*)((char*)h->peer_base[p] + P2P_HDR_BYTES) + (ch == 0 ? 0 : 2 * (size_t)a.n_ranks * strideA);
    }
}

extern "C" int m3_p2p_put_ch(m3_handle* h, int ch) {
    if (!h) return M3_ERR_BAD_ARG;
    if (ch != 0 && !(ch == 1 && update_second_record(h->protocol))) return fail(h, M3_ERR_BAD_ARG, "m3_p2p_put: channel 1 exists on shard_mix = 3 handles only");
    if (!h->p2p_ready) return fail(h, M3_ERR_STATE, "m3_p2p_put: m3_p2p_connect first");
    h->p2p_seq[ch] += 1;
    P2PArgs a;
    p2p_args(h, a, ch);
    launch_p2p_put(a, h->stream);
    HIPCHK(h, hipGetLastError());
    return M3_OK;
}

extern "C" int m3_p2p_wait_ch(m3_handle* h, int ch) {
    if (!h) return M3_ERR_BAD_ARG;
    if (ch != 0 && !(ch == 1 && update_second_record(h->protocol))) return fail(h, M3_ERR_BAD_ARG, "m3_p2p_wait: channel 1 exists on shard_mix = 3 handles only");
    if (!h->p2p_ready || h->p2p_seq[ch] == 0) return fail(h, M3_ERR_STATE, "m3_p2p_wait: no exchange in flight (m3_p2p_put first)");
    P2PArgs a;
    p2p_args(h, a, ch);
    launch_p2p_wait(a, h->stream);
    HIPCHK(h, hipGetLastError());
    const float* src = a.peer_data[a.rank] + (size_t)a.slot * a.n_ranks * a.rec_stride;
    if (ch == 0) { h->records_src = src; h->records_stride = a.rec_stride; }
    else { h->recb_src = src; h->recb_stride = a.rec_stride; }
    return M3_OK;
}

extern "C" int m3_p2p_put(m3_handle* h) { return m3_p2p_put_ch(h, 0); }
extern "C" int m3_p2p_wait(m3_handle* h) { return m3_p2p_wait_ch(h, 0); }
static int p2p_exchange_ch(m3_handle* h, int ch) {   // put + wait in one launch
    if (!h) return M3_ERR_BAD_ARG;
    if (ch != 0 && !(ch == 1 && update_second_record(h->protocol))) return fail(h, M3_ERR_BAD_ARG, "m3_p2p_exchange: channel 1 exists on shard_mix = 3 handles only");
    if (!h->p2p_ready) return fail(h, M3_ERR_STATE, "m3_p2p_exchange: m3_p2p_connect first");
    h->p2p_seq[ch] += 1;
    P2PArgs a;
    p2p_args(h, a, ch);
    launch_p2p_exchange(a, h->stream);
    HIPCHK(h, hipGetLastError());
    const float* src = a.peer_data[a.rank] + (size_t)a.slot * a.n_ranks * a.rec_stride;
    if (ch == 0) { h->records_src = src; h->records_stride = a.rec_stride; }
    else { h->recb_src = src; h->recb_stride = a.rec_stride; }
    return M3_OK;
}
extern "C" int m3_p2p_exchange(m3_handle* h) { return p2p_exchange_ch(h, 0); }
extern "C" int m3_p2p_exchange_b(m3_handle* h) { return p2p_exchange_ch(h, 1); }

extern "C" int m3_p2p_set_timeout_ms(m3_handle* h, int first_ms, int ms) {
    if (!h) return M3_ERR_BAD_ARG;
    if (first_ms < 1 || first_ms > 600000 || ms < 1 || ms > 600000)
        return fail(h, M3_ERR_BAD_ARG, "m3_p2p_set_timeout_ms: 1 .. 600000 ms each");
    h->p2p_first_ms = first_ms;
    h->p2p_ms = ms;
    return M3_OK;
}

extern "C" int m3_p2p_status(m3_handle* h, int* missing_rank, int* memory_kind) {
    if (!h) return M3_ERR_BAD_ARG;
    if (!h->xb) return fail(h, M3_ERR_STATE, "m3_p2p_status: no exchange block");
    int e = 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(&e, (char*)h->xb + 2 * MIX_MAX_RANKS * sizeof(int), sizeof(int), hipMemcpyDeviceToHost));
    if (missing_rank) *missing_rank = e - 1;      // -1: every exchange so far was complete
    if (memory_kind) *memory_kind = h->xb_kind;
    return M3_OK;
}

extern "C" int m3_finalize(m3_handle* h) {
    if (!h) return M3_ERR_BAD_ARG;
    struct Consume { m3_handle* h; ~Consume() { h->records_src = nullptr; h->recb_src = nullptr; } } consume{h};   // one exchange, one finalize
    return run_update_entry(h, UPDATE_ENTRY_FINALIZE, false);
}

extern "C" int m3_update_finalize(m3_handle* h) {
    if (!h) return M3_ERR_BAD_ARG;
    return run_update_entry(h, UPDATE_ENTRY_UPDATE_FINALIZE, false);
}

extern "C" int m3_command(m3_handle* h, float* action_host) {
    if (!h) return M3_ERR_BAD_ARG;
    // a sharded handle needs the collective(s) between the phases: running update + finalize on the
    // local costs alone would return a plan built from zero / stale remote slices without an error
    if (const UpdateRefusal r = update_refusal(update_plan_input(h, false, false), UPDATE_ENTRY_UPDATE_FINALIZE)) return update_refused(h, r, true);
    int rc = m3_rollout(h);
    if (rc != M3_OK) return rc;
    // weights -> sums + (last workgroup) mean update / filter; the costs the update reads are this rollout's
    // (with sample groups the rollout's rows of wave minima are minima of costs that no longer exist: the update forms its own)
    rc = run_update_entry(h, UPDATE_ENTRY_UPDATE_FINALIZE, h->groups.n == 0 && h->wave_min != nullptr && h->wave_min_rows > 0);
    if (rc != M3_OK) return rc;
    if (action_host) {
        HIPCHK(h, hipMemcpyAsync(action_host, plan_dst(h), plan_floats(h->cfg) * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return M3_OK;
}

// ---------------------------------- batched command ------------------------------------
// One command() of each of n unsharded handles of one environment (handle 0's): per group of handles that run the same
// kernel instance, ONE rollout launch and ONE update launch (a multi-modal group: as many as its residency chunks), the
// handles' arguments read from a device table indexed by blockIdx.y (DESIGN.md "Batched command").  A panda_env group that
// keeps the reach-cost record adds one k_panda_reach_cost launch (not counted by m3_batch_launches).  A batch created with
// M3_BATCH_PANDA_RUNTIME also takes panda_env handles with a run-time workspace, tuned weights or a workspace per sample: the
// second section of its panda table (BatchPandaEntryRT, rollout_panda_batch_rt.hip).  The handles keep
// all of their state; the batch owns only the table: BATCH_SLOTS pinned host slots, each with a device slot and an event
// recorded after the call's last launch (so it guards the host slot's copy AND the device slot's readers, whichever
// stream they ran on).
static thread_local std::string g_batch_err;
constexpr int BATCH_SLOTS = 4;

namespace {
struct BatchKey {
    int variant;               // panda_env: 0 kb_rollout_panda (the literal section), 1 kb_rollout_panda_w, 2 kb_rollout_panda_v
                               // (the run-time section); point_env: 0 (its variants are in the plan)
    RolloutPlan roll;          // rollout: the handle's plan (plan_rollout) ...
    int K, T;                  // ... and sizes
    SmallUpdateInstance upd;   // update: k_update_small's template arguments, width, top-k workgroups
};
// the fields a group shares, in the order the groups are sorted by
auto rollout_fields(const BatchKey& k) {
    const RolloutPlan& p = k.roll;
    // (scene, then weighted, first: that is the order of PointVariant, by which the table's sections lie)
    // (panda_env: the variant first, so that each of its two sections is contiguous in key order)
    // (priors first: the handles with prior samples sort last, as their section lies; their key carries scene 1 whether or not
    // they have an arena per sample -- batch_command -- so they group by K, T and lanes alone)
    return std::tie(k.variant, p.priors, p.scene, p.weighted, p.instance, p.ref, p.lps, p.forces, p.general, p.shadows, p.rec, k.K, k.T, p.lanes);
}
auto update_fields(const BatchKey& k) { return std::tie(k.upd.nu, k.upd.multi, k.upd.jr, k.upd.wt, k.upd.n_cand, k.T); }
bool same_rollout(const BatchKey& x, const BatchKey& y) { return rollout_fields(x) == rollout_fields(y); }
bool less_rollout(const BatchKey& x, const BatchKey& y) { return rollout_fields(x) < rollout_fields(y); }
bool same_update(const BatchKey& x, const BatchKey& y) { return update_fields(x) == update_fields(y); }
bool less_update(const BatchKey& x, const BatchKey& y) { return update_fields(x) < update_fields(y); }
struct BatchHandle {   // one handle's command as planned, in call order (copied into the table by group)
    RolloutArgs a;
    PandaArgs pa;      // (panda_env only)
    UpdateArgs u;
    BatchKey key;
    PandaDecision panda;   // (panda_env only: the batch side's, panda_variant.hpp)
};
// The sections of an environment's table, in the order they lie in: the creation bit that enables the
// section (M3_BATCH_SECTION_*; 0: every batch has it), the size of its entry type, and how one entry is written from a planned
// handle.  batch_section_of says which section a planned handle's entry lies in; m3_batch_create and batch_command read
// nothing else about the sections.
struct BatchSection {
    int bit;
    size_t entry;
    void (*fill)(void* e, const m3_handle* h, const BatchHandle& d);
};
template <class E>
constexpr BatchSection batch_section(int bit, void (*fill)(void*, const m3_handle*, const BatchHandle&)) {
    static_assert(alignof(E) <= 16, "the table's sections start on multiples of 16");
    return {bit, sizeof(E), fill};
}
// point_env: by point_section(plan) -- the three variants, the handles with an arena per sample, the handles with prior samples
const BatchSection BATCH_POINT_SECTIONS[POINT_SECTIONS] = {
    batch_section<BatchRolloutEntry>(0, [](void* e, const m3_handle* h, const BatchHandle& d) {
        *static_cast<BatchRolloutEntry*>(e) = {d.a, h->scene};
    }),
    batch_section<BatchRolloutEntryW>(0, [](void* e, const m3_handle* h, const BatchHandle& d) {
        *static_cast<BatchRolloutEntryW*>(e) = {d.a, h->scene, h->cost_weights};
    }),
    batch_section<BatchRolloutEntryS>(0, [](void* e, const m3_handle* h, const BatchHandle& d) {
        *static_cast<BatchRolloutEntryS*>(e) = {d.a, h->scene_rt, h->cost_weights};
    }),
    batch_section<BatchRolloutEntrySV>(M3_BATCH_SECTION_POINT_ROLLOUT_SCENES, [](void* e, const m3_handle* h, const BatchHandle& d) {
        *static_cast<BatchRolloutEntrySV*>(e) = {d.a, h->scene_rt, h->cost_weights, h->point_rows.dev};
    }),
    batch_section<BatchRolloutEntryPR>(M3_BATCH_SECTION_POINT_PRIORS, [](void* e, const m3_handle* h, const BatchHandle& d) {
        // (the handle's own blocks; without a controller kind 0: the table is the caller's)
        PriorControllerArgs ctl = {{}, h->cfg.dt, h->priors.tab_dev};
        if (prior_controller_on(h)) ctl.pc = h->priors.ctl;
        *static_cast<BatchRolloutEntryPR*>(e) = {d.a, h->scene_rt, h->cost_weights, h->point_rows.sample_on ? h->point_rows.dev : nullptr,
                                                 h->priors.slot_dev, ctl};
    }),
};
static_assert(POINT_PLAIN == 0 && POINT_WEIGHTED == 1 && POINT_SCENE == 2 && POINT_SECTION_SV == 3 && POINT_SECTION_PR == 4, "the order above");
// panda_env: the literal entries, then the run-time ones (a run-time workspace, tuned weights or a workspace per sample)
constexpr int PANDA_SECTIONS = 2;
const BatchSection BATCH_PANDA_SECTIONS[PANDA_SECTIONS] = {
    batch_section<BatchPandaEntry>(0, [](void* e, const m3_handle* h, const BatchHandle& d) {
        *static_cast<BatchPandaEntry*>(e) = {d.a, d.pa, *panda_launch_scene(h, d.panda.variant).lit};
    }),
    batch_section<BatchPandaEntryRT>(M3_BATCH_SECTION_PANDA_RUNTIME, [](void* e, const m3_handle* h, const BatchHandle& d) {
        const PandaLaunchScene sc = panda_launch_scene(h, d.panda.variant);
        *static_cast<BatchPandaEntryRT*>(e) = {d.a, d.pa, *sc.rt, *sc.wt, sc.variant == PANDA_ROWS ? sc.rows : nullptr};
    }),
};
static_assert(POINT_SECTIONS <= BATCH_MAX_SECTIONS && PANDA_SECTIONS <= BATCH_MAX_SECTIONS, "");
struct BatchSections {
    const BatchSection* sec;
    int n;
};
BatchSections batch_sections(bool panda) {
    return panda ? BatchSections{BATCH_PANDA_SECTIONS, PANDA_SECTIONS} : BatchSections{BATCH_POINT_SECTIONS, POINT_SECTIONS};
}
int batch_section_of(bool panda, const BatchHandle& d) {
    return panda ? (d.panda.variant == PANDA_LITERAL ? 0 : 1) : point_section(d.key.roll);
}
// the shape of the environment's tables in a batch created with `flags`
BatchTableShape batch_table_shape(bool panda, int flags) {
    const BatchSections t = batch_sections(panda);
    BatchTableShape z{t.n, {}, sizeof(UpdateArgs)};
    for (int v = 0; v < t.n; ++v) z.entry[v] = (t.sec[v].bit == 0 || (flags & t.sec[v].bit)) ? t.sec[v].entry : 0;
    return z;
}
// the refusal of a point_env handle with an arena per sample by a batch or an episode set that was not created for it
constexpr const char* PRIORS_UNBATCHED = "it has prior samples (m3_set_prior_samples), which only m3_rollout / m3_command run";
constexpr const char* POINT_ROWS_UNBATCHED = "it has an arena per sample (m3_set_point_rollout_scenes), which only m3_rollout / m3_command run";
}  // namespace

struct m3_batch {
    int device = 0, max_handles = 0;
    int flags = 0;           // the sections it was created with (M3_BATCH_SECTION_*; bit 1 is m3_batch_create_ex's M3_BATCH_PANDA_RUNTIME)
    BatchTableShape shape[2] = {};   // of its point_env [0] and panda_env [1] tables: the sections it was created with (flags)
    std::string err;
    size_t slot_bytes = 0;   // of a slot: the largest table of max_handles handles of either shape (batch_table_layout.hpp)
    OwnedBlocks mem{&m3_release_block, 3 * BATCH_SLOTS};   // owns the slots; the three arrays below are views
    char* host[BATCH_SLOTS] = {};
    char* dev[BATCH_SLOTS] = {};
    hipEvent_t done[BATCH_SLOTS] = {};
    bool in_flight[BATCH_SLOTS] = {};
    int next = 0;
    int rollout_launches = 0, update_launches = 0;   // of the last successful m3_batch_command
    // host scratch, sized by m3_batch_create
    std::vector<m3_handle*> seen;
    std::vector<BatchHandle> hd;
    std::vector<int> by_roll, by_upd;
};

extern "C" const char* m3_batch_last_error(const m3_batch* b) { return b ? b->err.c_str() : g_batch_err.c_str(); }

extern "C" void m3_batch_destroy(m3_batch* b) {
    if (!b) return;
    for (int q = 0; q < BATCH_SLOTS; ++q)
        if (b->in_flight[q]) (void)hipEventSynchronize(b->done[q]);   // (kernels may still read the device slot)
    b->mem.release_all();
    delete b;
}

extern "C" int m3_batch_create(int device, int max_handles, m3_batch** out) { return m3_batch_create_ex(device, max_handles, 0, out); }

extern "C" int m3_batch_flags(const m3_batch* b) { return b ? b->flags : M3_ERR_BAD_ARG; }

static int batch_create(int device, int max_handles, int flags, m3_batch** out);
// (the messages keep m3_batch_create's name: flags == 0 is that call)
extern "C" int m3_batch_create_ex(int device, int max_handles, int flags, m3_batch** out) {
    if (!out) { g_batch_err = "m3_batch_create: null argument"; return M3_ERR_BAD_ARG; }
    *out = nullptr;
    if (flags & ~M3_BATCH_PANDA_RUNTIME) { g_batch_err = "m3_batch_create_ex: unknown flag bits"; return M3_ERR_BAD_ARG; }
    return batch_create(device, max_handles, flags, out);
}
static_assert(M3_BATCH_SECTION_PANDA_RUNTIME == M3_BATCH_PANDA_RUNTIME, "one bit, two names");
extern "C" int m3_batch_create_sections(int device, int max_handles, int sections, m3_batch** out) {
    if (out) *out = nullptr;
    if (sections & ~(M3_BATCH_SECTION_PANDA_RUNTIME | M3_BATCH_SECTION_POINT_ROLLOUT_SCENES | M3_BATCH_SECTION_POINT_PRIORS)) {
        g_batch_err = "m3_batch_create_sections: unknown section bits";
        return M3_ERR_BAD_ARG;
    }
    return batch_create(device, max_handles, sections, out);
}
// flags: checked section bits
static int batch_create(int device, int max_handles, int flags, m3_batch** out) {
    if (!out) { g_batch_err = "m3_batch_create: null argument"; return M3_ERR_BAD_ARG; }
    *out = nullptr;
    if (max_handles < 1 || max_handles > 65535) {   // (blockIdx.y picks the handle)
        g_batch_err = "m3_batch_create: max_handles must be in 1 .. 65535";
        return M3_ERR_BAD_ARG;
    }
    int count = 0;
    const hipError_t ce = hipGetDeviceCount(&count);
    if (ce != hipSuccess) {
        g_batch_err = std::string("m3_batch_create: hipGetDeviceCount: ") + hipGetErrorString(ce);
        return M3_ERR_HIP;
    }
    if (device < 0 || device >= count) { g_batch_err = "m3_batch_create: no such HIP device"; return M3_ERR_BAD_ARG; }
    m3_batch* b = new (std::nothrow) m3_batch();
    if (!b) { g_batch_err = "m3_batch_create: out of host memory"; return M3_ERR_HIP; }
    b->device = device;
    b->max_handles = max_handles;
    b->flags = flags;
    for (int panda = 0; panda < 2; ++panda) {
        b->shape[panda] = batch_table_shape(panda != 0, flags);
        b->slot_bytes = std::max(b->slot_bytes, batch_table_capacity(b->shape[panda], max_handles));
    }
    try {
        b->seen.resize(max_handles);
        b->hd.resize(max_handles);
        b->by_roll.resize(max_handles);
        b->by_upd.resize(max_handles);
    } catch (...) {
        delete b;
        g_batch_err = "m3_batch_create: out of host memory";
        return M3_ERR_HIP;
    }
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    hipError_t e = hipSetDevice(device);
    for (int q = 0; q < BATCH_SLOTS && e == hipSuccess; ++q) {
        e = own_pinned(b->mem, b->host[q], b->slot_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = own_device(b->mem, b->dev[q], b->slot_bytes);
        if (e == hipSuccess) e = own_event(b->mem, b->done[q], hipEventDisableTiming);
    }
    if (prev >= 0) (void)hipSetDevice(prev);
    if (e != hipSuccess) {
        g_batch_err = std::string("m3_batch_create: ") + hipGetErrorString(e);
        m3_batch_destroy(b);
        return M3_ERR_HIP;
    }
    *out = b;
    return M3_OK;
}

extern "C" int m3_batch_launches(const m3_batch* b, int* rollout_launches, int* update_launches) {
    if (!b) return M3_ERR_BAD_ARG;
    if (rollout_launches) *rollout_launches = b->rollout_launches;
    if (update_launches) *update_launches = b->update_launches;
    return M3_OK;
}

// the conditions under which m3_batch_command refuses a handle of the call's environment, device and stream (nullptr: none;
// code: the return code) -- m3_episodes_create checks them too.  u: the arguments of the handle's update, as m3_command
// launches it.  sections: the M3_BATCH_SECTION_* bits the caller may use.  With the run-time section a panda_env planner that
// needs the run-time-scene instance, the weighted family or has a workspace per sample passes; with the per-sample section a
// point_env planner with an arena per sample; with the priors section a point_env planner with prior samples -- with or without
// an arena per sample, which that section's entry carries as well
static const char* batch_refusal(m3_handle* h, UpdateArgs& u, int& code, int sections) {
    const m3_config& c = h->cfg;
    const bool in_priors_section = h->priors.n > 0 && (sections & M3_BATCH_SECTION_POINT_PRIORS);   // (its entry carries the rows as well)
    code = M3_ERR_STATE;
    if (c.K_local != c.K_global) return "sharded handle (K_local != K_global)";
    if (c.sim_only) return "handle was created sim_only";
    if (h->groups.n > 0) {   // (no batched launch aggregates: the update of a batch follows its rollout directly)
        code = M3_ERR_UNSUPPORTED;
        return SAMPLE_GROUPS_UNBATCHED;
    }
    if (h->point_rows.sample_on && !(sections & M3_BATCH_SECTION_POINT_ROLLOUT_SCENES) && !in_priors_section) {   // (the table's slots have no fourth section)
        code = M3_ERR_UNSUPPORTED;
        return POINT_ROWS_UNBATCHED;
    }
    if (h->priors.n > 0 && !in_priors_section) {   // (no table entry carries a slot map and a table of priors)
        code = M3_ERR_UNSUPPORTED;
        return PRIORS_UNBATCHED;
    }
    // (no table entry carries a slot map and a table of priors, with or without the run-time section)
    if (c.env_type == M3_ENV_PANDA && panda_refusal(panda_input(h), PANDA_SIDE_BATCH) == PANDA_UNBATCHED_PRIORS) {
        code = M3_ERR_UNSUPPORTED;
        return panda_refusal_text(PANDA_UNBATCHED_PRIORS);
    }
    if (const char* why = rollout_refusal(h)) return why;
    if (!(sections & M3_BATCH_SECTION_PANDA_RUNTIME)) {
        // (the table's entry carries a PandaScene, no table of rows and no weights: its kernels form the literal cost)
        if (const char* why = panda_unbatched(h, PANDA_ROWS_THEN_WEIGHTS)) {
            code = M3_ERR_UNSUPPORTED;
            return why;
        }
    }
    fill_update_impl_args(h, u, true);
    code = M3_ERR_UNSUPPORTED;
    if (const UpdatePlanInput in = update_plan_input(h, true, false); !can_fuse_finalize(in) || !update_small_applies(in))
        return c.env_type == M3_ENV_PANDA
                   ? "its command does not take the one-launch update (nu = 9: K <= 4096, T * nu <= 2048)"
                   : "its command does not take the one-launch update (nu = 2: K <= 16384; multi-modal K <= 8192)";
    return nullptr;
}

static int batch_refuse(m3_batch* b, int code, int i, const char* msg) {
    char head[64];
    if (i >= 0) std::snprintf(head, sizeof(head), "m3_batch_command: handle %d: ", i);
    else std::snprintf(head, sizeof(head), "m3_batch_command: ");
    b->err = std::string(head) + msg;
    return code;
}

// sections: the M3_BATCH_SECTION_* bits of the batch that this call may use -- all of them for m3_batch_command; for a lockstep
// episode set those that its own flags allow as well (eps_sections, peps_sections), whatever batch it is handed
static int batch_command(m3_batch* b, m3_handle* const* hs, int n, float* actions_host, int sections) {
    // ---- every check before any launch: a refused call leaves every handle as it was ----
    if (!hs) return batch_refuse(b, M3_ERR_BAD_ARG, -1, "null handle list");
    if (n <= 0 || n > b->max_handles) return batch_refuse(b, M3_ERR_BAD_ARG, -1, "n must be in 1 .. max_handles");
    for (int i = 0; i < n; ++i) {
        if (!hs[i]) return batch_refuse(b, M3_ERR_BAD_ARG, i, "null handle");
        if (hs[i]->cfg.device != b->device) return batch_refuse(b, M3_ERR_BAD_ARG, i, "handle on another device than the batch");
        b->seen[i] = hs[i];
    }
    std::sort(b->seen.begin(), b->seen.begin() + n);
    if (std::adjacent_find(b->seen.begin(), b->seen.begin() + n) != b->seen.begin() + n) {
        for (int i = 1; i < n; ++i)
            for (int j = 0; j < i; ++j)
                if (hs[j] == hs[i]) return batch_refuse(b, M3_ERR_BAD_ARG, i, "handle listed twice");
    }
    const hipStream_t s = hs[0]->stream;
    const bool panda = hs[0]->cfg.env_type == M3_ENV_PANDA;   // one environment per call: handle 0's
    BatchHandle* hd = b->hd.data();
    for (int i = 0; i < n; ++i) {
        m3_handle* h = hs[i];
        if (h->cfg.env_type != hs[0]->cfg.env_type)
            return batch_refuse(b, M3_ERR_UNSUPPORTED, i, panda ? "point_env handle in a batch of panda_env handles (one environment per call)"
                                                                : "panda_env handle in a batch of point_env handles (one environment per call)");
        if (h->stream != s) return batch_refuse(b, M3_ERR_STATE, i, "its stream differs from handle 0's");
        int code;
        if (const char* why = batch_refusal(h, hd[i].u, code, sections)) return batch_refuse(b, code, i, why);
        BatchKey& k = hd[i].key;
        if (panda) hd[i].panda = panda_decision(panda_input(h), PANDA_SIDE_BATCH);   // (by m3_rollout's own dispatch)
        k.variant = panda ? panda_batch_key(hd[i].panda.variant) : 0;
        k.upd = update_small_instance(hd[i].u);
        hd[i].u.n_cand = k.upd.n_cand;   // (what launch_update_small hands its instance)
        k.K = h->cfg.K_local; k.T = h->cfg.T;
        b->by_roll[i] = b->by_upd[i] = i;
    }
    // ---- each handle's rollout, as m3_rollout plans it, in call order (+ its wave-order refresh when it is due: its own
    // launch on the stream, ahead of the batched rollout) ----
    for (int i = 0; i < n; ++i) {
        const int rc = plan_rollout(hs[i], hd[i].a, hd[i].pa, hd[i].key.roll);
        if (rc != M3_OK) { b->err = "m3_batch_command: " + hs[i]->err; return rc; }
        // (the run-time families are GENERAL builds only: the plan's choice of the literal kernel's build does not split a group)
        if (panda && panda_general_only(hd[i].panda.variant)) hd[i].key.roll.general = 1;
        // (one kernel family serves the handles with priors with and without an arena per sample -- the entry's rows say which:
        // the arena per sample does not split a group)
        if (!panda && hd[i].key.roll.priors) hd[i].key.roll.scene = 1;
    }
    // ---- groups: handles in key order (ties in call order) ----
    std::sort(b->by_roll.begin(), b->by_roll.begin() + n, [hd](int x, int y) {
        return less_rollout(hd[x].key, hd[y].key) || (!less_rollout(hd[y].key, hd[x].key) && x < y);
    });
    std::sort(b->by_upd.begin(), b->by_upd.begin() + n, [hd](int x, int y) {
        return less_update(hd[x].key, hd[y].key) || (!less_update(hd[y].key, hd[x].key) && x < y);
    });
    // ---- the argument table: a free ring slot, filled on the host, ONE copy ----
    const int slot = b->next;
    if (b->in_flight[slot]) {
        HIPCHK(b, hipEventSynchronize(b->done[slot]));
        b->in_flight[slot] = false;
    }
    // in key order the handles come by section, as the table's sections lie (rollout_fields: point_env priors, then scene 0 by
    // weighted, 1, 2; panda_env the variant)
    const BatchTableShape& shape = b->shape[panda];
    const BatchSection* sec = batch_sections(panda).sec;
    int count[BATCH_MAX_SECTIONS] = {};
    for (int i = 0; i < n; ++i) ++count[batch_section_of(panda, hd[i])];
    const BatchTableLayout lay = batch_table_layout(shape, count);
    // byte offset of the rollout entry of the p-th handle in key order
    auto entry_off = [&](int p) {
        int v = 0;
        for (; p >= count[v]; ++v) p -= count[v];
        return lay.off[v] + (size_t)p * shape.entry[v];
    };
    for (int p = 0; p < n; ++p) {
        const int i = b->by_roll[p];
        sec[batch_section_of(panda, hd[i])].fill(b->host[slot] + entry_off(p), hs[i], hd[i]);
    }
    UpdateArgs* hu = reinterpret_cast<UpdateArgs*>(b->host[slot] + lay.upd_off);
    for (int p = 0; p < n; ++p) hu[p] = hd[b->by_upd[p]].u;
    char* dslot = b->dev[slot];
    HIPCHK(b, hipMemcpyAsync(dslot, b->host[slot], lay.total, hipMemcpyHostToDevice, s));
    const UpdateArgs* du = reinterpret_cast<const UpdateArgs*>(dslot + lay.upd_off);
    // ---- one rollout launch per group (panda_env: + one k_panda_reach_cost launch when the group keeps the record buffer,
    // not counted) ----
    int n_roll = 0, n_upd = 0;
    // the ancillary controllers of the handles that have one fill their tables of priors from the worlds the rollouts are about
    // to start from: one launch over the priors section, ahead of the rollout launches (not counted)
    if (!panda && count[POINT_SECTION_PR] > 0) {
        bool any = false;
        for (int i = 0; i < n; ++i) {
            any = any || prior_controller_on(hs[i]);
            if (hd[i].key.roll.priors) hs[i]->priors.used = 1;   // (as m3_rollout records it)
        }
        if (any)
            launch_prior_controllers_batch(static_cast<const BatchRolloutEntryPR*>(static_cast<const void*>(dslot + lay.off[POINT_SECTION_PR])),
                                           count[POINT_SECTION_PR], s);
    }
    for (int p = 0; p < n;) {
        const BatchKey& k = hd[b->by_roll[p]].key;
        int q = p + 1;
        while (q < n && same_rollout(hd[b->by_roll[q]].key, k)) ++q;
        if (panda) launch_rollout_panda_batch(dslot + entry_off(p), q - p, hd[b->by_roll[p]].panda.variant, k.roll, k.K, s);
        else launch_rollout_point_batch(dslot + entry_off(p), q - p, k.roll, s);
        ++n_roll;
        p = q;
    }
    HIPCHK(b, hipGetLastError());
    // what each handle's rollout ran, as m3_rollout records it (a batch without the run-time section runs the literal kernels
    // only and leaves the record as it always did)
    if (panda && (sections & M3_BATCH_SECTION_PANDA_RUNTIME))
        for (int i = 0; i < n; ++i) panda_record_used(hs[i], hd[i].panda);
    // ---- one update launch per group; multi-modal groups in chunks whose whole grid is resident ----
    for (int p = 0; p < n;) {
        const BatchKey& k = hd[b->by_upd[p]].key;
        int q = p + 1;
        while (q < n && same_update(hd[b->by_upd[q]].key, k)) ++q;
        int chunk = q - p;
        if (k.upd.multi) {
            const int per_cu = k.upd.nu == 9 ? update_small9_batch_blocks_per_cu(k.upd) : update_small_batch_blocks_per_cu(k.upd);
            chunk = std::max(1, M3_CUS * per_cu / (k.T + k.upd.n_cand));
        }
        for (int r = p; r < q; r += chunk) {
            launch_update_small_batch(du + r, std::min(chunk, q - r), k.upd, k.T, s);
            ++n_upd;
        }
        p = q;
    }
    HIPCHK(b, hipGetLastError());
    // ---- per handle, as m3_update_finalize (without its timing events): the covariance step, the call count ----
    for (int i = 0; i < n; ++i) {
        const int rc = finish_command(hs[i], false);
        if (rc != M3_OK) { b->err = "m3_batch_command: " + hs[i]->err; return rc; }
    }
    HIPCHK(b, hipEventRecord(b->done[slot], s));
    b->in_flight[slot] = true;
    b->next = (slot + 1) % BATCH_SLOTS;
    b->rollout_launches = n_roll;
    b->update_launches = n_upd;
    if (actions_host) {   // the plans one after the other
        size_t off = 0;
        for (int i = 0; i < n; ++i) {
            const size_t len = plan_floats(hs[i]->cfg);
            HIPCHK(b, hipMemcpyAsync(actions_host + off, plan_dst(hs[i]), len * sizeof(float), hipMemcpyDeviceToHost, s));
            off += len;
        }
        HIPCHK(b, hipStreamSynchronize(s));
    }
    return M3_OK;
}

extern "C" int m3_batch_command(m3_batch* b, m3_handle* const* hs, int n, float* actions_host) {
    if (!b) { g_batch_err = "m3_batch_command: null batch"; return M3_ERR_BAD_ARG; }
    return batch_command(b, hs, n, actions_host, b->flags);
}

static int ensure_sim(m3_handle* h);
extern "C" int m3_record_b_len(const m3_handle* h) {
    if (!h || !update_second_record(h->protocol)) return 0;
    return recb_length(h->cfg.T, h->cfg.nu);
}

extern "C" int m3_record_len(const m3_handle* h) {
    if (!h) return 0;
    return update_costs_head_record(h->protocol) ? regen_record_length(h->cfg.K_local, h->cfg.T) : record_length(h->cfg.T, h->cfg.nu);
}

extern "C" int m3_get_buffer(m3_handle* h, int which, void** p, long long* nbytes) {
    if (!h || !p) return M3_ERR_BAD_ARG;
    if (which < 0 || which >= M3_BUF_COUNT) return fail(h, M3_ERR_BAD_ARG, "m3_get_buffer: unknown buffer id");
    if (which == M3_BUF_SIM_WORLD) {
        int rc = ensure_sim(h);
        if (rc != M3_OK) return rc;
        *p = h->sim_world;
        if (nbytes) *nbytes = (long long)(h->cfg.env_type == M3_ENV_POINT ? NW : NWP) * h->cfg.K_local * sizeof(float);
        return M3_OK;
    }
    if (which == M3_BUF_TRAJ_COST_ALL && !h->cfg.sim_only && h->cfg.K_local == h->cfg.K_global)
        which = M3_BUF_TRAJ_COST;  // unsharded: the local costs are the global costs
    if (!h->buf[which]) return fail(h, M3_ERR_STATE, "m3_get_buffer: buffer not allocated for this handle");
    *p = h->buf[which];
    if (nbytes) *nbytes = h->nbytes[which];
    return M3_OK;
}

extern "C" int m3_reduce_len(const m3_handle* h) {
    return h ? reduce_length(h->cfg.T, h->cfg.nu) : M3_ERR_BAD_ARG;
}

extern "C" int m3_get_info(m3_handle* h, m3_info* out) {
    if (!h || !out) return M3_ERR_BAD_ARG;
    HIPCHK(h, hipMemcpyAsync(out, h->buf[M3_BUF_INFO], sizeof(m3_info), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    out->calls = (int)h->calls;
    return M3_OK;
}

extern "C" int m3_get_timing(m3_handle* h, m3_timing* out) {
    if (!h || !out) return M3_ERR_BAD_ARG;
    if (!h->timing) return fail(h, M3_ERR_STATE, "m3_get_timing: timing not enabled");
    HIPCHK(h, hipEventSynchronize(h->ev[3]));
    HIPCHK(h, hipEventElapsedTime(&out->rollout_ms, h->ev[0], h->ev[1]));
    HIPCHK(h, hipEventElapsedTime(&out->update_ms, h->ev[1], h->ev[2]));
    HIPCHK(h, hipEventElapsedTime(&out->finalize_ms, h->ev[2], h->ev[3]));
    HIPCHK(h, hipEventElapsedTime(&out->total_ms, h->ev[0], h->ev[3]));
    return M3_OK;
}

// ---------------------------------- step mode ------------------------------------------
static int ensure_sim(m3_handle* h) {
    const m3_config& c = h->cfg;
    if (!h->sim_world) {
        const size_t nw = (c.env_type == M3_ENV_POINT) ? NW : NWP;
        BlockGroup g(h->mem);   // both or none: a failure leaves sim_world null, the next call tries again
        HIPCHK(h, own_device(h->mem, h->sim_world, nw * c.K_local * sizeof(float)));
        HIPCHK(h, hipMemsetAsync(h->sim_world, 0, nw * c.K_local * sizeof(float), h->stream));
        HIPCHK(h, own_device(h->mem, h->sim_u, (size_t)c.K_local * c.nu * sizeof(float)));
        HIPCHK(h, hipMemsetAsync(h->sim_u, 0, (size_t)c.K_local * c.nu * sizeof(float), h->stream));
        g.keep = true;
    }
    return M3_OK;
}

extern "C" int m3_sim_bind_views(m3_handle* h, float* dof, float* root, float* rb, float* ncf, int n_actors, int n_bodies) {
    if (!h) return M3_ERR_BAD_ARG;
    const bool point = h->cfg.env_type == M3_ENV_POINT;
    // actor tables of this build (DESIGN.md "Scene tables"), robot last (skill_utils.py:89-90):
    //   point_env: walls 0-3, obs 4, dyn-obs 5, box 6, goal 7, yaxis 8, xaxis 9, robot 10;
    //              bodies = actors 0..9 + plane 10, link_x 11, link_y 12
    //   panda_env: table 0, table_stand 1, shelf_stand 2, dyn-obs 3, cubeA 4, cubeB 5, panda 6;
    //              bodies = actors 0..5 + panda_link0..7, hand, leftfinger, rightfinger (6..16)
    if (point && (n_actors != 11 || n_bodies != 13)) return fail(h, M3_ERR_SHAPE, "m3_sim_bind_views: point_env has 11 actors / 13 bodies");
    if (!point && (n_actors != 7 || n_bodies != 17)) return fail(h, M3_ERR_SHAPE, "m3_sim_bind_views: panda_env has 7 actors / 17 bodies");
    int rc = ensure_sim(h);
    if (rc != M3_OK) return rc;
    SimViews& v = h->views;
    v.dof_state = dof; v.root_state = root; v.rigid_body_state = rb; v.net_contact_force = ncf;
    v.n_actors = n_actors; v.n_bodies = n_bodies;
    if (point) {
        v.box_actor = 6; v.dyn_actor = 5; v.robot_actor = 10;
        v.box_body = 6; v.dyn_body = 5; v.robot_body = 12;
        v.table_body = v.shelf_body = 0;
    } else {
        v.box_actor = 4; v.dyn_actor = 5; v.robot_actor = 6;  // cubeA, cubeB, panda
        v.box_body = 4; v.dyn_body = 5; v.robot_body = 6;
        v.table_body = 0; v.shelf_body = 2;
        v.obs_actor = 3; v.obs_body = 3;
    }
    h->views_bound = true;
    return M3_OK;
}

extern "C" int m3_sim_pull_state(m3_handle* h) {
    if (!h) return M3_ERR_BAD_ARG;
    if (!h->views_bound || !h->views.dof_state || !h->views.root_state) return fail(h, M3_ERR_STATE, "m3_sim_pull_state: views not bound");
    if (const char* why = panda_refusal(h, PANDA_SIDE_VIEWS)) return fail(h, M3_ERR_STATE, (std::string("m3_sim_pull_state: ") + why).c_str());
    if (h->cfg.env_type == M3_ENV_POINT) launch_sim_pull(h->views, h->sim_world, h->cfg.K_local, h->stream);
    else launch_psim_pull(panda_launch_scene(h, panda_decision(panda_input(h), PANDA_SIDE_VIEWS).variant), h->views, h->sim_world, h->cfg.K_local, h->stream);
    HIPCHK(h, hipGetLastError());
    return M3_OK;
}

extern "C" int m3_sim_shift_actor(m3_handle* h, int actor, float dx, float dy, float dz) {
    if (!h) return M3_ERR_BAD_ARG;
    if (!h->views_bound) return fail(h, M3_ERR_STATE, "m3_sim_shift_actor: views not bound");
    if (h->cfg.env_type != M3_ENV_POINT) return fail(h, M3_ERR_UNSUPPORTED, "m3_sim_shift_actor: point_env (its dyn-obs walks; the panda_env's offset is zero)");
    if (actor < 0 || actor >= h->views.n_actors) return fail(h, M3_ERR_SHAPE, "m3_sim_shift_actor: actor index out of range");
    launch_sim_shift_pull(h->views, h->sim_world, h->cfg.K_local, actor, dx, dy, dz, h->stream);
    HIPCHK(h, hipGetLastError());
    return M3_OK;
}

extern "C" int m3_sim_push_state(m3_handle* h) {
    if (!h) return M3_ERR_BAD_ARG;
    if (!h->views_bound) return fail(h, M3_ERR_STATE, "m3_sim_push_state: views not bound");
    if (const char* why = panda_refusal(h, PANDA_SIDE_VIEWS)) return fail(h, M3_ERR_STATE, (std::string("m3_sim_push_state: ") + why).c_str());
    if (h->cfg.env_type == M3_ENV_POINT) launch_sim_push(h->views, h->sim_world, h->cfg.K_local, h->stream);
    else launch_psim_push(panda_launch_scene(h, panda_decision(panda_input(h), PANDA_SIDE_VIEWS).variant), h->views, h->sim_world, h->cfg.K_local, h->stream);
    HIPCHK(h, hipGetLastError());
    return M3_OK;
}

extern "C" int m3_sim_set_velocity_target(m3_handle* h, const float* u) {
    if (!h || !u) return M3_ERR_BAD_ARG;
    int rc = ensure_sim(h);
    if (rc != M3_OK) return rc;
    HIPCHK(h, hipMemcpyAsync(h->sim_u, u, (size_t)h->cfg.K_local * h->cfg.nu * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    return M3_OK;
}

extern "C" int m3_sim_apply_body_forces(m3_handle* h, const float* f) {
    if (!h || !f) return M3_ERR_BAD_ARG;
    if (!h->views_bound) return fail(h, M3_ERR_STATE, "m3_sim_apply_body_forces: views not bound");
    if (h->cfg.env_type != M3_ENV_POINT)
        return fail(h, M3_ERR_UNSUPPORTED, "m3_sim_apply_body_forces: the panda_env path applies no body forces (only get_pull_cost does, point_env)");
    launch_sim_forces(h->views, h->sim_world, f, h->cfg.K_local, h->stream);
    HIPCHK(h, hipGetLastError());
    return M3_OK;
}

static int sim_step_impl(m3_handle* h, const float* u) {
    if (!h->views_bound) return fail(h, M3_ERR_STATE, "m3_sim_step: views not bound");
    if (h->cfg.env_type == M3_ENV_POINT) {
        if (const char* why = point_variant_refusal(h, SIDE_STEP)) return fail(h, M3_ERR_STATE, (std::string("m3_sim_step: ") + why).c_str());
        const int Kl = h->cfg.K_local;
        switch (point_step_variant(h)) {
            case STEP_ROWS: launch_sim_step_sv(h->scene_rt, h->point_rows.dev, h->views, h->sim_world, u, h->sim_u, Kl, h->stream); break;
            case STEP_RUNTIME: launch_sim_step_s(h->scene_rt, h->views, h->sim_world, u, h->sim_u, Kl, h->stream); break;
            default: launch_sim_step(h->scene, h->views, h->sim_world, u, h->sim_u, Kl, h->stream); break;
        }
    } else {
        const PandaDecision d = panda_decision(panda_input(h), PANDA_SIDE_STEP);
        if (const char* why = panda_refusal_text(d.refusal)) return fail(h, M3_ERR_STATE, (std::string("m3_sim_step: ") + why).c_str());
        panda_record_used(h, d);
        launch_psim_step(panda_launch_scene(h, d.variant), h->views, h->sim_world, u, h->sim_u, h->cfg.K_local, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return M3_OK;
}

extern "C" int m3_sim_step(m3_handle* h) {
    if (!h) return M3_ERR_BAD_ARG;
    return sim_step_impl(h, h->sim_u);
}

extern "C" int m3_sim_step_with_target(m3_handle* h, const float* u) {
    if (!h || !u) return M3_ERR_BAD_ARG;
    return sim_step_impl(h, u);
}

static int suction_impl(m3_handle* h, float kp, const float* action, int apply, float* forces, int* flags,
                        const int* gate) {
    if (!h) return M3_ERR_BAD_ARG;
    if (h->cfg.env_type != M3_ENV_POINT) return fail(h, M3_ERR_UNSUPPORTED, "suction is a point_env skill (skill_utils.py:36-94)");
    if (!h->views_bound || !h->sim_world) return fail(h, M3_ERR_STATE, "suction: views not bound");
    const float thresh = (h->cfg.K_local == 1) ? 1.5f : 1.8f;   // skill_utils.py:75-82 (sim.num_envs == 1: real world)
    launch_sim_suction(h->views, h->sim_world, h->cfg.K_local, kp, thresh, 0.6f /* skill_utils.py:56 */, action, apply,
                       forces, flags, gate, h->stream);
    HIPCHK(h, hipGetLastError());
    return M3_OK;
}

extern "C" int m3_sim_suction_forces(m3_handle* h, float kp_suction, float* forces_dev) {
    if (!forces_dev) return fail(h, M3_ERR_BAD_ARG, "m3_sim_suction_forces: null argument");
    return suction_impl(h, kp_suction, nullptr, 0, forces_dev, nullptr, nullptr);
}

extern "C" int m3_sim_check_and_apply_suction(m3_handle* h, const float* action_dev, float kp_suction, int apply,
                                              int* applied_dev, const int* enabled_dev) {
    if (!action_dev) return fail(h, M3_ERR_BAD_ARG, "m3_sim_check_and_apply_suction: null argument");
    return suction_impl(h, kp_suction, action_dev, apply, nullptr, applied_dev, enabled_dev);
}

extern "C" int m3_cost(m3_handle* h, float* cost) {
    if (!h || !cost) return M3_ERR_BAD_ARG;
    if (!h->sim_world) return fail(h, M3_ERR_STATE, "m3_cost: step-mode state not initialised");
    if (h->cfg.env_type == M3_ENV_POINT) {
        if (const char* why = point_variant_refusal(h, SIDE_COST)) return fail(h, M3_ERR_STATE, (std::string("m3_cost: ") + why).c_str());
        CostParams cp;
        fill_cost_params(h, cp);
        const PointCostWeights* wt = point_variant(h, SIDE_COST) == POINT_WEIGHTED ? &h->cost_weights : nullptr;
        launch_sim_cost(cp, wt, h->sim_world, h->cfg.K_local, h->cfg.k_offset, cost, h->stream);
    } else {
        PandaCostParams cp;
        fill_panda_cost_params(h, cp);
        // quirk Q8 exactly where m3_rollout applies it (its shadow lanes): reach on an unsharded handle
        const bool env0_cube = cp.task == 4 && h->cfg.k_offset == 0 && h->cfg.K_local == h->cfg.K_global && h->cfg.K_global >= 2;
        const PandaDecision d = panda_decision(panda_input(h), PANDA_SIDE_COST);
        if (const char* why = panda_refusal_text(d.refusal)) return fail(h, M3_ERR_STATE, (std::string("m3_cost: ") + why).c_str());
        panda_record_used(h, d);
        launch_psim_cost(panda_launch_scene(h, d.variant), cp, h->sim_world, h->cfg.K_local, h->cfg.k_offset, env0_cube, cost, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return M3_OK;
}

// ---------------------------------- batched closed-loop episodes ------------------------------------
// N episodes of tools/closed_loop.run (point_env) in lockstep: the world handle's N rows are the episodes' 1-env worlds
// (DESIGN.md §7c).  Per tick: k_episodes_pre, m3_batch_command of the running episodes' planners, k_episodes_post, one
// copy of the status words, one synchronisation.
static thread_local std::string g_eps_err;

struct m3_episodes {
    m3_handle* world = nullptr;
    int n = 0, max_ticks = 0, tick = 0;
    int flags = 0;                   // m3_episodes_create_ex's (M3_EPISODES_ROLLOUT_SCENES, M3_EPISODES_PRIORS)
    bool mid_tick = false;           // between m3_episodes_begin and m3_episodes_end
    std::string err;
    std::vector<m3_handle*> planners;
    std::vector<const float*> plan;  // each planner's action-out, fixed at create
    std::vector<m3_handle*> live;    // scratch: this tick's batch
    OwnedBlocks mem{&m3_release_block, 3};   // owns the three blocks; dev, trace and host are views
    char* dev = nullptr;             // lanes | status | gates
    float* trace = nullptr;
    m3_episode_status* host = nullptr;   // pinned copy of the status words
    m3::EpisodeArgs args{};
};

extern "C" const char* m3_episodes_last_error(const m3_episodes* eps) { return eps ? eps->err.c_str() : g_eps_err.c_str(); }

extern "C" void m3_episodes_destroy(m3_episodes* eps) {
    if (!eps) return;
    if (eps->world) (void)hipStreamSynchronize(eps->world->stream);   // (kernels may still use the memory)
    eps->mem.release_all();
    delete eps;
}

static int eps_refuse(int code, int i, const std::string& msg) {
    char head[64];
    if (i >= 0) std::snprintf(head, sizeof(head), "m3_episodes_create: planner %d: ", i);
    else std::snprintf(head, sizeof(head), "m3_episodes_create: ");
    g_eps_err = std::string(head) + msg;
    return code;
}

extern "C" int m3_episodes_create(m3_handle* world, m3_handle* const* planners, const m3_episode_spec* specs, int n,
                                  int max_ticks, int trace, m3_episodes** out) {
    return m3_episodes_create_ex(world, planners, specs, n, max_ticks, trace, 0, out);
}

extern "C" int m3_episodes_flags(const m3_episodes* eps) { return eps ? eps->flags : M3_ERR_BAD_ARG; }

// the sections of a batch that a set created with `flags` may use: the per-sample section with M3_EPISODES_ROLLOUT_SCENES
// (planners with an arena per sample pass), the priors section with M3_EPISODES_PRIORS (planners with prior samples pass); the
// panda run-time section means nothing to point_env planners and is left to the batch
static int eps_sections(int flags) {
    return M3_BATCH_SECTION_PANDA_RUNTIME | ((flags & M3_EPISODES_ROLLOUT_SCENES) ? M3_BATCH_SECTION_POINT_ROLLOUT_SCENES : 0) |
           ((flags & M3_EPISODES_PRIORS) ? M3_BATCH_SECTION_POINT_PRIORS : 0);
}

// (the messages keep m3_episodes_create's name: flags == 0 is that call)
extern "C" int m3_episodes_create_ex(m3_handle* world, m3_handle* const* planners, const m3_episode_spec* specs, int n,
                                     int max_ticks, int trace, int flags, m3_episodes** out) {
    if (out) *out = nullptr;
    if (flags & ~(M3_EPISODES_ROLLOUT_SCENES | M3_EPISODES_PRIORS)) { g_eps_err = "m3_episodes_create_ex: unknown flag bits"; return M3_ERR_BAD_ARG; }
    if (!out) return eps_refuse(M3_ERR_BAD_ARG, -1, "null argument");
    // ---- every check before any allocation or launch ----
    if (!world || !planners || !specs) return eps_refuse(M3_ERR_BAD_ARG, -1, "null argument");
    if (n <= 0 || n > 65535) return eps_refuse(M3_ERR_BAD_ARG, -1, "n must be in 1 .. 65535");
    if (max_ticks <= 0) return eps_refuse(M3_ERR_BAD_ARG, -1, "max_ticks must be > 0");
    const m3_config& wc = world->cfg;
    if (wc.env_type != M3_ENV_POINT || !wc.sim_only || !world->views_bound || !world->sim_world || !world->views.dof_state ||
        !world->views.root_state || !world->views.rigid_body_state || !world->views.net_contact_force)
        return eps_refuse(M3_ERR_STATE, -1, "the world must be a sim_only point_env handle with all four views bound");
    if (wc.K_local != n || wc.K_global != n) return eps_refuse(M3_ERR_STATE, -1, "the world's K_local must equal n (one row per episode)");
    for (int i = 0; i < n; ++i) {
        m3_handle* h = planners[i];
        if (!h) return eps_refuse(M3_ERR_BAD_ARG, i, "null handle");
        if (h == world) return eps_refuse(M3_ERR_BAD_ARG, i, "the world handle is listed as a planner");
        for (int j = 0; j < i; ++j)
            if (planners[j] == h) return eps_refuse(M3_ERR_BAD_ARG, i, "handle listed twice");
        const m3_config& c = h->cfg;
        if (c.env_type != M3_ENV_POINT) return eps_refuse(M3_ERR_UNSUPPORTED, i, "panda_env planner (point_env episodes only)");
        if (c.device != wc.device) return eps_refuse(M3_ERR_BAD_ARG, i, "handle on another device than the world");
        if (h->stream != world->stream) return eps_refuse(M3_ERR_STATE, i, "its stream differs from the world's");
        UpdateArgs u;
        int code;
        if (const char* why = batch_refusal(h, u, code, eps_sections(flags))) return eps_refuse(code, i, why);
        if (!h->action_out) return eps_refuse(M3_ERR_STATE, i, "no action-out destination (m3_set_action_out)");
        const m3_episode_spec& sp = specs[i];
        if (sp.task < M3_TASK_NAVIGATION || sp.task > M3_TASK_PUSH_PULL) return eps_refuse(M3_ERR_BAD_ARG, i, "spec: task is not a point_env task");
        if (sp.suction < M3_SUCTION_OFF || sp.suction > M3_SUCTION_PULL_PREFERENCE) return eps_refuse(M3_ERR_BAD_ARG, i, "spec: unknown suction mode");
        if (sp.suction == M3_SUCTION_PULL_PREFERENCE && !c.multi_modal)
            return eps_refuse(M3_ERR_STATE, i, "spec: suction from the pull preference needs a multi-modal planner");
        if (sp.dyn_phase < 0) return eps_refuse(M3_ERR_BAD_ARG, i, "spec: dyn_phase must be >= 0");
    }
    // ---- allocations: all of the set's memory, here ----
    m3_episodes* eps = new (std::nothrow) m3_episodes();
    if (!eps) return eps_refuse(M3_ERR_HIP, -1, "out of host memory");
    try {
        eps->planners.assign(planners, planners + n);
        eps->plan.resize(n);
        eps->live.reserve(n);
    } catch (...) {
        delete eps;
        return eps_refuse(M3_ERR_HIP, -1, "out of host memory");
    }
    eps->world = world;
    eps->n = n;
    eps->max_ticks = max_ticks;
    eps->flags = flags;
    const size_t lane_b = align16((size_t)n * sizeof(m3::EpisodeLane));
    const size_t st_b = align16((size_t)n * sizeof(m3_episode_status));
    const size_t gate_b = align16((size_t)n * sizeof(int));
    std::vector<m3::EpisodeLane> lanes(n);
    std::vector<m3_episode_status> st0(n);
    for (int i = 0; i < n; ++i) {
        m3_handle* h = planners[i];
        const m3_episode_spec& sp = specs[i];
        m3::EpisodeLane& L = lanes[i];
        L.task = sp.task; L.phase = sp.dyn_phase; L.suction = sp.suction;
        L.gx = sp.goal[0]; L.gy = sp.goal[1]; L.kp = sp.kp_suction;
        L.pref = sp.suction == M3_SUCTION_PULL_PREFERENCE
                     ? (const int*)((const char*)h->buf[M3_BUF_INFO] + offsetof(m3_info, pull_preference)) : nullptr;
        L.plan = eps->plan[i] = h->action_out;
        st0[i].done_tick = -1; st0[i].success = 0; st0[i].collision_ticks = 0;
        st0[i].final_pos[0] = st0[i].final_pos[1] = 0.0f;
    }
    const hipStream_t s = world->stream;
    hipError_t e = own_device(eps->mem, eps->dev, lane_b + st_b + gate_b);
    if (e == hipSuccess && trace) e = own_device(eps->mem, eps->trace, (size_t)max_ticks * n * 10 * sizeof(float));
    if (e == hipSuccess) e = own_pinned(eps->mem, eps->host, (size_t)n * sizeof(m3_episode_status), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemcpyAsync(eps->dev, lanes.data(), (size_t)n * sizeof(m3::EpisodeLane), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(eps->dev + lane_b, st0.data(), (size_t)n * sizeof(m3_episode_status), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(eps->dev + lane_b + st_b, 0, gate_b, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // (the host vectors above go out of scope)
    if (e != hipSuccess) {
        m3_episodes_destroy(eps);
        return eps_refuse(M3_ERR_HIP, -1, hipGetErrorString(e));
    }
    std::memcpy(eps->host, st0.data(), (size_t)n * sizeof(m3_episode_status));
    m3::EpisodeArgs& a = eps->args;
    a.v = world->views;
    a.world = world->sim_world;
    a.n = n;
    a.last_tick = max_ticks - 1;
    a.lane = reinterpret_cast<const m3::EpisodeLane*>(eps->dev);
    a.st = reinterpret_cast<m3_episode_status*>(eps->dev + lane_b);
    a.gate = reinterpret_cast<int*>(eps->dev + lane_b + st_b);
    a.trace = eps->trace;
    *out = eps;
    return M3_OK;
}

static int eps_ready(m3_episodes* eps, const char* who) {
    if (eps->tick >= eps->max_ticks) { eps->err = std::string(who) + ": all max_ticks ticks are done"; return M3_ERR_STATE; }
    for (int i = 0; i < eps->n; ++i)
        if (eps->planners[i]->action_out != eps->plan[i]) {
            eps->err = std::string(who) + ": planner " + std::to_string(i) + "'s action-out destination changed since create";
            return M3_ERR_STATE;
        }
    return M3_OK;
}

// the step of the world's rows with the WORLD handle's scene (the planners plan with their own)
static void episodes_post(const m3_handle* w, const m3::EpisodeArgs& a, int tick) {
    switch (point_step_variant(w)) {
        case STEP_ROWS: m3::launch_episodes_post_sv(w->scene_rt, w->point_rows.dev, a, tick, w->stream); break;   // a scene per episode
        case STEP_RUNTIME: m3::launch_episodes_post_s(w->scene_rt, a, tick, w->stream); break;
        default: m3::launch_episodes_post(w->scene, a, tick, w->stream); break;
    }
}

static int eps_status_sync(m3_episodes* eps) {
    const hipStream_t s = eps->world->stream;
    HIPCHK(eps, hipMemcpyAsync(eps->host, eps->args.st, (size_t)eps->n * sizeof(m3_episode_status), hipMemcpyDeviceToHost, s));
    HIPCHK(eps, hipStreamSynchronize(s));
    return M3_OK;
}

// a planner that got prior samples after m3_episodes_create (which refuses it): nothing of the tick is launched.  A set created
// with M3_EPISODES_PRIORS takes such planners
static int eps_priors_refusal(m3_episodes* eps, const char* who) {
    for (int i = 0; i < eps->n; ++i)   // (likewise sample groups, which no set takes)
        if (eps->planners[i]->groups.n > 0) {
            eps->err = std::string(who) + ": planner " + std::to_string(i) + ": " + SAMPLE_GROUPS_UNBATCHED;
            return M3_ERR_UNSUPPORTED;
        }
    if (eps->flags & M3_EPISODES_PRIORS) return M3_OK;
    for (int i = 0; i < eps->n; ++i)
        if (eps->planners[i]->priors.n > 0) {
            eps->err = std::string(who) + ": planner " + std::to_string(i) + ": " + PRIORS_UNBATCHED;
            return M3_ERR_UNSUPPORTED;
        }
    return M3_OK;
}

extern "C" int m3_episodes_begin(m3_episodes* eps) {
    if (!eps) return M3_ERR_BAD_ARG;
    if (eps->mid_tick) { eps->err = "m3_episodes_begin: the tick was begun already"; return M3_ERR_STATE; }
    int rc = eps_ready(eps, "m3_episodes_begin");
    if (rc != M3_OK) return rc;
    if ((rc = eps_priors_refusal(eps, "m3_episodes_begin")) != M3_OK) return rc;
    m3::launch_episodes_pre(eps->args, eps->tick, eps->world->stream);
    HIPCHK(eps, hipGetLastError());
    eps->mid_tick = true;
    return eps_status_sync(eps);
}

extern "C" int m3_episodes_end(m3_episodes* eps) {
    if (!eps) return M3_ERR_BAD_ARG;
    if (!eps->mid_tick) { eps->err = "m3_episodes_end: no tick begun"; return M3_ERR_STATE; }
    int rc = eps_ready(eps, "m3_episodes_end");
    if (rc != M3_OK) return rc;
    if ((rc = eps_priors_refusal(eps, "m3_episodes_end")) != M3_OK) return rc;
    if (const char* why = point_variant_refusal(eps->world, SIDE_STEP)) { eps->err = std::string("m3_episodes_end: world: ") + why; return M3_ERR_STATE; }
    episodes_post(eps->world, eps->args, eps->tick);
    HIPCHK(eps, hipGetLastError());
    eps->mid_tick = false;
    eps->tick += 1;
    return eps_status_sync(eps);
}

extern "C" int m3_episodes_tick(m3_episodes* eps, m3_batch* batch) {
    if (!eps) return M3_ERR_BAD_ARG;
    if (!batch) { eps->err = "m3_episodes_tick: null batch"; return M3_ERR_BAD_ARG; }
    if (eps->mid_tick) { eps->err = "m3_episodes_tick: inside m3_episodes_begin / m3_episodes_end"; return M3_ERR_STATE; }
    int rc = eps_ready(eps, "m3_episodes_tick");
    if (rc != M3_OK) return rc;
    if ((rc = eps_priors_refusal(eps, "m3_episodes_tick")) != M3_OK) return rc;
    if (const char* why = point_variant_refusal(eps->world, SIDE_STEP)) { eps->err = std::string("m3_episodes_tick: world: ") + why; return M3_ERR_STATE; }
    // the batch: episodes still running after the last tick's status (one that succeeds in this tick's pre kernel is
    // commanded once more -- its plan is never recorded)
    eps->live.clear();
    const m3_handle* w = eps->world;
    const int allowed = eps_sections(eps->flags);
    for (int i = 0; i < eps->n; ++i) {
        if (eps->host[i].done_tick >= 0) continue;
        m3_handle* h = eps->planners[i];
        // (a set created for planners with priors, a batch without the section: the batch's own refusal, ahead of the pre kernel)
        if (h->priors.n > 0 && !(batch->flags & M3_BATCH_SECTION_POINT_PRIORS)) {
            rc = batch_refuse(batch, M3_ERR_UNSUPPORTED, (int)eps->live.size(), PRIORS_UNBATCHED);
            eps->err = std::string("m3_episodes_tick: ") + m3_batch_last_error(batch);
            return rc;
        }
        const bool in_priors_section = h->priors.n > 0 && (allowed & M3_BATCH_SECTION_POINT_PRIORS);   // (its entry carries the rows as well)
        if (h->point_rows.sample_on && !(allowed & M3_BATCH_SECTION_POINT_ROLLOUT_SCENES) && !in_priors_section) {   // (set after m3_episodes_create, which refuses it: nothing of this tick is launched)
            eps->err = "m3_episodes_tick: planner " + std::to_string(i) + ": " + POINT_ROWS_UNBATCHED;
            return M3_ERR_UNSUPPORTED;
        }
        // (a set created for such planners, a batch without the section: the batch's own refusal, ahead of the pre kernel)
        if (h->point_rows.sample_on && !in_priors_section && !(batch->flags & M3_BATCH_SECTION_POINT_ROLLOUT_SCENES)) {
            rc = batch_refuse(batch, M3_ERR_UNSUPPORTED, (int)eps->live.size(), POINT_ROWS_UNBATCHED);
            eps->err = std::string("m3_episodes_tick: ") + m3_batch_last_error(batch);
            return rc;
        }
        // (f) planner i reads row i of the world: the rollout takes row 0 of its bound views
        // (rollout_point_kernel.hpp), so it sees the floats closed_loop.run copies into its K-env sim
        rc = m3_bind_sim_point(h, w->views.dof_state + (size_t)i * 4, w->views.root_state + (size_t)i * w->views.n_actors * 13,
                               w->views.n_actors, w->views.box_actor, w->views.dyn_actor);
        if (rc != M3_OK) { eps->err = "m3_episodes_tick: " + h->err; return rc; }
        eps->live.push_back(h);
    }
    m3::launch_episodes_pre(eps->args, eps->tick, w->stream);
    HIPCHK(eps, hipGetLastError());
    if (!eps->live.empty()) {
        // (a set created without a flag never uses that section, whatever batch it is handed)
        rc = batch_command(batch, eps->live.data(), (int)eps->live.size(), nullptr, batch->flags & allowed);
        if (rc != M3_OK) { eps->err = std::string("m3_episodes_tick: ") + m3_batch_last_error(batch); return rc; }
    }
    episodes_post(w, eps->args, eps->tick);
    HIPCHK(eps, hipGetLastError());
    eps->tick += 1;
    return eps_status_sync(eps);
}

extern "C" int m3_episodes_ticks_done(const m3_episodes* eps) { return eps ? eps->tick : M3_ERR_BAD_ARG; }

extern "C" int m3_episodes_running(const m3_episodes* eps) {
    if (!eps) return M3_ERR_BAD_ARG;
    int r = 0;
    for (int i = 0; i < eps->n; ++i) r += eps->host[i].done_tick < 0;
    return r;
}

extern "C" int m3_episodes_status(m3_episodes* eps, m3_episode_status* status_out, float* trace_out) {
    if (!eps || !status_out) return M3_ERR_BAD_ARG;
    const hipStream_t s = eps->world->stream;
    HIPCHK(eps, hipMemcpyAsync(status_out, eps->args.st, (size_t)eps->n * sizeof(m3_episode_status), hipMemcpyDeviceToHost, s));
    if (trace_out) {
        if (!eps->trace) { eps->err = "m3_episodes_status: the set was created without a trace"; return M3_ERR_STATE; }
        HIPCHK(eps, hipMemcpyAsync(trace_out, eps->trace, (size_t)eps->max_ticks * eps->n * 10 * sizeof(float),
                                 hipMemcpyDeviceToHost, s));
    }
    HIPCHK(eps, hipStreamSynchronize(s));
    return M3_OK;
}

// ---------------------------------- batched closed-loop episodes, panda_env ------------------------------------
// N reactive pick-and-place episodes of tools/closed_loop.run in lockstep.  The task planner stays on the
// host, so a tick is two calls: m3_panda_episodes_observe (pre kernel, one copy, one synchronisation), the host's task
// planners, m3_panda_episodes_act (bind, one batched command, post kernel; no synchronisation).
static thread_local std::string g_peps_err;

struct m3_panda_episodes {
    m3_handle* world = nullptr;
    int n = 0, max_ticks = 0, settle_ticks = 0, tick = 0;
    bool observed = false;           // between observe and act
    std::string err;
    std::vector<m3_handle*> planners;
    std::vector<const float*> plan;  // each planner's action-out, fixed at create
    std::vector<m3_handle*> live;    // scratch: this tick's batch
    std::vector<m3_panda_episode_status> mirror;   // the device's status words, advanced on the host by the same pe_advance
    OwnedBlocks mem{&m3_release_block, 7};   // owns the blocks; dev, trace, pinned and the tables are views (and the three below into them)
    char* dev = nullptr;             // status | plan pointers | kept targets | ended | planning view: dof, root, rigid bodies
    float* trace = nullptr;
    char* pinned = nullptr;          // rigid-body rows of the planning view | ended
    size_t rb_bytes = 0;
    // M3_PANDA_EPISODES_RUNTIME (m3_panda_episodes_create_ex): the two workspace tables [PANDA_SCENE_ROW_WORDS][n]
    // (panda_episode_tables.hpp), index 0 the planning side (row e: planner e's workspace), 1 the world side (row e: the
    // workspace of row e of the world).  Each has its device table, its pinned mirror and the host's copy of the scenes the
    // mirror was packed from; all from create, null / empty without the flag
    int flags = 0;
    float* rows_dev[2] = {};
    float* rows_pinned[2] = {};
    std::vector<m3_panda_scene> rows_kept[2];
    bool rows_fresh[2] = {true, true};   // nothing packed yet: the next refresh packs every row
    int* ended_pinned = nullptr;
    int* ended_dev = nullptr;
    float* kept_dev = nullptr;
    m3::PandaEpisodeArgs args{};
};

extern "C" const char* m3_panda_episodes_last_error(const m3_panda_episodes* eps) {
    return eps ? eps->err.c_str() : g_peps_err.c_str();
}

extern "C" void m3_panda_episodes_destroy(m3_panda_episodes* eps) {
    if (!eps) return;
    if (eps->world) (void)hipStreamSynchronize(eps->world->stream);   // (kernels may still use the memory)
    eps->mem.release_all();
    delete eps;
}

static int peps_refuse(int code, int i, const std::string& msg) {
    char head[64];
    if (i >= 0) std::snprintf(head, sizeof(head), "m3_panda_episodes_create: planner %d: ", i);
    else std::snprintf(head, sizeof(head), "m3_panda_episodes_create: ");
    g_peps_err = std::string(head) + msg;
    return code;
}

// the mode of a set, and which workspace each of its rows runs in: the planning side's row e is what row 0 of planner e's own
// simulator steps in -- row 0 of its per-sample rows when it has them (the simulator's environment 0), else its single scene,
// which _bind_world pushes from the simulator it follows; the world side's row e is scenes[e] of m3_set_panda_scene_rows, else
// the world's single scene
static PandaEpisodesMode peps_mode(int flags) { return (flags & M3_PANDA_EPISODES_RUNTIME) ? PANDA_EPISODES_RUNTIME : PANDA_EPISODES_LITERAL; }
// the sections of a batch that a set created with `flags` may use: a run-time set hands its planners to the run-time section;
// a set created without the flag never uses it -- its planners and world stay on the compiled-in workspace and the literal
// cost, whatever batch they are handed
static int peps_sections(int flags) { return peps_mode(flags) == PANDA_EPISODES_RUNTIME ? M3_BATCH_SECTION_PANDA_RUNTIME : 0; }
static const m3_panda_scene& peps_planner_scene(const m3_handle* h) { return h->panda_rows.sample_on ? h->panda_rows.set[0] : h->panda_scene; }
static const m3_panda_scene& peps_world_scene(const m3_handle* w, int e) { return w->panda_rows.env_on ? w->panda_rows.set[e] : w->panda_scene; }

// Table `side` (0 planning, 1 world) of a run-time set from the handles' current state, on the world's stream: the rows whose
// workspace changed since the last refresh are packed into the pinned mirror again (make_panda_scene_rt on the host) and the
// table is uploaded in one copy; nothing changed: no copy.  No allocation, no synchronisation.  The pinned mirror is free to
// rewrite: the last copy from it was enqueued by an earlier observe (planning side) or act (world side), and every tick's
// observe has synchronised the stream since -- the planning side is refreshed BEFORE this tick's observe synchronises and after
// the previous tick's did, the world side after this tick's (tick 0: nothing was in flight but create's own copy, which create
// waited for).
static hipError_t peps_refresh_rows(m3_panda_episodes* eps, int side) {
    const m3_handle* w = eps->world;
    const int n = eps->n;
    const int packed = panda_episode_table_refresh(eps->rows_pinned[side], eps->rows_kept[side].data(), eps->rows_fresh[side], n,
                                                   w->cfg.dt, w->cfg.substeps, [&](int e) -> const m3_panda_scene& {
                                                       return side == 0 ? peps_planner_scene(eps->planners[e]) : peps_world_scene(w, e);
                                                   });
    eps->rows_fresh[side] = false;
    if (packed == 0) return hipSuccess;
    return hipMemcpyAsync(eps->rows_dev[side], eps->rows_pinned[side], (size_t)PANDA_SCENE_ROW_WORDS * n * sizeof(float),
                          hipMemcpyHostToDevice, w->stream);
}
static PandaEpisodesLaunchScene peps_launch_scene(const m3_panda_episodes* eps) {
    return {panda_episodes_variant(peps_mode(eps->flags)), &eps->world->pscene, &eps->world->pscene_rt, eps->rows_dev[0], eps->rows_dev[1]};
}

// (the messages keep m3_panda_episodes_create's name: flags == 0 is that call)
static int peps_create(m3_handle* world, m3_handle* const* planners, int n, int max_ticks, int settle_ticks, int trace, int flags,
                       m3_panda_episodes** out) {
    if (!out) return peps_refuse(M3_ERR_BAD_ARG, -1, "null argument");
    *out = nullptr;
    const PandaEpisodesMode mode = peps_mode(flags);
    // ---- every check before any allocation or launch ----
    if (!world || !planners) return peps_refuse(M3_ERR_BAD_ARG, -1, "null argument");
    if (n <= 0 || n > 65535) return peps_refuse(M3_ERR_BAD_ARG, -1, "n must be in 1 .. 65535");
    if (max_ticks <= 0) return peps_refuse(M3_ERR_BAD_ARG, -1, "max_ticks must be > 0");
    if (settle_ticks < 0) return peps_refuse(M3_ERR_BAD_ARG, -1, "settle_ticks must be >= 0");
    const m3_config& wc = world->cfg;
    if (wc.env_type != M3_ENV_PANDA || !wc.sim_only || !world->views_bound || !world->sim_world || !world->views.dof_state ||
        !world->views.root_state || !world->views.rigid_body_state)
        return peps_refuse(M3_ERR_STATE, -1, "the world must be a sim_only panda_env handle with its views bound");
    if (wc.K_local != n || wc.K_global != n) return peps_refuse(M3_ERR_STATE, -1, "the world's K_local must equal n (one row per episode)");
    // (the world is sim_only: its step reads no weight, and none is asked about)
    if (const char* why = panda_refusal(world, PANDA_SIDE_STEP)) return peps_refuse(M3_ERR_STATE, -1, std::string("the world: ") + why);
    {
        int code = M3_ERR_UNSUPPORTED;
        if (const char* why = panda_episodes_refusal(world, mode, PANDA_ROWS_THEN_WEIGHTS, code)) return peps_refuse(code, -1, std::string("the world: ") + why);
    }
    for (int i = 0; i < n; ++i) {
        m3_handle* h = planners[i];
        if (!h) return peps_refuse(M3_ERR_BAD_ARG, i, "null handle");
        if (h == world) return peps_refuse(M3_ERR_BAD_ARG, i, "the world handle is listed as a planner");
        for (int j = 0; j < i; ++j)
            if (planners[j] == h) return peps_refuse(M3_ERR_BAD_ARG, i, "handle listed twice");
        const m3_config& c = h->cfg;
        if (c.env_type != M3_ENV_PANDA) return peps_refuse(M3_ERR_UNSUPPORTED, i, "point_env planner (panda_env episodes only)");
        if (c.device != wc.device) return peps_refuse(M3_ERR_BAD_ARG, i, "handle on another device than the world");
        if (h->stream != world->stream) return peps_refuse(M3_ERR_STATE, i, "its stream differs from the world's");
        UpdateArgs u;
        int code;
        if (const char* why = batch_refusal(h, u, code, peps_sections(flags))) return peps_refuse(code, i, why);
        if (!h->action_out) return peps_refuse(M3_ERR_STATE, i, "no action-out destination (m3_set_action_out)");
    }
    // ---- allocations: all of the set's memory, here ----
    m3_panda_episodes* eps = new (std::nothrow) m3_panda_episodes();
    if (!eps) return peps_refuse(M3_ERR_HIP, -1, "out of host memory");
    m3_panda_episode_status st0;
    std::memset(&st0, 0, sizeof(st0));
    st0.phase = m3::PE_RUNNING; st0.done_tick = -1;
    try {
        eps->planners.assign(planners, planners + n);
        eps->plan.resize(n);
        eps->live.reserve(n);
        eps->mirror.assign(n, st0);
        if (mode == PANDA_EPISODES_RUNTIME)
            for (auto& kept : eps->rows_kept) kept.assign(n, PANDA_SCENE_DEFAULT);
    } catch (...) {
        delete eps;
        return peps_refuse(M3_ERR_HIP, -1, "out of host memory");
    }
    for (int i = 0; i < n; ++i) eps->plan[i] = planners[i]->action_out;
    eps->world = world;
    eps->n = n;
    eps->max_ticks = max_ticks;
    eps->settle_ticks = settle_ticks;
    eps->flags = flags;
    const SimViews& wv = world->views;
    const size_t st_b = align16((size_t)n * sizeof(m3_panda_episode_status));
    const size_t plan_b = align16((size_t)n * sizeof(const float*));
    const size_t kept_b = align16((size_t)n * 9 * sizeof(float));
    const size_t end_b = align16((size_t)n * sizeof(int));
    const size_t dof_b = align16((size_t)n * 18 * sizeof(float));
    const size_t root_b = align16((size_t)n * wv.n_actors * 13 * sizeof(float));
    const size_t rb_b = align16((size_t)n * wv.n_bodies * 13 * sizeof(float));
    eps->rb_bytes = (size_t)n * wv.n_bodies * 13 * sizeof(float);
    const hipStream_t s = world->stream;
    hipError_t e = own_device(eps->mem, eps->dev, st_b + plan_b + kept_b + end_b + dof_b + root_b + rb_b);
    if (e == hipSuccess && trace)
        e = own_device(eps->mem, eps->trace, (size_t)max_ticks * n * m3::PE_TRACE_FLOATS * sizeof(float));
    if (e == hipSuccess) e = own_pinned(eps->mem, eps->pinned, rb_b + end_b, hipHostMallocDefault);
    if (mode == PANDA_EPISODES_RUNTIME) {
        // the two tables, filled from the handles as they stand (a tick refreshes what changed since)
        const size_t table_bytes = (size_t)PANDA_SCENE_ROW_WORDS * n * sizeof(float);
        for (int side = 0; side < 2; ++side) {
            if (e == hipSuccess) e = own_device(eps->mem, eps->rows_dev[side], table_bytes);
            if (e == hipSuccess) e = own_pinned(eps->mem, eps->rows_pinned[side], table_bytes, hipHostMallocDefault);
            if (e == hipSuccess) e = peps_refresh_rows(eps, side);
        }
    }
    char* d_st = eps->dev;
    char* d_plan = d_st + st_b;
    char* d_kept = d_plan + plan_b;
    char* d_end = d_kept + kept_b;
    char* d_dof = d_end + end_b;
    char* d_root = d_dof + dof_b;
    char* d_rb = d_root + root_b;
    if (e == hipSuccess) e = hipMemcpyAsync(d_st, eps->mirror.data(), (size_t)n * sizeof(m3_panda_episode_status), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_plan, eps->plan.data(), (size_t)n * sizeof(const float*), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_kept, 0, kept_b + end_b, s);   // (a simulator's targets are zero until its first step_with_target)
    // the planning view starts as a copy of the world's views: the rows panda_push_views never writes (table, stands) are
    // the scene's, as in a planner's own simulator
    if (e == hipSuccess) e = hipMemcpyAsync(d_dof, wv.dof_state, (size_t)n * 18 * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_root, wv.root_state, (size_t)n * wv.n_actors * 13 * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rb, wv.rigid_body_state, eps->rb_bytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        m3_panda_episodes_destroy(eps);
        return peps_refuse(M3_ERR_HIP, -1, hipGetErrorString(e));
    }
    eps->ended_pinned = reinterpret_cast<int*>(eps->pinned + rb_b);
    eps->ended_dev = reinterpret_cast<int*>(d_end);
    eps->kept_dev = reinterpret_cast<float*>(d_kept);
    m3::PandaEpisodeArgs& a = eps->args;
    a.v = wv;
    a.pv = wv;
    a.pv.dof_state = reinterpret_cast<float*>(d_dof);
    a.pv.root_state = reinterpret_cast<float*>(d_root);
    a.pv.rigid_body_state = reinterpret_cast<float*>(d_rb);
    a.pv.net_contact_force = nullptr;
    a.world = world->sim_world;
    a.n = n;
    a.last_tick = max_ticks - 1;
    a.settle_ticks = settle_ticks;
    a.plan = reinterpret_cast<const float* const*>(d_plan);
    a.kept = eps->kept_dev;
    a.ended = eps->ended_dev;
    a.st = reinterpret_cast<m3_panda_episode_status*>(d_st);
    a.trace = eps->trace;
    *out = eps;
    return M3_OK;
}

extern "C" int m3_panda_episodes_create(m3_handle* world, m3_handle* const* planners, int n, int max_ticks, int settle_ticks,
                                        int trace, m3_panda_episodes** out) {
    return peps_create(world, planners, n, max_ticks, settle_ticks, trace, 0, out);
}

extern "C" int m3_panda_episodes_create_ex(m3_handle* world, m3_handle* const* planners, int n, int max_ticks, int settle_ticks,
                                           int trace, int flags, m3_panda_episodes** out) {
    if (out) *out = nullptr;
    if (flags & ~M3_PANDA_EPISODES_RUNTIME) {
        g_peps_err = "m3_panda_episodes_create_ex: unknown flag bits";
        return M3_ERR_BAD_ARG;
    }
    return peps_create(world, planners, n, max_ticks, settle_ticks, trace, flags, out);
}

extern "C" int m3_panda_episodes_flags(const m3_panda_episodes* eps) { return eps ? eps->flags : M3_ERR_BAD_ARG; }

static int peps_active(const m3_panda_episodes* eps) {
    int r = 0;
    for (int i = 0; i < eps->n; ++i) r += eps->mirror[i].phase != m3::PE_FROZEN;
    return r;
}

static int peps_ready(m3_panda_episodes* eps, const char* who) {
    if (peps_active(eps) == 0) { eps->err = std::string(who) + ": every episode has ended and settled"; return M3_ERR_STATE; }
    // (a workspace or cost weights set after m3_panda_episodes_create, which refuses them, or a switch forced off under a
    // run-time set: nothing of this tick is launched)
    const PandaEpisodesMode mode = peps_mode(eps->flags);
    for (int i = -1; i < eps->n; ++i) {
        const m3_handle* h = i < 0 ? eps->world : eps->planners[i];
        const char* why = panda_refusal(h, i < 0 ? PANDA_SIDE_STEP : PANDA_SIDE_ROLLOUT);   // (the world's step reads no weight)
        int code = M3_ERR_STATE;
        if (!why) why = panda_episodes_refusal(h, mode, PANDA_WEIGHTS_THEN_ROWS, code);
        if (why) {
            eps->err = std::string(who) + (i < 0 ? ": the world: " : ": planner " + std::to_string(i) + ": ") + why;
            return code;
        }
    }
    for (int i = 0; i < eps->n; ++i) {
        if (eps->planners[i]->groups.n > 0) {   // (sample groups set after create, which refuses them)
            eps->err = std::string(who) + ": planner " + std::to_string(i) + ": " + SAMPLE_GROUPS_UNBATCHED;
            return M3_ERR_UNSUPPORTED;
        }
        if (eps->planners[i]->action_out != eps->plan[i]) {
            eps->err = std::string(who) + ": planner " + std::to_string(i) + "'s action-out destination changed since create";
            return M3_ERR_STATE;
        }
    }
    return M3_OK;
}

extern "C" int m3_panda_episodes_observe(m3_panda_episodes* eps, const float** rb_host) {
    if (!eps) return M3_ERR_BAD_ARG;
    if (!rb_host) { eps->err = "m3_panda_episodes_observe: null argument"; return M3_ERR_BAD_ARG; }
    if (eps->observed) { eps->err = "m3_panda_episodes_observe: the tick was observed already"; return M3_ERR_STATE; }
    int rc = peps_ready(eps, "m3_panda_episodes_observe");
    if (rc != M3_OK) return rc;
    const hipStream_t s = eps->world->stream;
    // (a planner's m3_set_panda_scene / _rollout_scenes since the last tick applies from this one)
    if (peps_mode(eps->flags) == PANDA_EPISODES_RUNTIME) HIPCHK(eps, peps_refresh_rows(eps, 0));
    m3::launch_panda_episodes_pre(peps_launch_scene(eps), eps->args, s);
    HIPCHK(eps, hipGetLastError());
    HIPCHK(eps, hipMemcpyAsync(eps->pinned, eps->args.pv.rigid_body_state, eps->rb_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(eps, hipStreamSynchronize(s));
    eps->observed = true;
    *rb_host = reinterpret_cast<const float*>(eps->pinned);
    return M3_OK;
}

// the post kernel of the current tick under the host's word, and the host mirror's same step.  The pinned `ended` words are
// free to rewrite: the observe of this tick synchronised after the last tick's copy (tick 0: nothing was in flight)
static int peps_post(m3_panda_episodes* eps, const int* ended_host) {
    const hipStream_t s = eps->world->stream;
    for (int i = 0; i < eps->n; ++i) eps->ended_pinned[i] = ended_host[i] != 0;
    HIPCHK(eps, hipMemcpyAsync(eps->ended_dev, eps->ended_pinned, (size_t)eps->n * sizeof(int), hipMemcpyHostToDevice, s));
    // (the world's m3_set_panda_scene / _scene_rows since the last tick applies from this one; the mirror: peps_refresh_rows)
    if (peps_mode(eps->flags) == PANDA_EPISODES_RUNTIME) HIPCHK(eps, peps_refresh_rows(eps, 1));
    m3::launch_panda_episodes_post(peps_launch_scene(eps), eps->args, eps->tick, s);
    HIPCHK(eps, hipGetLastError());
    for (int i = 0; i < eps->n; ++i)
        (void)m3::pe_advance(eps->mirror[i], eps->ended_pinned[i], eps->tick, eps->args.last_tick, eps->settle_ticks);
    eps->tick += 1;
    eps->observed = false;
    return M3_OK;
}

extern "C" int m3_panda_episodes_act(m3_panda_episodes* eps, m3_batch* batch, const int* ended_host) {
    if (!eps) return M3_ERR_BAD_ARG;
    if (!batch || !ended_host) { eps->err = "m3_panda_episodes_act: null argument"; return M3_ERR_BAD_ARG; }
    if (eps->tick == 0) { eps->err = "m3_panda_episodes_act: tick 0 is m3_panda_episodes_act_first's"; return M3_ERR_STATE; }
    if (!eps->observed) { eps->err = "m3_panda_episodes_act: the tick was not observed (m3_panda_episodes_observe)"; return M3_ERR_STATE; }
    int rc = peps_ready(eps, "m3_panda_episodes_act");
    if (rc != M3_OK) return rc;
    eps->live.clear();
    const SimViews& pv = eps->args.pv;
    for (int i = 0; i < eps->n; ++i) {
        if (eps->mirror[i].phase != m3::PE_RUNNING || ended_host[i]) continue;
        m3_handle* h = eps->planners[i];
        // planner i plans from row i of the planning view: the rollout takes row 0 of its bound views, so it sees the floats
        // row 0 of its own simulator would hold after update_plan's step
        rc = m3_bind_sim_panda(h, pv.dof_state + (size_t)i * 18, pv.root_state + (size_t)i * pv.n_actors * 13, pv.n_actors,
                               pv.box_actor, pv.dyn_actor, pv.obs_actor);
        if (rc != M3_OK) { eps->err = "m3_panda_episodes_act: " + h->err; return rc; }
        eps->live.push_back(h);
    }
    if (!eps->live.empty()) {
        // (a run-time set passes the batch's own flag through, as m3_batch_command does: a batch without the section refuses a
        // planner that needs it, with its code and message, before anything is launched)
        rc = batch_command(batch, eps->live.data(), (int)eps->live.size(), nullptr, batch->flags & peps_sections(eps->flags));
        if (rc != M3_OK) { eps->err = std::string("m3_panda_episodes_act: ") + m3_batch_last_error(batch); return rc; }
    }
    return peps_post(eps, ended_host);
}

extern "C" int m3_panda_episodes_act_first(m3_panda_episodes* eps, m3_handle* const* sims, const int* ended_host) {
    if (!eps) return M3_ERR_BAD_ARG;
    if (!sims || !ended_host) { eps->err = "m3_panda_episodes_act_first: null argument"; return M3_ERR_BAD_ARG; }
    if (eps->tick != 0) { eps->err = "m3_panda_episodes_act_first: tick 0 is done"; return M3_ERR_STATE; }
    int rc = peps_ready(eps, "m3_panda_episodes_act_first");
    if (rc != M3_OK) return rc;
    const m3_handle* w = eps->world;
    for (int i = 0; i < eps->n; ++i) {
        if (ended_host[i]) continue;
        const m3_handle* sh = sims[i];
        const char* why = nullptr;
        if (!sh) why = "null handle";
        else if (sh->cfg.env_type != M3_ENV_PANDA || !sh->cfg.sim_only || !sh->sim_u) why = "not a sim_only panda_env handle with bound views";
        else if (sh->cfg.device != w->cfg.device || sh->stream != w->stream) why = "its device or stream differs from the world's";
        else if (sh->cfg.dt != w->cfg.dt || sh->cfg.substeps != w->cfg.substeps) why = "its dt / substeps differ from the world's";
        if (why) { eps->err = "m3_panda_episodes_act_first: simulator " + std::to_string(i) + ": " + why; return M3_ERR_STATE; }
    }
    // the targets planner i's simulator keeps from here on (row 0: the only row ever read again)
    for (int i = 0; i < eps->n; ++i) {
        if (ended_host[i]) continue;
        HIPCHK(eps, hipMemcpyAsync(eps->kept_dev + (size_t)i * 9, sims[i]->sim_u, 9 * sizeof(float), hipMemcpyDeviceToDevice, w->stream));
    }
    return peps_post(eps, ended_host);
}

extern "C" int m3_panda_episodes_ticks_done(const m3_panda_episodes* eps) { return eps ? eps->tick : M3_ERR_BAD_ARG; }

extern "C" int m3_panda_episodes_running(const m3_panda_episodes* eps) {
    if (!eps) return M3_ERR_BAD_ARG;
    int r = 0;
    for (int i = 0; i < eps->n; ++i) r += eps->mirror[i].phase == m3::PE_RUNNING;
    return r;
}

extern "C" int m3_panda_episodes_active(const m3_panda_episodes* eps) { return eps ? peps_active(eps) : M3_ERR_BAD_ARG; }

extern "C" int m3_panda_episodes_status(m3_panda_episodes* eps, m3_panda_episode_status* status_out, float* trace_out) {
    if (!eps || !status_out) return M3_ERR_BAD_ARG;
    if (eps->observed) { eps->err = "m3_panda_episodes_status: between observe and act (the host copy is in use)"; return M3_ERR_STATE; }
    const hipStream_t s = eps->world->stream;
    const SimViews& v = eps->args.v;
    HIPCHK(eps, hipMemcpyAsync(status_out, eps->args.st, (size_t)eps->n * sizeof(m3_panda_episode_status), hipMemcpyDeviceToHost, s));
    // an ended and settled episode's row of the world is not stepped any more: its rigid-body rows hold the cubes as the
    // episode's last step left them (through the set's pinned buffer: nothing is allocated here either)
    HIPCHK(eps, hipMemcpyAsync(eps->pinned, v.rigid_body_state, eps->rb_bytes, hipMemcpyDeviceToHost, s));
    if (trace_out) {
        if (!eps->trace) { eps->err = "m3_panda_episodes_status: the set was created without a trace"; return M3_ERR_STATE; }
        HIPCHK(eps, hipMemcpyAsync(trace_out, eps->trace, (size_t)eps->max_ticks * eps->n * m3::PE_TRACE_FLOATS * sizeof(float),
                                 hipMemcpyDeviceToHost, s));
    }
    HIPCHK(eps, hipStreamSynchronize(s));
    const float* rb = reinterpret_cast<const float*>(eps->pinned);
    for (int i = 0; i < eps->n; ++i) {
        const float* row = rb + (size_t)i * v.n_bodies * 13;
        for (int j = 0; j < 3; ++j) {
            status_out[i].cubeA[j] = row[v.box_body * 13 + j];
            status_out[i].cubeB[j] = row[v.dyn_body * 13 + j];
        }
    }
    return M3_OK;
}
