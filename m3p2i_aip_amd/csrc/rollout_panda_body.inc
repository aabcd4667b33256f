// rollout_panda_body.inc -- the body of k_rollout_panda (rollout_panda.hip), included by the kernel and by its batched form
// kb_rollout_panda: the same tokens in both, so that k_rollout_panda compiles to exactly the code it did as a plain kernel
// (as update_small_body.inc).  In scope where it is included: FORCES, GENERAL, LPS, the scene type `SceneT` (PandaScene, or
// PandaSceneRT in rollout_panda_scene.hip), `const RolloutArgs& a_`, `const PandaArgs& pa`, `const SceneT& sc_`, a selection of
// each of the two hooks (rollout_panda_common.hpp), optionally of the third (prior samples), and whatever the selections name:
// `WT_OFFSET`, `scene_rows` or `tab`, `prior_slot` and `prior_tab`.
#if !defined(PANDA_BODY_COST) || !defined(PANDA_BODY_SCENE)
#error "rollout_panda_body.inc: define PANDA_BODY_COST and PANDA_BODY_SCENE as selections of rollout_panda_common.hpp in front of this #include"
#endif
#ifndef PANDA_BODY_PRIORS     // (the third hook is optional: no prior samples)
#define PANDA_BODY_PRIORS PANDA_PRIORS_NONE
#endif
    PANDA_CORNER_LDS(LPS);
    // (a_.lanes samples per 64-wide wavefront: m3_set_rollout_lanes; the idle lanes leave at once)
    // Shadow lanes (quirk Q8, pa.shadows = 1 or 2; reach on an unsharded handle): the reference's reach cost measures every
    // rollout against the cube of ENVIRONMENT 0 (and, for the tilted mode, the orientation of the first environment of the
    // second half), which under world spec v2 is a quantity of THAT rollout's simulation.  The last sample slot of every
    // wavefront (lane 63; with LPS = 16 the last group of sixteen) re-simulates sample 0 and the one before it sample K / 2 in
    // lockstep with the wavefront's own samples (same noise rows, same operations, so the same bits in every wavefront);
    // their cubes are read with v_readlane after each step.  They store nothing.  Cost: 64 / 63 (62) more wavefronts
    // (LPS = 16: 4 / 3, 4 / 2), no cross-wavefront synchronisation.
    constexpr int SPW = 64 / LPS;                       // sample slots per wavefront
    const bool deferred = LPS != 1 && pa.reach_rec != nullptr;   // (the one-lane form keeps its shadow slots: launch_rollout_panda)
    const int slot = (int)threadIdx.x / LPS, gl = (int)threadIdx.x % LPS;
    const bool shadow = slot >= SPW - pa.shadows;
    const bool writer = !shadow && gl == 0;             // the lane that stores the sample's scalars
    int i = blockIdx.x * a_.lanes + slot;
    if (shadow) i = (slot == SPW - 1) ? 0 : pa.cp.half_K;
    else if (slot >= a_.lanes || i >= a_.Kl) return;
    // The per-joint constants (bounds, noise scale, servo coefficients: 54 floats) are uniform, but
    // there are not enough scalar registers to keep them across the step loop, and the compiler
    // re-read them from the kernel arguments every step (~12 scalar loads per step, each followed by
    // a wait with nothing else resident on the SIMD to cover it).  Vector registers are plentiful at
    // one wave per SIMD, so they are parked there once.
    RolloutArgs a = a_;
    SceneT sc = sc_;
    if constexpr (!GENERAL) { a.sampling_random = 0; a.mode_simple = 0; a.full_sigma = 0; a.noise_abs_cost = 0; }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        a.u_min[j] = in_vgpr(a_.u_min[j]); a.u_max[j] = in_vgpr(a_.u_max[j]);
        // (update_cov rewrites the scale on the device after every command: mppi.py:516)
        a.scale_tril[j] = in_vgpr(a_.scale_dev ? a_.scale_dev[j] : a_.scale_tril[j]);
        sc.a[j] = in_vgpr(sc_.a[j]); sc.rden[j] = in_vgpr(sc_.rden[j]); sc.dv[j] = in_vgpr(sc_.dv[j]);
    }
    const int Kl = a.Kl, T = a.T;
    const int k = a.k0 + i;
    PANDA_BODY_SCENE(sc, i)      // (the scene hook: rollout_panda_common.hpp)
    PANDA_BODY_PRIORS(SLOT, i)   // (the priors hook, here and at three more places)
    PandaWorld w;
    if (a.sim_dof) panda_world_from_sim(a.sim_dof, a.sim_root, pa.cubeA_actor, pa.cubeB_actor, pa.obs_actor, w);
    else panda_world_from_raw(pa.world0, w);
    float hp[3], trav = 0.0f;   // hand origin at the last evaluated kinematics, joint travel since (panda_step)
    panda_infer_held(sc, w, hp);

    const bool is_last = (k == a.Kg - 1);
    const bool first_half = k < pa.cp.half_K;
    const bool halton = !a.mode_simple;
    const float* mptr = a.mean;
    if (a.multi_modal && halton) mptr = first_half ? a.mean1 : a.mean2;

    // inputs of step t+1 are fetched before step t is simulated (one wavefront per SIMD: nothing
    // else hides the latency of a load that is consumed at once)
    const bool use_best = halton && a.multi_modal && (k == 0 || k == pa.cp.half_K);
    const float* bptr = (k == 0) ? a.best1 : a.best2;
    float nd[9], nm[9];
    auto fetch = [&](int t) {
        // _shift_action: mppi.py:266-273; simple mode: torch.roll(U, -1), mppi.py:221
        const int ts = a.mode_simple ? ((t + 1 == T) ? 0 : t + 1) : ((t + 1 < T) ? t + 1 : T - 1);
        const float* dptr = a.delta + ((size_t)t * Kl + i) * 9;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            nd[j] = a.sampling_random ? 0.0f : dptr[j];
            nm[j] = use_best ? bptr[ts * 9 + j] : mptr[ts * 9 + j];
        }
        PANDA_BODY_PRIORS(FETCH, t)
    };
    fetch(0);
    FkCarry<LPS> fkc;
    fkc.valid = false;
    fkc.near_lane_substeps = 0;
    float J = 0.0f, g = 1.0f, S = 0.0f, pc = 0.0f;
#ifdef M3_PABL_PROF
    PandaProf prof = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    long long prof_step = 0;
    const long long prof_start = __builtin_readcyclecounter();
#endif
    for (int t = 0; t < T; ++t) {
        float cd[9], cm[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) { cd[j] = nd[j]; cm[j] = nm[j]; }
        PANDA_BODY_PRIORS(HOLD)
        if (t + 1 < T) fetch(t + 1);
        if constexpr (GENERAL) {
            if (a.sampling_random) {   // N(noise_mu, noise_sigma) = mu + L z (noise_stream.hpp; order as the oracle)
                float z[10];
#pragma unroll
                for (int p = 0; p < 5; ++p) gauss_pair(a.seed, a.call, (unsigned)k, (unsigned)t, (unsigned)p, z[2 * p], z[2 * p + 1]);
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    float acc;
                    if (a.full_sigma) {
                        acc = a.noise_mats[j * 9 + 0] * z[0];
#pragma unroll
                        for (int q = 1; q <= j; ++q) acc = acc + a.noise_mats[j * 9 + q] * z[q];
                    } else acc = z[j] * a_.scale_tril[j];   // (the configured scale, not update_cov's)
                    cd[j] = a.noise_mu[j] + acc;
                }
            }
        }
        float u[9], e[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            float aj;
            if (GENERAL && a.mode_simple) {
                aj = fmaxf(fminf(cm[j] + cd[j], a.u_max[j]), a.u_min[j]);             // mppi.py:341-345
            } else {
                const float d = is_last ? 0.0f : cd[j];                                // mppi.py:392
                aj = fmaxf(fminf(cm[j] + d * a.scale_tril[j], a.u_max[j]), a.u_min[j]);
                if (use_best) aj = cm[j];                                              // :407-409
            }
            PANDA_BODY_PRIORS(SELECT, aj, j)
            if (j >= 7) {                                                              // :412-416 / :346-350
                if (a.gripper_cmd == 1) aj = 1.5f;
                else if (a.gripper_cmd == 2) aj = -1.5f;
            }
            float uj = a.u_scale * aj;                                                 // :297
            if (a.sample_null_action && is_last) uj = 0.0f;                            // :300-302
            u[j] = uj;
            e[j] = uj;                                     // :313 (the update consumes the scaled stack)
        }
        PandaObs obs;
#ifdef M3_PABL_PROF
        const long long prof_s0 = __builtin_readcyclecounter();
        panda_step<FORCES, true, LPS>(sc, w, u, obs, cs, hp, &trav, &fkc, &prof);
        prof_step += __builtin_readcyclecounter() - prof_s0;
#else
        panda_step<FORCES, true, LPS>(sc, w, u, obs, cs, hp, &trav, &fkc);
#endif
        float cube0[3], qh0[4];
        if (deferred) {
            // the reach cost of this step is formed by k_panda_reach_cost (below) from what it reads of the sample -- and of
            // samples 0 and K / 2, whose cube it is measured against (quirk Q8): no shadow slots in this launch
            if (writer) {
                float* r = pa.reach_rec + (size_t)t * REACH_REC * Kl + i;
#pragma unroll
                for (int j = 0; j < 3; ++j) { r[(0 + j) * Kl] = obs.left[j]; r[(3 + j) * Kl] = obs.right[j]; r[(14 + j) * Kl] = w.A.p[j]; }
#pragma unroll
                for (int j = 0; j < 4; ++j) { r[(6 + j) * Kl] = obs.left_q[j]; r[(10 + j) * Kl] = w.A.q[j]; }
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) cube0[j] = w.A.p[j];
#pragma unroll
            for (int j = 0; j < 4; ++j) qh0[j] = w.A.q[j];
        } else if (pa.shadows) {
#pragma unroll
            for (int j = 0; j < 3; ++j) cube0[j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w.A.p[j]), 63));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float q0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w.A.q[j]), 63));
                const float q1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w.A.q[j]), 63 - LPS));
                qh0[j] = first_half ? q0 : q1;     // (one shadow: single mode, the tilt term does not read it)
            }
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) cube0[j] = w.A.p[j];
#pragma unroll
            for (int j = 0; j < 4; ++j) qh0[j] = w.A.q[j];
        }
        const float c = deferred ? 0.0f : PANDA_BODY_COST(w, obs, k, cube0, qh0);   // (the cost hook: rollout_panda_common.hpp)
        if (writer) {
            *reinterpret_cast<float4*>(a.states + ((size_t)t * Kl + i) * 4) =
                make_float4(w.q[0], w.qd[0], w.q[1], w.qd[1]);                   // reactive_tamp.py:66-69
            if (!deferred) a.cost_h[(size_t)t * Kl + i] = c;
        }
        if constexpr (LPS == 1) {
            if (!shadow) {
                float* ap = a.actions + ((size_t)t * Kl + i) * 9;
#pragma unroll
                for (int j = 0; j < 9; ++j) ap[j] = e[j];
            }
        } else {          // the sample's lanes store one control each
            const Gen<LPS> eo = gen_from9<LPS>(e);
#pragma unroll
            for (int el = 0; el < Gen<LPS>::N; ++el) {
                const int cj = gen_coord<LPS>(el);
                if (!shadow && cj < 9) a.actions[((size_t)t * Kl + i) * 9 + cj] = eo.a[el];
            }
        }
        J = J + g * c;
        g = g * a.gamma;
        if constexpr (GENERAL) {
            if (a.mode_simple) {   // mppi.py:309 and the perturbation cost :355-372: sum U * ((lambda * noise) @ Sigma^-1)
                S = S + c;
                float ln[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    float n = e[j] - cm[j];
                    if (a.noise_abs_cost) n = fabsf(n);
                    ln[j] = a.lambda_ * n;
                }
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    float ac;
                    if (a.full_sigma) {
                        ac = ln[0] * a.noise_mats[81 + 0 * 9 + j];
#pragma unroll
                        for (int q = 1; q < 9; ++q) ac = ac + ln[q] * a.noise_mats[81 + q * 9 + j];
                    } else ac = ln[j] * a.sigma_inv[j];
                    pc = pc + cm[j] * ac;
                }
            }
        }
    }
#ifdef M3_PABL_PROF     // (cost_horizon rows 0-5 of the sample: total / solver / near-path clocks, substeps with gripper rows / body rows / near)
    if (writer && T >= 6) {
        a.cost_h[(size_t)0 * Kl + i] = (float)(__builtin_readcyclecounter() - prof_start);
        a.cost_h[(size_t)1 * Kl + i] = (float)prof.solve_clk;
        a.cost_h[(size_t)2 * Kl + i] = (float)prof.near_clk;
        a.cost_h[(size_t)3 * Kl + i] = (float)prof.n_robot;
        a.cost_h[(size_t)4 * Kl + i] = (float)prof.n_body;
        a.cost_h[(size_t)5 * Kl + i] = (float)prof.n_near;
        if (T >= 10) {
            a.cost_h[(size_t)6 * Kl + i] = (float)prof.detect_clk;
            a.cost_h[(size_t)7 * Kl + i] = (float)prof.post_clk;
            a.cost_h[(size_t)8 * Kl + i] = (float)prof.n_act;
            a.cost_h[(size_t)9 * Kl + i] = (float)prof.n_fk;
        }
        if (T >= 14) {
            a.cost_h[(size_t)10 * Kl + i] = (float)prof.pre_clk;
            a.cost_h[(size_t)11 * Kl + i] = (float)prof.mid_clk;
            a.cost_h[(size_t)12 * Kl + i] = (float)prof.wake_clk;
            a.cost_h[(size_t)13 * Kl + i] = (float)prof_step;
        }
    }
#endif
    if (!deferred) {      // (else: k_panda_reach_cost writes the costs and leaves the minima behind)
        if (writer) a.J[i] = (GENERAL && a.mode_simple) ? (S + pc) : J;
        if (a.wave_min) wave_min_store(a.wave_min, J, first_half, writer);
    }
    // What the NEXT reach commands' kernel form is chosen by (panda_lps_for): the share of (sample, substep) pairs of this launch
    // in which the gripper was within reach of a box or a cube was awake, in 1/1000.  Every wavefront adds its count; the last one to finish (the
    // same atomic is its ticket) turns the sum into the share, stores it into a word of mapped host memory and clears the counters for the next
    // launch.  A hint: results do not depend on the form.
    if (pa.busy_hint != nullptr && threadIdx.x == 0) {
        // ONE atomic carries both: bits 0-23 wavefronts finished, bits 24-63 the sum of their counts
        const unsigned long long mine = ((unsigned long long)(unsigned)(fkc.near_lane_substeps / LPS) << 24) | 1ull;
        const unsigned long long old = atomicAdd(pa.busy_count, mine);
        if ((old & 0xffffffull) == (unsigned long long)(gridDim.x - 1u)) {
            const unsigned long long total = (old + mine) >> 24;
            *pa.busy_count = 0ull;
            const unsigned long long all = (unsigned long long)Kl * (unsigned long long)(T * sc.substeps);
            *(volatile int*)pa.busy_hint = (int)((total * 1000ull) / (all ? all : 1ull)) + 1;    // (+ 1: 0 = nothing reported yet)
        }
    }
#undef PANDA_BODY_COST
#undef PANDA_BODY_SCENE
#undef PANDA_BODY_PRIORS
