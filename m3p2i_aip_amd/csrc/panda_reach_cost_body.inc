// panda_reach_cost_body.inc -- the body of k_panda_reach_cost (rollout_panda.hip), included by the kernel and by its
// batched form kb_panda_reach_cost (as rollout_panda_body.inc).  In scope where it is included: `const RolloutArgs& a` and
// `const PandaArgs& pa`, a selection of the cost hook (rollout_panda_common.hpp) and whatever it names: `WT_OFFSET` or `tab`.
#ifndef PANDA_BODY_COST
#error "panda_reach_cost_body.inc: define PANDA_BODY_COST as a selection of rollout_panda_common.hpp in front of this #include"
#endif
    __shared__ float s_c[RC_CH][64];
    const int Kl = a.Kl, T = a.T;
    const int lane = (int)threadIdx.x & 63, slice = (int)threadIdx.x >> 6;
    const int i0 = blockIdx.x * 64 + lane;
    const bool mine = i0 < Kl;
    const int i = mine ? i0 : 0;          // (every lane stays for the barriers)
    const int k = a.k0 + i;
    const bool first_half = k < pa.cp.half_K;
    const int h = (pa.cp.multi_modal && !first_half) ? pa.cp.half_K : 0;    // whose cube orientation the tilt term reads
    float J = 0.0f, g = 1.0f;
    for (int t0 = 0; t0 < T; t0 += RC_CH) {
        for (int tt = slice; tt < RC_CH && t0 + tt < T; tt += RC_TS) {
            const int t = t0 + tt;
            const float* r = pa.reach_rec + (size_t)t * REACH_REC * Kl;
            PandaObs o;
            PandaWorld w;
            float cube0[3], qh0[4];
#pragma unroll
            for (int j = 0; j < 3; ++j) { o.left[j] = r[(0 + j) * Kl + i]; o.right[j] = r[(3 + j) * Kl + i]; cube0[j] = r[(14 + j) * Kl]; }
#pragma unroll
            for (int j = 0; j < 4; ++j) { o.left_q[j] = r[(6 + j) * Kl + i]; w.A.q[j] = r[(10 + j) * Kl + i]; qh0[j] = r[(10 + j) * Kl + h]; }
            const float c = PANDA_BODY_COST(w, o, k, cube0, qh0);
            if (mine) a.cost_h[(size_t)t * Kl + i] = c;
            s_c[tt][lane] = c;
        }
        __syncthreads();
        if (slice == 0) {
            for (int tt = 0; tt < RC_CH && t0 + tt < T; ++tt) {
                J = J + g * s_c[tt][lane];
                g = g * a.gamma;
            }
        }
        __syncthreads();
    }
    if (slice == 0 && mine) a.J[i] = J;
    if (a.wave_min) wave_min_store(a.wave_min, J, first_half, mine && slice == 0);
#undef PANDA_BODY_COST
