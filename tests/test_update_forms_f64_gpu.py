"""Every form of the update (the importance weights and everything formed from them) against the float64 restatement
of the reference (tests/update_ref.py), on synthetic costs, actions, states and means written into the buffers.

Which kernels run depends on K, nu, the mode, the entry point and m3_set_update_launches:

  form                                                    reached by
  k_update_small<2,false,8/16/32/64>                      nu=2 single, fused, K <= 16384 (rows: K = 2048/4096/8192)
  k_update_small<2,true,...> (256 and 512 threads)        nu=2 multi-modal, fused, K <= 8192 (512 above 2048)
  k_update_small<9,...>                                   Panda (nu=9), fused, K <= 4096
  k_weights<32,256> + k_wsum + k_finalize                 unfused, K <= 8192, and Panda 4097..8192
  k_weights<24,1024>: register, LDS, global-memory tiers  K > 8192 where the paths below do not apply: Panda
                                                          8193..16384; multi-modal unfused with
                                                          apply_workgroups(K) > 256 (K > 2^20: all three tiers)
  k_sumexp_single + k_apply_weights<false>                single / simple mode, K > 16384
  k_mins + k_ladder + k_search + k_apply_weights<true>    multi-modal unfused, K > 8192 (also fused with
                                                          set_update_launches(5), and fused K > 131072)
  k_ladder_search + k_regen_part + k_regen_done           multi-modal fused, 4096 < K <= 131072
  k_cov_partial + k_cov_apply                             update_cov, after every finalize
  top-k stage A / B and their argmin-round fallbacks      > TK_CAP = 1024 candidates in a 4096-cost workgroup;
                                                          stage B with more than 1024 candidates of the lists

"fused" is m3_update_finalize (what m3_command runs after its rollout; with T * nu > 2048 it is m3_update +
m3_finalize), "phases" m3_update then m3_finalize, "five" m3_update_finalize after m3_set_update_launches(5).

Tolerances, from a float32 error bound.  u = 2^-24.  A kernel weight is (1/eta) * exp2(log2(e) * (-1/beta) * (J - m)):
J - m, -1/beta and the product each round once (relative u each), so the exponent x = (J - m)/beta carries an absolute
error <= 3u|x| and exp adds ~2 ulp; eta is a sum of at most 2^21 positive terms in blocked order (a few u * log2(K)
on the sums that occur, bounded here by 1e-5), and 1/eta and the product round once more.  Hence
    |w - w_ref| <= (2e-5 + 4u|x|) w_ref          for w_ref >= 1e-30 (|x| <= ~85 there),
    |w - w_ref| <= 1e-30                          below (exp flushes to zero).
The reference's beta is a Python float; the kernels carry the chain of x0.9 / x1.2 steps as binary32 products, which
after n passes differ by <= n u relative -- at |x| = 70 that alone would move a weight by far more than the bar.  So
the float64 formulas are evaluated at the binary32 chain (`beta32` of update_ref) and the kernels' beta must equal it
bit for bit; the float64 chain is held to n u of it.  Sums of weighted actions (means) carry the weights' relative
error on the samples that matter (small |x|) plus the blocked sum's rounding: <= 1e-5 of the actions' scale; the
covariance the same of its own scale; the filtered plan that times the filter's largest absolute row sum.
eta of a search pass lands on the other side of a bound of its window than in float64 only when it grazes the bound:
then the reference's eta at the deciding pass must lie within 1e-5 relative of 3 or 10 (20 or 10 for the Panda beta
step), and the comparison continues against the reference with that one decision reversed.  Nothing is skipped."""
import numpy as np
import pytest

from tests import update_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U32 = 2.0 ** -24


def _sg_gain():
    import scipy.signal
    return max(np.abs(np.array([scipy.signal.savgol_coeffs(9, 2, pos=p, use="dot") for p in range(9)])).sum(1))


# (id, K, T, nu, mode, dist, entry, calls, update_cov): the form each is meant to reach is in the id
CASES = [
    # ---- nu = 2, single mode ----
    ("small2_r8_K20_T9", 20, 9, 2, "single", "s1", "fused", 1, False),
    ("small2_r8_K24_inf_in_top20", 24, 30, 2, "single", "inf24", "fused", 1, False),
    ("weights32_K21", 21, 30, 2, "single", "s1", "phases", 1, False),
    ("small2_r8_K63_negative", 63, 30, 2, "single", "neg", "fused", 1, False),
    ("weights32_K64_signed_zeros", 64, 30, 2, "single", "zeros", "phases", 1, False),
    ("small2_r8_K65_signed_zeros", 65, 30, 2, "single", "zeros", "fused", 1, False),
    ("small2_r8_K255_argmax_tie", 255, 30, 2, "single", "tie", "fused", 1, False),
    ("weights32_K257_spread1e-5", 257, 30, 2, "single", "s1e-5", "phases", 1, False),
    ("small2_r8_K2047_spread1e8", 2047, 30, 2, "single", "s1e8", "fused", 1, False),
    ("small2_r8_K2048_offset", 2048, 30, 2, "single", "offset", "fused", 1, False),
    ("small2_r16_K2049", 2049, 30, 2, "single", "s1", "fused", 1, False),
    ("weights32_K4095_stageA_rounds", 4095, 30, 2, "single", "stageA", "phases", 1, False),
    ("small2_r16_K4096_stageA_rounds", 4096, 30, 2, "single", "stageA", "fused", 1, False),
    ("small2_r32_K4097_dup_min", 4097, 30, 2, "single", "dupmin", "fused", 1, False),
    ("small2_r32_K8191", 8191, 30, 2, "single", "s1", "fused", 1, False),
    ("weights32_K8192_signed_zeros", 8192, 30, 2, "single", "zeros", "phases", 1, False),
    ("small2_r64_K8193_dup_min", 8193, 30, 2, "single", "dupmin", "fused", 1, False),
    ("weights24_reg_K16383", 16383, 30, 2, "single", "s1", "phases", 1, False),
    ("small2_r64_K16384_inf", 16384, 30, 2, "single", "inf", "fused", 1, False),
    ("sumexp_K16385", 16385, 30, 2, "single", "s1", "fused", 1, False),
    ("sumexp_K57345_argmax_tie", 57345, 30, 2, "single", "tie", "phases", 1, False),
    ("sumexp_K131073_offset", 131073, 30, 2, "single", "offset", "fused", 1, False),
    ("sumexp_K262144_stageB_rounds", 262144, 30, 2, "single", "stageB", "fused", 1, False),
    ("unfused_finalize_K2049_T1030", 2049, 1030, 2, "single", "s1", "fused", 1, False),
    ("small2_r16_K2049_cov", 2049, 30, 2, "single", "s1", "fused", 3, True),
    # ---- nu = 2, multi-modal (odd K: the halves differ) ----
    ("small2_mm256_K21", 21, 30, 2, "multi", "s1", "fused", 1, False),
    ("weights32_mm_K63_signed_zeros", 63, 30, 2, "multi", "zeros", "phases", 1, False),
    # (1e6 + U(0, 1) holds 16 distinct float32 values: beyond ~10 samples per half tied at the minimum the search has no
    # end, in the reference too -- so the offset case of the multi-modal searches is a small K)
    ("weights32_mm_K65_offset", 65, 30, 2, "multi", "offset", "phases", 1, False),
    ("small2_mm256_K255_argmax_tie", 255, 9, 2, "multi", "tie", "fused", 1, False),
    ("small2_mm256_K2047_spread1e-5", 2047, 30, 2, "multi", "s1e-5", "fused", 1, False),
    ("small2_mm512_K2049_spread1e8", 2049, 30, 2, "multi", "s1e8", "fused", 1, False),
    ("weights32_mm_K4095", 4095, 30, 2, "multi", "s1", "phases", 1, False),
    ("small2_mm512_K4097_negative", 4097, 30, 2, "multi", "neg", "fused", 1, False),
    ("small2_mm512_K8191_dup_min", 8191, 30, 2, "multi", "dupmin", "fused", 1, False),
    ("ladder_search_K8193", 8193, 30, 2, "multi", "s1", "fused", 1, False),
    ("five_launch_K8193", 8193, 30, 2, "multi", "s1", "five", 1, False),
    ("split_K16383_spread1e-5", 16383, 30, 2, "multi", "s1e-5", "phases", 1, False),
    ("ladder_search_K16385_negative", 16385, 30, 2, "multi", "neg", "fused", 1, False),
    ("five_launch_K57345_inf", 57345, 30, 2, "multi", "inf", "five", 1, False),
    ("ladder_search_K131071_spread1e8", 131071, 30, 2, "multi", "s1e8", "fused", 1, False),
    ("split_fused_K131073", 131073, 30, 2, "multi", "s1", "fused", 1, False),
    ("split_K262143", 262143, 30, 2, "multi", "s1", "phases", 1, False),
    ("weights24_all_tiers_K1052673_T9", 1052673, 9, 2, "multi", "s1", "phases", 1, False),
    # ---- nu = 2, simple mode (beta = lambda_, U rolled) ----
    ("small2_simple_K20_T9", 20, 9, 2, "simple", "s1", "fused", 3, False),
    ("weights32_simple_K2049", 2049, 30, 2, "simple", "s1", "phases", 3, False),
    ("small2_simple_K8193_zeros", 8193, 30, 2, "simple", "zeros", "fused", 1, False),
    ("sumexp_simple_K16385", 16385, 30, 2, "simple", "s1", "fused", 3, False),
    ("sumexp_simple_K262144_spread1e-5", 262144, 30, 2, "simple", "s1e-5", "phases", 1, False),
    # ---- nu = 9 (Panda), single mode: beta adapted after every call and persisted ----
    ("small9_K21", 21, 20, 9, "single", "cycle", "fused", 3, False),
    ("small9_K4096_cov", 4096, 20, 9, "single", "cycle", "fused", 3, True),
    ("weights32_panda_K4097", 4097, 20, 9, "single", "cycle", "fused", 3, False),
    ("weights24_reg_panda_K8193_cov", 8193, 20, 9, "single", "cycle", "phases", 3, True),
    ("weights24_reg_panda_K16384", 16384, 20, 9, "single", "cycle", "fused", 3, False),
    ("sumexp_panda_K16385_cov", 16385, 20, 9, "single", "cycle", "fused", 3, True),
    ("unfused_finalize_panda_K2049_T228_cov", 2049, 228, 9, "single", "cycle", "fused", 3, True),
]


def stage_a_layout(K):
    """Costs that overflow top-k stage A's candidate list (TK_CAP = 1024) in every 4096-cost workgroup, all distinct:
    local index i = e * 256 + tid (tid = 64 * wave + lane, e < 16 register rows) holds lane * 1e-3 + e * 1e-5 +
    wave * 1e-6 (+ 0.1 per workgroup).  Each wave's threshold is its lanes' 20th smallest minimum, lane 19's
    row 0; every cost of lanes 0..18 lies below it: 19 * 16 * 4 > 1024 survivors."""
    i = np.arange(K)
    blk, loc = i // 4096, i % 4096
    e, tid = loc // 256, loc % 256
    return (0.1 * blk + (tid % 64) * 1e-3 + e * 1e-5 + (tid // 64) * 1e-6).astype(np.float32)


def stage_a_survivors(J):
    """What the kernel's stage A keeps of the first workgroup (update_common.hpp: topk_stage_a), counted on the host."""
    blk = np.full(4096, np.inf, np.float32)
    blk[:min(4096, len(J))] = J[:4096]
    rv = blk.reshape(16, 4, 64)                  # [row e][wave][lane]
    lane_min = rv.min(axis=0)                    # [wave][lane]
    tau = np.sort(lane_min, axis=1)[:, 19].min()
    return int((blk <= tau).sum())


def make_costs(dist, K, rng, call=0):
    a = np.abs(rng.standard_normal(K))
    if dist == "s1":
        return a.astype(np.float32)
    if dist in ("s1e-5", "s1e8"):
        return (float("1" + dist[2:]) * a).astype(np.float32)
    if dist == "cycle":   # Panda: eta > 20 and < 10 in turn, so the beta step goes both ways
        return ((1.0, 1e3, 0.03)[call % 3] * a).astype(np.float32)
    if dist == "offset":
        return (1e6 + rng.uniform(0, 1, K)).astype(np.float32)
    if dist == "neg":
        return (-50.0 - 3.0 * rng.standard_normal(K)).astype(np.float32)
    J = a.astype(np.float32) + np.float32(0.5)
    if dist == "dupmin":   # the minimum twice, on both sides of a 4096-sample workgroup boundary (of each half)
        for p in ((4095, 4096) if K > 4096 else (K // 3, K - 2)):
            J[p] = -1.0
        if K // 2 + 4097 < K:
            J[K // 2 + 4095] = J[K // 2 + 4096] = -1.0
        return J
    if dist == "tie":      # distinct costs whose float32 weights are equal: the first index of the max wins (3 and
        h = K // 2         # 3 + 256 share a thread in every form, 9 is another thread's)
        for base in (0, h):
            J[base + 3], J[base + (259 if h > 300 else 5)], J[base + 9] = 3e-9, 1e-9, 0.0
        return J
    if dist == "zeros":    # -0.0 and +0.0 (equal costs, ordered by index), three per half
        h = K // 2
        for base in (0, h):
            J[base + 2], J[base + 7], J[base + min(h - 1, 20)] = 0.0, -0.0, 0.0
        J[1] = -0.0
        return J
    if dist == "inf":
        J[rng.choice(K, 5, replace=False)] = np.inf
        return J
    if dist == "inf24":    # more than 4 of 24 at +inf: the top-20 holds +inf rows
        J[[1, 4, 9, 13, 17, 22]] = np.inf
        return J
    if dist == "stageA":
        J = stage_a_layout(K)
        assert stage_a_survivors(J) > 1024
        return J
    if dist == "stageB":   # every workgroup: 19 copies of F and 40 of C > F at its 20th place; the lists' first elements
        # are all F, so > 1024 of the 64 x 20 candidates pass stage B's bounds
        J = (10.0 + a).astype(np.float32)
        for b in range(K // 4096):
            pos = b * 4096 + rng.choice(4096, 59, replace=False)
            J[pos[:19]] = 1.0
            J[pos[19:]] = 2.0
        return J
    raise ValueError(dist)


def check_weights(w, J, beta, what):
    """w (kernel, float32) against the float64 weights at `beta` with the bound of the module docstring."""
    w_ref, eta_ref = R.weights_at(J, beta)
    J64 = J.astype(np.float64)
    with np.errstate(invalid="ignore"):
        x = np.abs(J64 - J64.min()) / beta
    big = w_ref >= 1e-30
    err = np.abs(w.astype(np.float64) - w_ref)
    bad = big & (err > (2e-5 + 4 * U32 * np.where(big, x, 0.0)) * w_ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} weights off, first at {np.flatnonzero(bad)[:5]}: " \
                          f"{w[bad][:3]} vs {w_ref[bad][:3]}"
    assert np.all(err[~big] <= 1e-30), f"{what}: tiny weights off by {err[~big].max()}"
    return w_ref, eta_ref


def search_like_kernel(JJ, iters, what):
    """The float64 search of m3p2i.py:24-44; if the kernel made a different number of passes, the deciding pass must
    graze 3 or 10 and the reference is re-run with that decision reversed."""
    r = R.update_infinite_beta(JJ - JJ.astype(np.float64).min(), 1.0, 10, 3)
    if r["iters"] != iters:
        p = min(r["iters"], iters)
        eta_p = r["etas"][p - 1]
        assert min(abs(eta_p - 3.0) / 3.0, abs(eta_p - 10.0) / 10.0) <= 1e-5, \
            f"{what}: {iters} passes, reference {r['iters']}, eta at pass {p} = {eta_p!r}"
        r = R.update_infinite_beta(JJ - JJ.astype(np.float64).min(), 1.0, 10, 3, flip_at=p)
        assert r["iters"] == iters, (what, iters, r["iters"])
    assert abs(r["beta32"] - r["beta"]) <= r["iters"] * U32 * r["beta"] * 1.01
    return r


def run_case(K, T, nu, mode, dist, entry, calls, cov, seed):
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipEngine, make_config
    panda = nu == 9
    kw = dict(u_min=[-2.0] * 7 + [-1.5] * 2, u_max=[2.0] * 7 + [1.5] * 2, noise_sigma_diag=[10.0] * 7 + [0.8] * 2,
              lambda_=0.05, dt=0.01, env_type="panda_env") if panda else \
        dict(u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3], lambda_=0.5 if mode == "simple" else 1.0)
    eng = HipEngine(make_config(K=K, T=T, nu=nu, multi_modal=mode == "multi", mode_simple=mode == "simple",
                                update_cov=cov, **kw))
    try:
        if entry == "five":
            eng.set_update_launches(5)
        rng = np.random.default_rng(seed)
        half = K // 2
        ss = float(eng.cfg.step_size_mean)
        sg_gain = _sg_gain()
        mean = rng.uniform(-1, 1, (T, nu)).astype(np.float32)
        eng.buffer(L.BUF_MEAN).copy_(torch.from_numpy(mean))
        mean_ref = mean.astype(np.float64)
        beta64, beta32 = 1.0, np.float32(1.0)
        cov_ref = np.array(list(eng.cfg.noise_sigma_diag)[:nu], np.float64)
        for call in range(calls):
            J = make_costs(dist, K, rng, call)
            A = rng.uniform(-3, 3, (T, K, nu)).astype(np.float32)
            S = rng.uniform(-5, 5, (T, K, 4)).astype(np.float32)
            eng.buffer(L.BUF_TRAJ_COST).copy_(torch.from_numpy(J))
            eng.buffer(L.BUF_ACTIONS).copy_(torch.from_numpy(A))
            eng.buffer(L.BUF_STATES).copy_(torch.from_numpy(S))
            if entry == "phases":
                eng.update()
                eng.finalize()
            else:
                eng.update_finalize()
            torch.cuda.synchronize()
            info = eng.info()
            out = {b: eng.buffer(b).cpu().numpy() for b in (L.BUF_WEIGHTS, L.BUF_MEAN, L.BUF_ACTION_OUT, L.BUF_TOP_IDX,
                                                             L.BUF_TOP_TRAJS, L.BUF_BEST, L.BUF_COV)}
            Akt = A.transpose(1, 0, 2)                         # [K, T, nu] (reference layout)
            tag = f"call {call}"
            w = out[L.BUF_WEIGHTS]
            # ---- weights, eta, beta, iters ----
            if mode == "multi":
                r = [search_like_kernel(J, info.iters, tag + " all"),
                     search_like_kernel(J[:half], info.iters_1, tag + " mode 1"),
                     search_like_kernel(J[half:], info.iters_2, tag + " mode 2")]
                assert np.float32(info.beta_1) == np.float32(r[1]["beta32"]) and \
                    np.float32(info.beta_2) == np.float32(r[2]["beta32"]), (info.beta_1, info.beta_2, r[1]["beta32"], r[2]["beta32"])
                w1, w2 = eng.buffer(L.BUF_WEIGHTS_1).cpu().numpy(), eng.buffer(L.BUF_WEIGHTS_2).cpu().numpy()
                wr, er = check_weights(w, J, r[0]["beta32"], tag + " weights")
                w1r, e1r = check_weights(w1, J[:half], r[1]["beta32"], tag + " weights_1")
                w2r, e2r = check_weights(w2, J[half:], r[2]["beta32"], tag + " weights_2")
                for got, want in ((info.eta, er), (info.eta_1, e1r), (info.eta_2, e2r)):
                    assert abs(got - want) <= 2e-5 * want, (tag, got, want)
                assert np.float32(info.beta) == np.float32(1.0)          # the persistent beta is never written
            else:
                b_used = (float(eng.cfg.lambda_) if mode == "simple" else float(beta32))
                wr, er = check_weights(w, J, b_used, tag + " weights")
                assert abs(info.eta - er) <= 2e-5 * er, (tag, info.eta, er)
                if mode == "single":
                    # mppi.py:446-454: panda_env adapts beta after use; point_env keeps it
                    _, eta64, nb64 = R.exp_util(J, beta64, panda)
                    step = nb64 / beta64
                    if panda and (abs(eta64 - 20) <= 2e-5 * 20 or abs(eta64 - 10) <= 2e-5 * 10):
                        step = info.beta / float(beta32)               # a grazing eta: either side is right
                    beta64 *= step
                    beta32 = np.float32(beta32 * np.float32(step)) if step != 1.0 else beta32
                    assert np.float32(info.beta) == beta32, (tag, info.beta, beta32)
                    assert abs(beta64 - float(beta32)) <= (call + 1) * 2 * U32 * beta64
            # ---- argmax (first index of the max of the returned weights), best rows ----
            bi = R.argmax_first(w)
            assert info.best_idx == bi, (tag, info.best_idx, bi)
            assert wr[bi] >= wr.max() * (1 - 1e-6)
            if mode == "multi":
                b1, b2 = R.argmax_first(w1), half + R.argmax_first(w2)
                assert (info.best_idx_1, info.best_idx_2) == (b1, b2), (tag, info.best_idx_1, info.best_idx_2, b1, b2)
                assert w1r[b1] >= w1r.max() * (1 - 1e-6) and w2r[b2 - half] >= w2r.max() * (1 - 1e-6)
                assert np.array_equal(eng.buffer(L.BUF_BEST_1).cpu().numpy(), A[:, b1])
                assert np.array_equal(eng.buffer(L.BUF_BEST_2).cpu().numpy(), A[:, b2])
            elif mode == "single":
                assert np.array_equal(out[L.BUF_BEST], A[:, bi])
            # ---- sums of the halves, pull preference (m3p2i.py:16-21) ----
            hp, hq = wr[:half].sum(), wr[half:].sum()
            assert abs(info.wsum_push - hp) <= 2e-5 and abs(info.wsum_pull - hq) <= 2e-5, (tag, info.wsum_push, hp, info.wsum_pull, hq)
            assert info.pull_preference == int(info.wsum_pull > info.wsum_push)
            if abs(hq - hp) > 1e-4:
                assert info.pull_preference == R.pull_preference(wr, half)
            # ---- top-k: the 20 largest reference weights, and the project's rule (ascending J, ties by index,
            # -0.0 == +0.0, as torch.argsort(J, stable=True)) ----
            ti = out[L.BUF_TOP_IDX].astype(np.int64)
            assert np.all((ti >= 0) & (ti < K)), ti
            _, vals = R.topk(wr)
            np.testing.assert_allclose(wr[ti], vals, rtol=1e-12, atol=0, err_msg=tag + " top-k weights")
            assert np.all(np.diff(wr[ti]) <= 0)
            want_ti = np.argsort(J, kind="stable")[:R.TOPK]
            assert np.array_equal(ti, want_ti), (tag, ti, want_ti)
            np.testing.assert_array_equal(out[L.BUF_TOP_TRAJS], S[:, ti][:, :, [0, 2]].transpose(1, 0, 2))
            # ---- means, filtered plan, covariance ----
            scale = float(np.abs(A).max())
            if mode == "simple":
                noise = Akt.astype(np.float64) - np.roll(mean_ref, -1, axis=0)[None]
                s = R.simple_update(J, noise, mean_ref, float(eng.cfg.lambda_))
                mean_ref = s["U"]
            elif mode == "multi":
                m = R.update_multi_modal_distribution([dict(w=wr), dict(w=w1r), dict(w=w2r)], Akt, R.shift_action(mean_ref), ss, half)
                np.testing.assert_allclose(eng.buffer(L.BUF_MEAN_1).cpu().numpy(), m["mean_1"], rtol=0, atol=1e-5 * scale, err_msg=tag)
                np.testing.assert_allclose(eng.buffer(L.BUF_MEAN_2).cpu().numpy(), m["mean_2"], rtol=0, atol=1e-5 * scale, err_msg=tag)
                mean_ref = m["mean"]
            else:
                m = R.update_distribution(wr, Akt, R.shift_action(mean_ref), ss, cov_ref if cov else None)
                mean_ref = m["mean"]
                if cov:
                    cov_ref = m["cov"]
                    c = out[L.BUF_COV]
                    np.testing.assert_allclose(c[0], m["cov"], rtol=0, atol=1e-5 * m["cov"].max(), err_msg=tag + " cov")
                    np.testing.assert_allclose(c[1], m["scale_tril"], rtol=0, atol=1e-5 * m["scale_tril"].max(), err_msg=tag + " scale_tril")
            np.testing.assert_allclose(out[L.BUF_MEAN], mean_ref, rtol=0, atol=1e-5 * scale, err_msg=tag + " mean")
            np.testing.assert_allclose(out[L.BUF_ACTION_OUT], R.savgol(mean_ref), rtol=0, atol=sg_gain * 1e-5 * scale,
                                       err_msg=tag + " action_out")
    finally:
        eng.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_update_form_against_float64_reference(case):
    name, K, T, nu, mode, dist, entry, calls, cov = case
    run_case(K, T, nu, mode, dist, entry, calls, cov, seed=sum(map(ord, name)))
