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

from tests.update_f64_checks import check_call, make_costs, new_state

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


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
        ss = float(eng.cfg.step_size_mean)
        mean = rng.uniform(-1, 1, (T, nu)).astype(np.float32)
        eng.buffer(L.BUF_MEAN).copy_(torch.from_numpy(mean))
        st = new_state(mean, list(eng.cfg.noise_sigma_diag)[:nu])
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
            check_call(L, lambda b: eng.buffer(b).cpu().numpy(), eng.info(), J, A, S, st, K=K, nu=nu, mode=mode, cov=cov,
                       lambda_=float(eng.cfg.lambda_), ss=ss, call=call)
    finally:
        eng.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_update_form_against_float64_reference(case):
    name, K, T, nu, mode, dist, entry, calls, cov = case
    run_case(K, T, nu, mode, dist, entry, calls, cov, seed=sum(map(ord, name)))
