"""CPU self-check of the harness of tests/test_sharded_update_f64_gpu.py: the same driver, cost layouts, hand-made
collectives and float64 comparison (tests/sharded_update_driver.py), run on tests/oracle_engine.OracleEngine -- the
float32 NumPy restatement of the sharded protocols the gloo sharding tests rest on -- for the point_env cases it supports
(gather + reduce and shard_mix 1 / 2 / 3, single and multi-modal; simple mode and Panda stay GPU-only).  A correct float32
implementation must stay inside the bars derived in the GPU module's docstring; where the OracleEngine misses one, the
float64 reference decides which side is wrong.  What it cannot show: the OracleEngine forms the weights of shard_mix = 2 / 3
with the oracle's update on all gathered costs, it does not mix per-rank ladder tables; so the mixture term of the bound is
exercised here by the k_mix emulation (shard_mix = 1, single mode) only, and for 2 / 3 this module checks the case generators,
the collectives, the re-generated actions, the top-k merge and the second record."""
import pytest

from tests.sharded_update_driver import Case, OracleBackend, run_sharded_case

CASES = [
    # ---- gather + reduce ----
    Case("gr_single_unequal_300_251_450", 0, "single", [300, 251, 450], "s1"),
    Case("gr_single_N3_rank_all_inf", 0, "single", [40, 40, 40], "rank_inf"),
    Case("gr_multi_unequal_300_251_450_half_inside_rank1", 0, "multi", [300, 251, 450], "zeros_edge"),
    Case("gr_multi_N3_edge_tie_places_20_21", 0, "multi", [64, 64, 64], "edge_20_21"),
    # ---- shard_mix = 1, single mode: the mixture of local softmins ----
    Case("mix_single_N3_s1", 1, "single", [100, 100, 100], "s1"),
    Case("mix_single_N3_rank_all_inf", 1, "single", [40, 40, 40], "rank_inf"),
    Case("mix_single_N3_rank_some_inf", 1, "single", [40, 40, 40], "rank_some_inf"),
    Case("mix_single_N5_shift1e3", 1, "single", [30] * 5, "shift1e3"),
    Case("mix_single_N5_shift1e8", 1, "single", [30] * 5, "shift1e8"),
    Case("mix_single_N3_argmax_tie_in_three_ranks", 1, "single", [50, 50, 50], "tie3"),
    Case("mix_single_N32_Kl20_top20_spread", 1, "single", [20] * 32, "top20_spread"),
    Case("mix_single_N4_top20_one_rank", 1, "single", [60] * 4, "top20_one_rank"),
    Case("mix_single_N3_edge_tie_in_top20", 1, "single", [50, 50, 50], "edge_in"),
    Case("mix_single_N3_edge_tie_places_20_21", 1, "single", [50, 50, 50], "edge_20_21"),
    Case("mix_single_N3_dup_min_two_ranks", 1, "single", [50, 50, 50], "dup2ranks"),
    Case("mix_single_N2_last_sample_min", 1, "single", [64, 64], "lastmin"),
    Case("mix_single_N3_zeros_edge", 1, "single", [50, 50, 50], "zeros_edge"),
    Case("gr_single_N3_Kl8_inf24_inf_rows_in_top20", 0, "single", [8, 8, 8], "inf24"),
    Case("mix_single_N3_3calls_warm_start", 1, "single", [50, 50, 50], "s1", calls=3),
    # ---- shard_mix = 1 / 2 / 3, multi-modal ----
    Case("regen1_multi_N3_half_inside_rank1", 1, "multi", [40, 40, 40], "s1"),
    Case("regen1_multi_N3_rank_all_inf", 1, "multi", [40, 40, 40], "rank_inf"),
    Case("regen2_multi_N3_half_inside_rank1", 2, "multi", [40, 40, 40], "s1"),
    Case("regen2_multi_N3_no_null_action_u_scale2", 2, "multi", [40, 40, 40], "s1", null_action=False, u_scale=2.0),
    Case("regen2_multi_N3_rank_all_inf", 2, "multi", [40, 40, 40], "rank_inf"),
    Case("regen2_multi_N5_shift1e3", 2, "multi", [24] * 5, "shift1e3"),
    Case("regen2_multi_N3_spread1e-5_fallback", 2, "multi", [40, 40, 40], "s1e-5", min_iters=65),
    Case("regen2_multi_N3_argmax_tie_in_three_ranks", 2, "multi", [40] * 6, "tie3"),
    Case("p3_multi_N3_half_inside_rank1", 3, "multi", [40, 40, 40], "s1"),
    Case("p3_multi_N3_rank_all_inf", 3, "multi", [40, 40, 40], "rank_inf"),
    Case("p3_multi_N3_edge_tie_places_20_21", 3, "multi", [40, 40, 40], "edge_20_21"),
    Case("p3_multi_N3_spread1e8_fallback", 3, "multi", [40, 40, 40], "s1e8", min_iters=34),
    Case("p3_multi_N3_zeros_edge_cov_noop_3calls", 3, "multi", [40, 40, 40], "zeros_edge", calls=3, cov=True),
]


# ---- every protocol x every edge once: what the lists above leave out, filled in (small: K = 120, N = 3 unless the edge needs more) ----
PROTOCOLS = (("gr_single", 0, "single"), ("gr_multi", 0, "multi"), ("mix_single", 1, "single"), ("regen1_multi", 1, "multi"),
             ("regen2_multi", 2, "multi"), ("p3_multi", 3, "multi"))
EDGES = ("s1", "lastmin", "dup2ranks", "edge_in", "edge_20_21", "top20_one_rank", "top20_spread", "tie3", "zeros_edge", "rank_inf",
         "rank_some_inf", "mode_inf", "inf24", "shift1e3", "shift1e8", "s1e-5", "s1e8", "offset", "neg", "dupmin")
# shift1e8 under a multi-modal search: the float32 costs of a rank 1e8 r above rank 0 are all equal (ulp 8), so a half whose
# minimum lies in such a rank has > 10 samples tied at it and its search has no end, in the reference too: not a case.
# mode_inf concerns the per-set minima of the multi-modal records only.


def _edge_case(name, proto, mode, dist):
    multi = mode == "multi"
    if (dist == "shift1e8" and multi) or (dist == "mode_inf" and not multi):
        return None
    shards = [40, 40, 40]
    if dist == "top20_spread":
        shards = [22 if multi else 20] * 32
    elif dist == "tie3" and multi:
        shards = [40] * 6
    elif dist == "inf24":
        shards = [8, 8, 8] if proto == 0 else None      # (shard_mix needs K_local >= 20: a 24-sample vector is gather + reduce only)
    elif dist == "offset" and multi:
        shards = [22, 22, 22]                             # (few samples per half tied at the minimum: see the unsharded module)
    elif dist.startswith("shift"):
        shards = [24] * 5
    if shards is None:
        return None
    kw = dict(min_iters=65) if (dist == "s1e-5" and multi) else dict(min_iters=34) if (dist == "s1e8" and multi) else {}
    return Case(f"{name}_N{len(shards)}_Kl{shards[0]}_{dist}", proto, mode, shards, dist, **kw)


_have = {(c.proto, c.mode, c.dist) for c in CASES if c.nu == 2}
for _name, _proto, _mode in PROTOCOLS:
    for _dist in EDGES:
        _c = _edge_case(_name, _proto, _mode, _dist)
        if _c is not None and (_proto, _mode, _dist) not in _have:
            CASES.append(_c)
CASES += [
    Case("gr_multi_N3_cov_noop_3calls", 0, "multi", [40, 40, 40], "s1", calls=3, cov=True),
    Case("regen1_multi_N3_cov_noop_3calls", 1, "multi", [40, 40, 40], "s1", calls=3, cov=True),
    Case("regen1_multi_N3_no_null_action_u_scale2", 1, "multi", [40, 40, 40], "s1", null_action=False, u_scale=2.0),
]
assert len({c.id for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_oracle_engine_sharded_update_against_float64_reference(case):
    run_sharded_case(OracleBackend(), case, seed=sum(map(ord, case.id)))
