"""The behaviour band of tests/test_behaviour_band_gpu.py at the logged N = 60, through the batched closed loop
(tools/band_stats.episodes_batched / band_batched: every episode of every scenario and size in lockstep).

Means and spreads of the final error and the task time: the rules of the serial test, one-sided where it is one-sided.
Success counts (fewer than logged) and episodes with a dyn-obs collision (more than logged): a one-sided Fisher exact test
at alpha = 0.01 of this build's count out of N against the logged count out of the logged n (tools/band_stats.py
fisher_one_sided).  At N = 8 the serial test's floors have almost no power (int(0.15 * 8) = 1); here the test is stated."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = json.load(open(os.path.join(ROOT, "tests", "golden", "behaviour_band.json")))
N = 60
ALPHA = 0.01
# the logged runs that ended by reaching the goal (as tests/test_behaviour_band_gpu.py LOGGED_SUCCESS, as counts of the
# logged n: case2 60 runs each, the corner scenarios 20)
LOGGED_SUCCESSES = {"case2_halton_push_coll": 60, "case2_halton_pull_coll": 45, "corner1_push": 20, "corner1_pull": 11,
                    "corner1_hybrid": 20, "corner2_push": 3, "corner2_pull": 9, "corner2_hybrid": 20}
FASTER_THAN_LOGGED = ("corner2_push", "corner2_pull")
SIZES = ("baseline", "default")


def _bs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import band_stats
    return band_stats


_RESULTS = {}


def _results():
    if not _RESULTS:
        _RESULTS.update(_bs().band_batched([(sc, size) for size in SIZES for sc in LOGGED_SUCCESSES], n=N, max_sim_time_s=40.0))
    return _RESULTS


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("scenario", list(LOGGED_SUCCESSES))
def test_point_env_band_at_n60(scenario, size):
    bs = _bs()
    band = BAND["point"][scenario]
    r = _results()[(scenario, size)]
    msg = json.dumps({k: v for k, v in r.items() if k != "runs"})
    n_log = band["task_time_s"]["n"]
    s_log = LOGGED_SUCCESSES[scenario]
    p = bs.fisher_one_sided(r["successes"], N - r["successes"], s_log, n_log - s_log, "less")
    assert p >= ALPHA, ("fewer successes than logged", p, msg)
    c_log = int(round(band["dyn_obs_collisions"]["mean"] * band["dyn_obs_collisions"]["n"]))
    c = r["dyn_obs_collided_episodes"]
    p = bs.fisher_one_sided(c, N - c, c_log, band["dyn_obs_collisions"]["n"] - c_log, "greater")
    assert p >= ALPHA, ("more collided episodes than logged", p, msg)
    if r["successes"] == 0:
        return
    for key in ("final_pos_error_m", "task_time_s"):
        ours, ref = r[key], band[key]
        if key == "final_pos_error_m" or scenario in FASTER_THAN_LOGGED:
            assert ours["mean"] <= ref["mean"] + 3.0 * ref["std"], (key, msg)
        else:
            assert abs(ours["mean"] - ref["mean"]) <= 3.0 * ref["std"], (key, msg)
        assert ours["std"] <= 3.0 * ref["std"], (key, msg)
