"""Batched panda_env episodes (m3p2i_aip_amd/episodes.py run_panda_episodes, m3_panda_episodes_*) against
the serial loop of tools/closed_loop.run, episode by episode and bit for bit: ticks, success, timeline, final cube
positions, every trace and full row; subsets; the kernel form each planner chose; the refusals of
m3_panda_episodes_create; the batched band against band_stats.panda_episodes.

The unsuccessful ending: no cube jitter within the band's +-2 cm makes the pick-and-place fail at these sizes, so it is
covered by a max_ticks cut below the shortest success (test_a_max_ticks_cut_ends_unsuccessful_without_settling)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHIPPED = ["mppi.num_samples=200", "mppi.horizon=12"]
C4 = ["mppi.num_samples=4000", "mppi.horizon=20"]
TICKS = 600


def _tools():
    import band_stats
    import closed_loop
    return band_stats, closed_loop


def _jitter(e):
    rng = np.random.default_rng([77, e])          # band_stats.panda_episodes
    return dict(cube=(0.0, 0.0) if e == 0 else tuple(rng.uniform(-0.02, 0.02, 2).tolist()))


_SERIAL = {}


def _serial(ov, e, ticks=TICKS, settle=None):
    """closed_loop.run of one episode (+ the kernel form of its planner's last command, read before Tamp.close)."""
    bs, closed_loop = _tools()
    settle = bs.SETTLE_TICKS if settle is None else settle
    key = (tuple(ov), e, ticks, settle)
    if key not in _SERIAL:
        lps, close = [], closed_loop.Tamp.close

        def closing(self):
            lps.append(self.motion_planner._engine.panda_lanes_per_sample_used())
            close(self)

        closed_loop.Tamp.close = closing
        try:
            r = closed_loop.run("config_panda", list(ov), ticks=ticks, jitter=_jitter(e), settle_ticks=settle, trace=True)
        finally:
            closed_loop.Tamp.close = close
        r["lanes_per_sample_used"] = lps[-1]
        _SERIAL[key] = r
    return _SERIAL[key]


def _bits(x):
    return np.asarray(x, np.float64).tobytes()


def _same(a, b, what=""):
    """a: batched report, b: closed_loop.run's.  Floats as bits."""
    print(what, "ticks", a["ticks"], b["ticks"], "success", a["success"], b["success"], "xy", a["cube_to_goal_xy"], b["cube_to_goal_xy"],
          "dz", a["cube_height_above_goal"], b["cube_height_above_goal"], "timeline", a["timeline"], b["timeline"])
    assert a["success"] == b["success"] and a["ticks"] == b["ticks"]
    assert a["timeline"] == [tuple(x) for x in b["timeline"]]
    assert a["sim_time_s"] == b["sim_time_s"]
    assert _bits(a["cube_to_goal_xy"]) == _bits(b["cube_to_goal_xy"])
    assert _bits(a["cube_height_above_goal"]) == _bits(b["cube_height_above_goal"])
    assert len(a["trace"]) == len(b["trace"]) and len(a.get("full", [])) == len(b.get("full", []))
    for i, (x, y) in enumerate(zip(a["trace"], b["trace"])):
        assert x[0] == y[0] and _bits(x[1:]) == _bits(y[1:]), (what, "trace row", i, x, y)
    for i, (x, y) in enumerate(zip(a.get("full", []), b.get("full", []))):
        assert x["tick"] == y["tick"] and x["task"] == y["task"], (what, "full row", i)
        for k in ("dof_state", "root_state", "action"):
            assert _bits(x[k]) == _bits(y[k]), (what, "full row", i, k)


def test_shipped_size_episodes_equal_the_serial_loop_bit_for_bit():
    from m3p2i_aip_amd.episodes import run_panda_episodes
    bs, _ = _tools()
    eps = [("config_panda", SHIPPED, _jitter(e)) for e in range(5)]
    reps = run_panda_episodes(eps, max_ticks=TICKS, settle_ticks=bs.SETTLE_TICKS, trace=True)
    for e, r in enumerate(reps):
        s = _serial(SHIPPED, e)
        _same(r, s, f"shipped episode {e}")
        # the kernel form is each planner's own choice: the same as in the serial run at its last command
        assert r["lanes_per_sample_used"] == s["lanes_per_sample_used"], (e, r["lanes_per_sample_used"], s["lanes_per_sample_used"])
    assert any(r["success"] for r in reps)          # (the set contains a success)


def test_c4_size_episode_equals_the_serial_loop_bit_for_bit():
    from m3p2i_aip_amd.episodes import run_panda_episodes
    bs, _ = _tools()
    r = run_panda_episodes([("config_panda", C4, _jitter(1))], max_ticks=TICKS, settle_ticks=bs.SETTLE_TICKS, trace=True)[0]
    s = _serial(C4, 1)
    _same(r, s, "C4 episode 1")
    assert r["lanes_per_sample_used"] == s["lanes_per_sample_used"]


def test_settling_after_success_equals_the_serial_loop():
    """settle_ticks > 0 (band_stats.SETTLE_TICKS is 0): the world steps on under the zero action before the cube positions
    are taken, one episode settling while the others still run."""
    from m3p2i_aip_amd.episodes import run_panda_episodes
    eps = [("config_panda", SHIPPED, _jitter(e)) for e in (0, 2)]
    reps = run_panda_episodes(eps, max_ticks=TICKS, settle_ticks=7, trace=True)
    for e, r in zip((0, 2), reps):
        _same(r, _serial(SHIPPED, e, settle=7), f"settle 7, episode {e}")
    assert any(r["success"] for r in reps)


def test_a_max_ticks_cut_ends_unsuccessful_without_settling():
    """The unsuccessful ending: max_ticks below the shortest success of the set (so: every episode runs out of ticks)."""
    from m3p2i_aip_amd.episodes import run_panda_episodes
    shortest = min(_serial(SHIPPED, e)["ticks"] for e in range(3) if _serial(SHIPPED, e)["success"])
    cut = shortest - 5
    assert cut > 20
    eps = [("config_panda", SHIPPED, _jitter(e)) for e in range(3)]
    reps = run_panda_episodes(eps, max_ticks=cut, settle_ticks=4, trace=True)
    for e, r in enumerate(reps):
        assert not r["success"] and r["ticks"] == cut
        _same(r, _serial(SHIPPED, e, ticks=cut, settle=4), f"cut at {cut}, episode {e}")


def test_subsets_give_the_same_episodes():
    """A set whose episodes end at different ticks gives each episode what a set of one gives it."""
    from m3p2i_aip_amd.episodes import run_panda_episodes
    eps = [("config_panda", SHIPPED, _jitter(e)) for e in range(4)]
    together = run_panda_episodes(eps, max_ticks=TICKS, trace=True)
    assert len({r["ticks"] for r in together}) > 1
    for e, (ep, r) in enumerate(zip(eps, together)):
        alone = run_panda_episodes([ep], max_ticks=TICKS, trace=True)[0]
        _same(r, dict(alone, timeline=[list(x) for x in alone["timeline"]]), f"subset, episode {e}")


def test_batched_band_equals_the_serial_band():
    bs, _ = _tools()
    for ov in (SHIPPED, C4):
        a, b = bs.panda_episodes_batched(4, ov), bs.panda_episodes(4, ov)
        assert a["successes"] == b["successes"] and a["final_xy_error_m"] == b["final_xy_error_m"]
        assert a["ticks_to_success"] == b["ticks_to_success"]
        for x, y in zip(a["runs"], b["runs"]):
            assert x["timeline"] == [tuple(t) for t in y["timeline"]]
            assert {k: v for k, v in x.items() if k != "timeline"} == {k: v for k, v in y.items() if k != "timeline"}


def test_create_refusals_leave_the_handles_as_they_were():
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipEngine, HipPandaEpisodes, make_config
    from m3p2i_aip_amd.episodes import build_panda_set, run_point_episodes
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymWrapper
    es = build_panda_set([("config_panda", SHIPPED, _jitter(e)) for e in range(2)], max_ticks=40)
    try:
        es.eps.close()
        world = es.real._engine
        engs = [s.motion_planner._engine for s in es.sides]

        def snapshot():
            torch.cuda.synchronize()
            return [(e.buffer(L.BUF_MEAN).clone(), e.buffer(L.BUF_INFO).clone(), e._action_out) for e in engs]

        before = snapshot()

        def refused(fragment, *args, **kw):
            with pytest.raises(L.M3Error, match=fragment):
                HipPandaEpisodes(*args, **kw)

        refused("sim_only panda_env", engs[0], engs, 10)                                   # a planner as the world
        three = HipEngine(make_config(K=3, K_local=3, T=1, nu=9, env_type="panda_env", sim_only=True, filter_u=False))
        refused("sim_only panda_env", three, engs, 10)                                      # world without views
        icfg = es.sides[0].cfg.isaacgym
        wp = IsaacGymWrapper(icfg, "point_env", num_envs=2)
        refused("sim_only panda_env", wp._engine, engs, 10)                                 # a point_env world
        w3 = IsaacGymWrapper(icfg, "panda_env", num_envs=3)
        refused("K_local must equal n", w3._engine, engs, 10)
        refused("max_ticks", world, engs, 0)
        refused("settle_ticks", world, engs, 10, settle_ticks=-1)
        refused("listed twice", world, [engs[0], engs[0]], 10)
        point = HipEngine(make_config(K=200, T=15, nu=2, u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3]))
        refused("point_env planner", world, [engs[0], point], 10)
        fresh = HipEngine(make_config(K=200, T=12, nu=9, env_type="panda_env"))
        fresh.set_action_out(torch.zeros(12, 9, device="cuda"))
        refused("planner 1: .*noise", world, [engs[0], fresh], 10)                        # what the batch refuses
        side = torch.cuda.Stream()
        engs[1].use_torch_stream(side)
        refused("stream differs", world, engs, 10)
        engs[1].use_torch_stream()
        keep = engs[1]._action_out
        engs[1].set_action_out(None)
        refused("action-out", world, engs, 10)
        engs[1].set_action_out(keep)
        after = snapshot()
        for (m0, i0, a0), (m1, i1, a1) in zip(before, after):
            assert torch.equal(m0, m1) and torch.equal(i0, i1) and a0 is a1
        for h in (three, point, fresh):
            h.close()
        wp.stop_sim()
        w3.stop_sim()
        # and the same handles make a working set afterwards: the whole episodes, equal to the serial loop
        es.eps = HipPandaEpisodes(world, engs, 40, trace=False)
        es.run()
        for e, r in enumerate(es.reports()):
            s = _serial(SHIPPED, e, ticks=40)
            assert (r["ticks"], r["success"]) == (s["ticks"], s["success"])
            assert _bits(r["cube_to_goal_xy"]) == _bits(s["cube_to_goal_xy"])
        # misuse of the tick protocol and the other family's refusal
        with pytest.raises(L.M3Error, match="ended and settled"):
            es.eps.observe()
        with pytest.raises(ValueError, match="point_env only"):
            run_point_episodes([("config_panda", SHIPPED, None)], max_ticks=5)
    finally:
        es.close()
