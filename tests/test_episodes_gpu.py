"""Batched closed-loop episodes (m3p2i_aip_amd/episodes.py, m3_episodes_*) against the serial loop of
tools/closed_loop.run, episode by episode and bit for bit; the refusals of m3_episodes_create; subsets."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

TICKS = 300     # 15 s of simulated time: successes and time-outs both occur


def _tools():
    import band_stats
    import closed_loop
    return band_stats, closed_loop


def _episode_set():
    bs, _ = _tools()
    # dyn-obs phases on both sides of the walk's turning ticks (25 / 75 of each 100)
    phases = [24, 25, 26, 74, 75, 76, 0, 99, 49, 50, 23, 77, 124, 175, 1, 98]
    eps = []
    for k, sc in enumerate(bs.SCENARIOS):
        for r in range(2):
            j = bs.jitter_of(sc, 1 + r)
            j["dyn_phase"] = phases[2 * k + r]
            eps.append(("config_point", bs.overrides(sc, "default"), j))
    for sc in ("case2_halton_pull_coll", "corner1_hybrid"):
        for r in range(2):
            j = bs.jitter_of(sc, 3 + r)
            j["dyn_phase"] = (24, 76)[r]
            eps.append(("config_point", bs.overrides(sc, "baseline"), j))
    return eps


def _same(a, b):
    assert a["success"] == b["success"] and a["ticks"] == b["ticks"], (a["success"], a["ticks"], b["success"], b["ticks"])
    assert a["final_pos_error"] == b["final_pos_error"]
    assert a["dyn_obs_collision_ticks"] == b["dyn_obs_collision_ticks"]
    assert a["timeline"] == [tuple(x) for x in b["timeline"]]
    assert a["sim_time_s"] == b["sim_time_s"]
    assert len(a["trace"]) == len(b["trace"])
    for i, (x, y) in enumerate(zip(a["trace"], b["trace"])):
        assert x == y, (i, x, y)


def test_batched_episodes_equal_the_serial_loop_bit_for_bit():
    from m3p2i_aip_amd.episodes import run_point_episodes
    _, closed_loop = _tools()
    eps = _episode_set()
    reps = run_point_episodes(eps, max_ticks=TICKS, trace=True)
    outcomes = set()
    for (cn, ov, j), r in zip(eps, reps):
        s = closed_loop.run(cn, ov, ticks=TICKS, jitter=j, trace=True)
        _same(r, s)
        outcomes.add(r["success"])
    assert outcomes == {True, False}        # (the set covers both endings)


def test_subsets_give_the_same_episodes():
    """A set whose episodes end at different ticks gives each episode what a set of one gives it."""
    from m3p2i_aip_amd.episodes import run_point_episodes
    bs, _ = _tools()
    eps = [("config_point", bs.overrides(sc, "default"), bs.jitter_of(sc, e))
           for sc, e in (("case2_halton_push_coll", 0), ("corner1_pull", 2), ("corner2_push", 1), ("corner1_hybrid", 3))]
    together = run_point_episodes(eps, max_ticks=200, trace=True)
    assert len({r["ticks"] for r in together}) > 1
    for ep, r in zip(eps, together):
        _same(r, run_point_episodes([ep], max_ticks=200, trace=True)[0])


def test_create_refusals_leave_the_handles_as_they_were():
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipEngine, HipEpisodes, make_config
    from m3p2i_aip_amd.episodes import build_set
    bs, _ = _tools()
    es = build_set([("config_point", bs.overrides("case2_halton_push_coll", "default"), bs.jitter_of("case2_halton_push_coll", e))
                    for e in range(2)], max_ticks=50)
    try:
        es.eps.close()
        world = es.real._engine
        engs = [s.motion_planner._engine for s in es.sides]
        spec = [("push", (-3.0, 3.0), 0, L.SUCTION_OFF, 400.0)] * 2

        def snapshot():
            torch.cuda.synchronize()
            return [(e.buffer(L.BUF_MEAN).clone(), e.buffer(L.BUF_INFO).clone(), e._action_out) for e in engs]

        before = snapshot()

        def refused(fragment, *args, **kw):
            with pytest.raises(L.M3Error, match=fragment):
                HipEpisodes(*args, **kw)

        refused("sim_only point_env", engs[0], engs, spec, 10)                              # a planner as the world
        three = HipEngine(make_config(K=3, K_local=3, T=1, nu=2, sim_only=True, filter_u=False))
        refused("sim_only point_env", three, engs, spec, 10)                                 # world without views
        from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymWrapper
        w3 = IsaacGymWrapper(es.sides[0].cfg.isaacgym, "point_env", num_envs=3)
        refused("K_local must equal n", w3._engine, engs, spec, 10)
        refused("max_ticks", world, engs, spec, 0)
        refused("listed twice", world, [engs[0], engs[0]], spec, 10)
        panda = HipEngine(make_config(K=256, T=12, nu=9, env_type="panda_env"))
        refused("panda_env planner", world, [engs[0], panda], spec, 10)
        fresh = HipEngine(make_config(K=200, T=15, nu=2, u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3]))
        fresh.set_action_out(torch.zeros(15, 2, device="cuda"))
        refused("planner 1: .*noise", world, [engs[0], fresh], spec, 10)                   # what the batch refuses
        side = torch.cuda.Stream()
        engs[1].use_torch_stream(side)
        refused("stream differs", world, engs, spec, 10)
        engs[1].use_torch_stream()
        keep = engs[1]._action_out
        engs[1].set_action_out(None)
        refused("action-out", world, engs, spec, 10)
        engs[1].set_action_out(keep)
        after = snapshot()
        for (m0, i0, a0), (m1, i1, a1) in zip(before, after):
            assert torch.equal(m0, m1) and torch.equal(i0, i1) and a0 is a1
        # and the same handles make a working set afterwards
        ok = HipEpisodes(world, engs, spec, 10)
        ok.close()
        for h in (three, panda, fresh):
            h.close()
        w3.stop_sim()
    finally:
        es.close()
