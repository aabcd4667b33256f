"""Lockstep point_env episodes whose planners have an arena per sample (m3_episodes_create_ex with M3_EPISODES_ROLLOUT_SCENES, a
batch with M3_BATCH_SECTION_POINT_ROLLOUT_SCENES) against the serial loop of tools/closed_loop.run,
episode by episode and bit for bit -- a nominal planner, two planners with `rollout_arena_spread` (one in a world of its own)
and a multi-modal one in one set; and the refusals of a set or a batch that was not created for such planners."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tests.test_episodes_gpu import _same  # noqa: E402

TICKS = 12
SIZE = ["mppi.num_samples=64", "mppi.horizon=12", "mppi.u_per_command=12"]   # (12: the shortest horizon the planner's degree-2 spline sampler takes)
PUSH = ["task=push", "goal=[-3,3]"] + SIZE
SPREAD = "rollout_arena_spread={spread: 0.3, seed: %d}"
EPISODES = [
    ("config_point", PUSH, dict(dyn_phase=0, box=(0.0, 0.0), robot=(0.0, 0.0))),
    ("config_point", PUSH + [SPREAD % 1], dict(dyn_phase=24, box=(0.02, -0.03), robot=(-0.01, 0.04))),
    ("config_point", PUSH + [SPREAD % 2, "world_point_scene={box_m: 5.0, box_I: 0.15, mu_rb: 0.3}"],
     dict(dyn_phase=76, box=(-0.04, 0.01), robot=(0.03, 0.02))),
    ("config_point", ["task=push_pull", "multi_modal=True", "goal=[-3.75,-3.75]", "mppi.num_samples=100", "mppi.horizon=12",
                      "mppi.u_per_command=12", SPREAD % 3], dict(dyn_phase=50, box=(0.01, 0.01), robot=(0.0, -0.02))),
]


def test_lockstep_episodes_with_arenas_per_sample_equal_the_serial_loop():
    import closed_loop
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.episodes import build_set
    es = build_set(EPISODES, max_ticks=TICKS, trace=True, point_runtime=True)
    try:
        assert es.eps.flags() == L.EPISODES_ROLLOUT_SCENES and es.batch.flags() == L.BATCH_SECTION_POINT_ROLLOUT_SCENES
        es.run()
        # (the tick-0 probe kept the fused path, and the engines hold the rows from then on)
        assert [s.motion_planner._engine.point_rollout_scenes_set() for s in es.sides] == [False, True, True, True]
        reps = es.reports()
    finally:
        es.close()
    for (cn, ov, j), r in zip(EPISODES, reps):
        s = closed_loop.run(cn, ov, ticks=TICKS, jitter=j, trace=True)
        _same(r, s)
        assert r["ticks"] == TICKS and len(r["trace"]) == TICKS       # (twelve ticks: no episode ends, every row is compared)


def test_sets_and_batches_without_the_flag_refuse_such_planners():
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipBatch, HipEpisodes
    from m3p2i_aip_amd.episodes import build_set
    from tests import rollout_scenes_fixture as R
    es = build_set(EPISODES[:2], max_ticks=TICKS, point_runtime=True)
    try:
        es.start()
        world = es.real._engine
        engs = [s.motion_planner._engine for s in es.sides]
        assert [e.point_rollout_scenes_set() for e in engs] == [False, True]
        spec = [("push", (-3.0, 3.0), 0, L.SUCTION_OFF, 400.0)] * 2
        es.eps.close()

        def snapshot():
            torch.cuda.synchronize()
            return [(e.buffer(L.BUF_MEAN).clone(), e.buffer(L.BUF_TRAJ_COST).clone(), e.info().calls) for e in engs], \
                world.buffer(L.BUF_SIM_WORLD).clone()

        def unchanged(before):
            after = snapshot()
            for (m0, j0, c0), (m1, j1, c1) in zip(before[0], after[0]):
                assert torch.equal(m0, m1) and torch.equal(j0, j1) and c0 == c1
            assert torch.equal(before[1], after[1])

        before = snapshot()
        # flags == 0 is m3_episodes_create: refused at create
        with pytest.raises(L.M3Error, match=r"error -5: m3_episodes_create: planner 1: it has an arena per sample"):
            HipEpisodes(world, engs, spec, TICKS)
        unchanged(before)
        # ... and at tick when the rows are set afterwards
        rows = R.cycle_rows(64)
        engs[1].set_point_rollout_scenes(None)
        plain = HipEpisodes(world, engs, spec, TICKS)
        batch = HipBatch(2, point_runtime=True)
        try:
            assert plain.flags() == 0
            engs[1].set_point_rollout_scenes(rows)
            before = snapshot()
            with pytest.raises(L.M3Error, match=r"error -5: m3_episodes_tick: planner 1: it has an arena per sample"):
                plain.tick(batch)
            unchanged(before)
            assert plain.ticks_done == 0
        finally:
            plain.close()
        # a flagged set and a batch without the section: the batch's own refusal, nothing launched
        flagged = HipEpisodes(world, engs, spec, TICKS, point_runtime=True)
        small = HipBatch(2)
        try:
            before = snapshot()
            with pytest.raises(L.M3Error, match=r"error -5: m3_episodes_tick: m3_batch_command: handle 1: it has an arena per sample "
                                                r"\(m3_set_point_rollout_scenes\), which only m3_rollout / m3_command run"):
                flagged.tick(small)
            unchanged(before)
            assert flagged.ticks_done == 0
            # rows cleared between two ticks apply from the next tick: the default batch then takes both planners
            flagged.tick(batch)
            engs[1].set_point_rollout_scenes(None)
            flagged.tick(small)
            assert flagged.ticks_done == 2 and small.launches()[0] == 1
            engs[1].set_point_rollout_scenes(rows)
            flagged.tick(batch)
            assert flagged.ticks_done == 3 and batch.launches()[0] == 2
        finally:
            small.close()
            batch.close()
            flagged.close()
    finally:
        es.close()
