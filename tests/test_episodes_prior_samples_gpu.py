"""Lockstep point_env episodes whose planners take prior samples from a controller on the device (m3_episodes_create_ex with
M3_EPISODES_PRIORS, a batch with M3_BATCH_SECTION_POINT_PRIORS) against the serial loop of
tools/closed_loop.run with the same `prior_samples={..., device: true}` key, episode by episode and bit for bit -- push with
push_behind, navigation with go_to, a multi-modal push_pull with priors in both halves and a nominal planner in one set; priors
set and cleared between two ticks; the refusals of a set or a batch that was not created for such planners; and the ValueErrors
of the Python layer."""
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
DEV = "prior_samples={controller: %s, n: 4, device: true}"
EPISODES = [
    ("config_point", PUSH + [DEV % "push_behind"], dict(dyn_phase=0, box=(0.0, 0.0), robot=(0.0, 0.0))),
    ("config_point", ["task=navigation", "goal=[-3,3]"] + SIZE + [DEV % "go_to"], dict(dyn_phase=24, box=(0.02, -0.03), robot=(-0.01, 0.04))),
    ("config_point", ["task=push_pull", "multi_modal=True", "goal=[-3.75,-3.75]", "mppi.num_samples=100", "mppi.horizon=12",
                      "mppi.u_per_command=12", DEV % "push_behind"], dict(dyn_phase=50, box=(0.01, 0.01), robot=(0.0, -0.02))),
    ("config_point", PUSH, dict(dyn_phase=76, box=(-0.04, 0.01), robot=(0.03, 0.02))),
]


def test_lockstep_episodes_with_device_controllers_equal_the_serial_loop():
    import closed_loop
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.episodes import build_set
    es = build_set(EPISODES, max_ticks=TICKS, trace=True, point_priors=True)
    try:
        assert es.eps.flags() == L.EPISODES_PRIORS and es.batch.flags() == L.BATCH_SECTION_POINT_PRIORS
        live = None
        es.start()
        while es.running:
            if es.eps.ticks_done == 2:
                live = L.load().m3_owned_blocks_live()
            es.tick()
        assert L.load().m3_owned_blocks_live() == live           # a tick allocates nothing
        engs = [s.motion_planner._engine for s in es.sides]
        # (the tick-0 probe kept the fused path; the controllers as the key asks, multi-modal: two priors in each half)
        assert [(e.prior_controller() or {}).get("kind", 0) for e in engs] == [2, 1, 2, 0]
        assert [e.prior_samples_set() for e in engs] == [4, 4, 4, 0] and [e.prior_samples_used() for e in engs[:3]] == [1, 1, 1]
        assert [engs[2].lib.m3_get_prior_sample(engs[2]._h, j, None, None) for j in range(4)] == [0] * 4
        assert es.batch.launches()[0] == 3        # (K = 64 priors, K = 100 priors, the nominal planner)
        reps = es.reports()
    finally:
        es.close()
    for (cn, ov, j), r in zip(EPISODES, reps):
        s = closed_loop.run(cn, ov, ticks=TICKS, jitter=j, trace=True)
        _same(r, s)
        assert r["ticks"] == TICKS and len(r["trace"]) == TICKS       # (twelve ticks: no episode ends, every row is compared)


def test_the_python_layer_refuses_what_a_lockstep_set_cannot_serve():
    from m3p2i_aip_amd.episodes import build_set, run_point_episodes
    host = ("config_point", PUSH + ["prior_samples={controller: push_behind, n: 4}"], None)
    with pytest.raises(ValueError, match="episode 1 asks for prior samples from a host controller"):
        build_set([EPISODES[3], host], max_ticks=TICKS, point_priors=True)
    with pytest.raises(ValueError, match="episode 0 asks for prior samples from a host controller"):
        run_point_episodes([host], max_ticks=TICKS)
    with pytest.raises(ValueError, match=r"episode 0 asks for prior samples \(prior_samples\), which the batched command runs only on request"):
        build_set(EPISODES[:1], max_ticks=TICKS)


def test_priors_between_ticks_and_sets_and_batches_without_the_flag():
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipBatch, HipEpisodes
    from m3p2i_aip_amd.episodes import build_set
    push = ("config_point", PUSH, dict(dyn_phase=0, box=(0.0, 0.0), robot=(0.0, 0.0)))
    es = build_set([push, EPISODES[0]], max_ticks=TICKS, point_priors=True)
    try:
        es.start()
        world = es.real._engine
        engs = [s.motion_planner._engine for s in es.sides]
        assert [e.prior_samples_set() for e in engs] == [0, 4]
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
        # sets without the flag: refused at create, in today's words
        for runtime in (False, True):
            with pytest.raises(L.M3Error, match=r"error -5: m3_episodes_create: planner 1: it has prior samples \(m3_set_prior_samples\)"):
                HipEpisodes(world, engs, spec, TICKS, point_runtime=runtime)
        unchanged(before)
        # unknown flag bits stay unknown
        import ctypes as C
        arr = (C.c_void_p * 2)(*[e._h.value for e in engs])
        for bits in (16, 2, 4, 8 | 2):
            out = C.c_void_p(1)
            assert world.lib.m3_episodes_create_ex(world._h, arr, None, 2, TICKS, 0, bits, C.byref(out)) == -1 and out.value is None
            assert b"unknown flag bits" in world.lib.m3_episodes_last_error(None)
        # a flagged set and a batch without the section: the batch's own refusal, ahead of the pre kernel -- nothing launched
        flagged = HipEpisodes(world, engs, spec, TICKS, point_priors=True)
        small, batch = HipBatch(2), HipBatch(2, point_priors=True)
        try:
            assert flagged.flags() == L.EPISODES_PRIORS
            before = snapshot()
            with pytest.raises(L.M3Error, match=r"error -5: m3_episodes_tick: m3_batch_command: handle 1: it has prior samples "
                                                r"\(m3_set_prior_samples\), which only m3_rollout / m3_command run"):
                flagged.tick(small)
            unchanged(before)
            assert flagged.ticks_done == 0
            flagged.tick(batch)
            assert flagged.ticks_done == 1 and batch.launches()[0] == 2
            # priors cleared between two ticks apply from the next tick: the default batch then takes both planners in one group
            engs[1].set_prior_controller(None)
            flagged.tick(small)
            assert flagged.ticks_done == 2 and small.launches()[0] == 1
            # ... and set again, on the other planner as well: one priors group
            engs[1].set_prior_controller("push_behind", 4)
            engs[0].set_prior_controller("go_to", 2, [5, 9])
            flagged.tick(batch)
            assert flagged.ticks_done == 3 and batch.launches()[0] == 1
            assert [e.prior_samples_used() for e in engs] == [1, 1]
            # begin / end of such a set take planners with priors
            flagged.begin()
            flagged.end()
            assert flagged.ticks_done == 4
        finally:
            small.close()
            batch.close()
            flagged.close()
    finally:
        es.close()
