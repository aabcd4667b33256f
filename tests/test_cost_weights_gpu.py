"""The point_env cost weights on the GPU: m3_set_point_cost_weights through the fused command, the batched command, the
lockstep episodes, sharded handles and the step-mode cost (include/m3p2i_hip.h).

  identity   the weighted kernels at the default weights leave the bytes the ordinary kernels leave
  scaling    outer weights and the softmin's temperature times a power of two: costs scale exactly, weights / plan / top-k keep their bits
  values     m3_cost equals the float32 restatement (tests/point_cost_ref.py) to the last bit -- the bound fixed in
             tests/test_cost_weights_cpu.py: both are the same sequence of correctly rounded binary32 operations (hipcc
             without contraction or fast-math: IEEE add / multiply, correctly rounded division and sqrt) -- and the fused
             rollout's per-step costs equal step + m3_cost replayed, bit for bit
  planner    a planner with `cost_weights` in its config keeps the fused path at its probe
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, make_config  # noqa: E402
from tests import point_cost_ref as R  # noqa: E402
from tests.test_batch_command_gpu import BUFS, L_ERR, PK, Twin, _noise, _run, _world  # noqa: E402

F = np.float32
OUTER = ("nav_dist", "collision", "push_dist", "push_align", "pull_dist", "pull_vel", "pull_align")
W_A = dict(push_align=2.5)
W_B = dict(nav_dist=0.5, collision=250.0, robot_box=2.0, box_goal=4.0, push_dist=1.5, push_align=-1.0, pull_dist=2.0,
           pull_vel=0.0, pull_align=3.0)


@pytest.fixture
def twins():
    made = []
    yield made
    for t in made:
        t.close()


def _weights(t, A=None, B=None, force_A=None):
    """the cost weights / the weighted-instance switch of a Twin's two handles"""
    if A is not None:
        t.A.set_point_cost_weights(A)
    if B is not None:
        t.B.set_point_cost_weights(B)
    if force_A is not None:
        t.A.set_weighted_cost_instance(force_A)
    return t


# ------------------------------------------------------------------ 4. entry points (fails on the parent)
def test_entry_points_round_trip():
    lib = L.load()
    e = HipEngine(make_config(K=200, T=15, nu=2, **PK))
    try:
        assert e.point_cost_weights() == L.COST_WEIGHT_DEFAULTS
        e.set_point_cost_weights(W_B)
        assert e.point_cost_weights() == {k: float(F(v)) for k, v in W_B.items()}
        e.set_point_cost_weights(W_A)                       # (missing keys: the defaults, not the last values)
        assert e.point_cost_weights() == {**L.COST_WEIGHT_DEFAULTS, **W_A}
        e.reset()                                           # per-handle state like the objective: survives m3_reset
        assert e.point_cost_weights()["push_align"] == 2.5
        e.set_point_cost_weights(None)
        assert e.point_cost_weights() == L.COST_WEIGHT_DEFAULTS
        w = L.PointCostWeights()
        lib.m3_default_point_cost_weights(C.byref(w))
        assert {n: getattr(w, n) for n in R.NAMES} == L.COST_WEIGHT_DEFAULTS
    finally:
        e.close()


# ------------------------------------------------------------------ 5. identity
IDENTITY = [dict(K=200, T=15, task="navigation", goal=(2.0, -2.0)),
            dict(K=2000, T=30, task="push", goal=(-1.0, -1.0)),
            dict(K=2000, T=15, task="pull", goal=(0.0, 0.0)),
            dict(K=4000, T=30, task="push_pull", goal=(-3.75, -3.75), multi_modal=True),
            dict(K=2000, T=30, task="push", goal=(-1.0, -1.0), sampling_random=True),
            dict(K=2000, T=30, task="pull", goal=(0.0, 0.0), mode_simple=True, sampling_random=True, u_per_command=10),
            dict(K=2000, T=30, task="push", goal=(-1.0, -1.0), avoid=True),
            dict(K=2000, T=30, task="navigation", goal=(2.0, -2.0), bind=True),
            dict(K=4000, T=30, task="push_pull", goal=(-3.75, -3.75), multi_modal=True, bind=True)]


def test_weighted_instance_at_default_weights_is_the_ordinary_command(twins):
    """A: the weighted instance forced on, default weights; B: the ordinary handle.  Six warm-started m3_commands each."""
    twins += [_weights(Twin(i, **s), force_A=1) for i, s in enumerate(IDENTITY)]
    for c in range(6):
        for t in twins:
            t.set_world(c)
            t.A.command()
            t.B.command()
        torch.cuda.synchronize()
        for t in twins:
            assert t.assert_same(f"call {c}") == c + 1


def test_weighted_batch_group_at_default_weights_is_the_ordinary_command(twins):
    """... and the same through m3_batch_command: the weighted kb_rollout_point against each twin's own ordinary m3_command."""
    twins += [_weights(Twin(i, **s), force_A=1) for i, s in enumerate(IDENTITY)]
    rl, _ = _run(twins, calls=6)
    assert rl == 4          # every forced handle runs the general weighted instance: groups by (K, T) only


# ------------------------------------------------------------------ 6. exact scaling
def _scaled_pair(i, task, goal, factor, avoid=False, **kw):
    """Two handles: A carries `factor` on the outer weights and on the softmin's temperature; B is the default handle."""
    e = []
    for f in (factor, 1.0):
        t = HipEngine(make_config(K=2000, T=30, nu=2, lambda_=0.5 * f, **PK, **kw))
        if not t.cfg.sampling_random:
            t.set_noise(_noise(2000, 30, 100 + i))
        t.set_objective(task, goal)
        if avoid:
            t.set_avoid_dyn_obs(True)
        t.set_beta(f)
        e.append(t)
    e[0].set_point_cost_weights({k: L.COST_WEIGHT_DEFAULTS[k] * factor for k in OUTER})
    return e


INFO_BUT_BETA = ("eta", "eta_1", "eta_2", "iters", "iters_1", "iters_2", "best_idx", "best_idx_1", "best_idx_2", "wsum_push",
                 "wsum_pull", "pull_preference", "calls")


@pytest.mark.parametrize("factor", [2.0, 0.5])
@pytest.mark.parametrize("task,goal,avoid,kw", [
    ("navigation", (2.0, -2.0), False, {}), ("push", (-1.0, -1.0), False, {}), ("pull", (0.0, 0.0), False, {}),
    ("push", (-1.0, -1.0), True, {}),
    ("push", (-1.0, -1.0), False, dict(mode_simple=True, sampling_random=True, u_per_command=10)),
    ("pull", (0.0, 0.0), False, dict(mode_simple=True, sampling_random=True, u_per_command=10))])
def test_outer_weights_and_temperature_times_a_power_of_two(task, goal, avoid, kw, factor):
    """Derived, not measured: a power of two scales every float32 exactly (no cost here is near the ends of the exponent
    range), so the trajectory costs scale exactly; the softmin sees (J - min J) / temperature, the simple mode's
    perturbation cost is lambda * ..., so with the temperature scaled alike the weights, the plan and the top-k keep their
    bits.  Which number the temperature is follows the reference: mppi_mode 'simple' reads lambda_;
    'halton-spline' never reads lambda_ -- its single-mode softmin divides by the persistent beta (m3_set_beta; 1 on a
    fresh point_env planner, never adapted there).  Both are scaled on A, so each mode's own temperature is."""
    A, B = _scaled_pair(3, task, goal, factor, avoid, **kw)
    same = [b for b in BUFS if b not in (L.BUF_TRAJ_COST, L.BUF_COST_HORIZON)]
    try:
        for c in range(6):
            for e in (A, B):
                e.set_world_point_raw(_world(3, c))
                e.command()
            torch.cuda.synchronize()
            for b in (L.BUF_TRAJ_COST, L.BUF_COST_HORIZON):
                a_, b_ = A.buffer(b).cpu().numpy(), B.buffer(b).cpu().numpy()
                assert a_.tobytes() == (b_ * F(factor)).tobytes(), (c, b)
                assert np.isfinite(b_).all() and (b_ != 0).any()
            for b in same:
                try:
                    x, y = A.buffer(b), B.buffer(b)
                except L.M3Error:
                    continue
                assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), f"call {c}: buffer {b} differs"
            ia, ib = A.info(), B.info()
            for f in INFO_BUT_BETA:
                assert getattr(ia, f) == getattr(ib, f), (c, f)
    finally:
        A.close()
        B.close()


def test_inner_weights_times_two_outer_distance_weights_halved(twins):
    """dist_cost doubles exactly, push_dist / pull_dist halve: the push and pull costs keep their bits."""
    w = dict(robot_box=2.0, box_goal=20.0, push_dist=1.5, pull_dist=1.5)
    twins += [_weights(Twin(0, K=2000, T=30, task="push", goal=(-1.0, -1.0)), A=w),
              _weights(Twin(1, K=2000, T=15, task="pull", goal=(0.0, 0.0)), A=w),
              _weights(Twin(2, K=4000, T=30, task="push_pull", goal=(-3.75, -3.75), multi_modal=True), A=w)]
    for c in range(4):
        for t in twins:
            t.set_world(c)
            t.A.command()
            t.B.command()
        torch.cuda.synchronize()
        for t in twins:
            t.assert_same(f"call {c}")


# ------------------------------------------------------------------ 7. against the restatement
def _random_weights(rng):
    v = rng.uniform(-5, 20, 9)
    v[rng.integers(0, 9)] = 0.0
    v[rng.integers(0, 9)] = -abs(v[0]) - 0.5
    return {n: float(F(x)) for n, x in zip(R.NAMES, v)}


@pytest.mark.parametrize("task,mm,avoid", [("navigation", False, False), ("push", False, False), ("pull", False, False),
                                           ("push_pull", True, False), ("pull", True, True), ("push", False, True)])
def test_step_mode_cost_equals_the_restatement(task, mm, avoid):
    from tests.test_cost_weights_cpu import random_cost_worlds
    K = 4096
    rng = np.random.default_rng([7, R.NAMES.index("pull_vel"), len(task)])
    worlds = random_cost_worlds(K, rng)
    goal = tuple(float(x) for x in rng.uniform(-3, 3, 2).astype(F))
    e = HipEngine(make_config(K=K, K_local=K, T=1, nu=2, sim_only=True, filter_u=False))
    try:
        e.set_multi_modal(mm)
        e.set_objective(task, goal)
        e.set_avoid_dyn_obs(avoid)
        kp = float(e.cfg.kp_suction)
        g = dict(robot=worlds[:, 0:2], vel=worlds[:, 2:4], box=worlds[:, 4:6], dynf=worlds[:, 6:8])
        for rep in range(3):
            wt = _random_weights(rng) if rep else dict(L.COST_WEIGHT_DEFAULTS)
            e.set_point_cost_weights(wt)
            sw = e.buffer(L.BUF_SIM_WORLD).view(-1, K)
            sw.zero_()
            for row, col in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (22, 6), (23, 7)):
                sw[row].copy_(torch.from_numpy(worlds[:, col].copy()))
            sw[6] = 1.0
            sw[13] = 1.0
            sw[18:22] = 12345.0
            c = e.cost().cpu().numpy()
            ref = R.cost(task, goal=np.array(goal, F), w=R.weights(**wt), multi_modal=mm, half_K=K // 2, avoid_dyn_obs=avoid, **g)
            assert c.tobytes() == ref.tobytes(), (rep, np.abs(c - ref).max())
            pend = e.buffer(L.BUF_SIM_WORLD).view(-1, K)[18:22].cpu().numpy().T
            pr = R.pending(task, g["robot"], g["vel"], g["box"], kp, 1.8, multi_modal=mm, half_K=K // 2)
            if pr is None:
                assert (pend == F(12345.0)).all()
            else:
                assert np.ascontiguousarray(pend).tobytes() == pr.tobytes()      # weights do not touch the suction
    finally:
        e.close()


@pytest.mark.parametrize("task,goal,mm", [("push", (-1.0, -1.0), False), ("pull", (0.5, 0.5), False),
                                          ("push_pull", (-3.75, -3.75), True), ("navigation", (-2.0, 2.0), False)])
def test_fused_rollout_costs_equal_step_and_cost_replayed(task, goal, mm):
    """The relation the planner's probe relies on, with weights on both sides: per-step costs, bit for bit."""
    from m3p2i_aip_amd import scenes
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    K, T = 512, 20
    sim = IsaacGymWrapper(IsaacGymConfig(dt=0.05), "point_env", num_envs=K)
    e = HipEngine(make_config(K=K, T=T, nu=2, multi_modal=mm, kp_suction=float(sim._engine.cfg.kp_suction), **PK))
    try:
        sim._dof_state[:, 0] = 0.4
        sim._dof_state[:, 2] = 1.2
        sim.set_dof_state_tensor(sim._dof_state)
        wt = dict(W_B, pull_vel=5.0)
        e.set_noise(_noise(K, T, 9))
        e.set_objective(task, goal)
        e.set_point_cost_weights(wt)
        e.bind_sim_point(sim._dof_state, sim._root_state, scenes.actor_index("point_env", "box"),
                         scenes.actor_index("point_env", "dyn-obs"))
        e.rollout()
        torch.cuda.synchronize()
        A = e.buffer(L.BUF_ACTIONS).clone()
        Cf = e.buffer(L.BUF_COST_HORIZON).cpu().numpy()
        s = sim._engine
        s.set_multi_modal(mm)
        s.set_objective(task, goal)
        s.set_point_cost_weights(wt)
        for t in range(T):
            u = A[t].contiguous()
            s._ck(s.lib.m3_sim_step_with_target(s._h, u.data_ptr()))
            c = s.cost().cpu().numpy()
            assert c.tobytes() == Cf[t].tobytes(), (t, np.abs(c - Cf[t]).max())
        assert len(np.unique(Cf[-1])) > K // 4
    finally:
        e.close()
        sim.stop_sim()


# ------------------------------------------------------------------ 8. the planner keeps the fused path
def _side(overrides):
    from m3p2i_aip_amd import compat
    from m3p2i_aip_amd.episodes import _PlannerSide
    compat.install(force_standins=True)
    return _PlannerSide(compat.make_config("config_point", overrides))


def test_planner_with_cost_weights_keeps_the_fused_path():
    """On the parent this planner can only be written with a torch cost, whose probe says False."""
    base = ["task=push", "goal=[-1.0, -1.0]", "mppi.num_samples=2000", "mppi.horizon=30"]
    sides = [_side(base + ["cost_weights={push_align: 2.5, box_goal: 4.0}"]), _side(base),
             _side(base + ["cost_weights={push_align: 2.5, box_goal: 4.0}", "mppi.fused=false"])]
    try:
        outs = []
        for s in sides:
            real_dof, real_root = s.sim._dof_state[0:1].clone(), s.sim._root_state[0:1].clone()
            outs.append(s.first_plan(real_dof, real_root).clone())
        torch.cuda.synchronize()
        weighted, default, step = sides
        assert weighted.motion_planner.probe_result["fused"] is True
        assert default.motion_planner.probe_result["fused"] is True
        assert step.motion_planner._fused is False
        assert weighted.motion_planner._engine.point_cost_weights()["push_align"] == 2.5
        assert weighted.sim._engine.point_cost_weights()["box_goal"] == 4.0
        assert default.motion_planner._engine.point_cost_weights() == L.COST_WEIGHT_DEFAULTS
        assert not torch.equal(outs[0][0], outs[1][0])                     # the weights are live
        # (the probe returns its step leg's plan; the fused leg's costs agreed with it to the probe's tolerance)
        assert torch.allclose(outs[0], outs[2], rtol=1e-5, atol=1e-4)
        nxt = weighted.motion_planner.command(weighted.sim._dof_state[0])  # a fused command afterwards
        assert weighted.motion_planner._fused is True and torch.isfinite(nxt).all()
    finally:
        for s in sides:
            s.close()


def test_non_default_weights_need_an_engine_that_takes_them():
    from m3p2i_aip_amd.cost_functions import Objective
    o = _side(["task=push", "goal=[-1.0, -1.0]", "cost_weights={push_align: 2.5}"])
    try:
        class Bare:
            pass
        with pytest.raises(TypeError, match="set_point_cost_weights"):
            o.objective.push_cost_weights(Bare())
        assert isinstance(o.objective, Objective)
    finally:
        o.close()


# ------------------------------------------------------------------ 9. batch and episodes
def test_batch_of_weighted_and_unweighted_handles(twins):
    ws = [dict(push_align=2.5), dict(push_align=0.0, box_goal=3.0), dict(collision=10.0, push_dist=-1.0), W_B]
    twins += [_weights(Twin(i, K=2000, T=30, task="push", goal=(-1.0, -1.0)), A=w, B=w) for i, w in enumerate(ws)]
    twins += [Twin(4 + i, K=2000, T=30, task="push", goal=(-1.0, -1.0)) for i in range(4)]
    order = {1: [7, 0, 6, 1, 5, 2, 4, 3], 2: [0, 4, 1]}
    launches = _run(twins, calls=4, order=lambda c: order.get(c, list(range(8))))
    assert launches == (2, 1)         # two rollout groups (weighted / per-task push), one update group
    costs = [t.A.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes() for t in twins[:4]]
    assert len(set(costs)) == 4       # different weights in one launch, each handle with its own


def _same_report(a, b):
    from tests.test_episodes_gpu import _same
    _same(a, b)


def test_weighted_episodes_equal_the_serial_loop():
    import band_stats as bs
    import closed_loop
    from m3p2i_aip_amd.episodes import run_point_episodes
    ws = ["cost_weights={push_align: 2.5}", "cost_weights={push_align: 0.0, box_goal: 6.0}",
          "cost_weights={push_dist: 2.0, robot_box: 2.0}", "cost_weights={push_align: 4.0, collision: 10.0}"]
    sc = "case2_halton_push_coll"
    eps = [("config_point", bs.overrides(sc, "default") + [w], bs.jitter_of(sc, 1 + i)) for i, w in enumerate(ws)]
    reps = run_point_episodes(eps, max_ticks=120, trace=True)
    for (cn, ov, j), r in zip(eps, reps):
        _same_report(r, closed_loop.run(cn, ov, ticks=120, jitter=j, trace=True))
    plain = run_point_episodes([("config_point", bs.overrides(sc, "default"), bs.jitter_of(sc, 1))], max_ticks=120, trace=True)[0]
    assert plain["trace"] != reps[0]["trace"]


# ------------------------------------------------------------------ 10. sharded
def test_two_shards_equal_the_unsharded_weighted_handle():
    from tests.sharded_update_driver import Case, HipBackend, smooth_noise
    case = Case("weighted", 0, "single", (1024, 1024), None, T=20)
    be = HipBackend()
    shards = [be.engine(case, r) for r in range(2)]
    whole = HipEngine(make_config(K=case.K, T=case.T, nu=2, lambda_=1.0, **PK))
    delta = smooth_noise(case.K, case.T, 2, 4)
    world = _world(1, 2)
    try:
        for e, lo, hi in [(shards[0], 0, 1024), (shards[1], 1024, 2048), (whole, 0, 2048)]:
            e.set_noise(delta[lo:hi])
            e.set_objective("push", (-1.0, -1.0))
            e.set_world_point_raw(world)
            e.set_point_cost_weights(W_B)
            e.rollout()
        torch.cuda.synchronize()
        for b in (L.BUF_TRAJ_COST, L.BUF_COST_HORIZON):
            cat = torch.cat([s.buffer(b) for s in shards], dim=-1).cpu().numpy()
            assert cat.tobytes() == whole.buffer(b).cpu().numpy().tobytes(), b
        plain = HipEngine(make_config(K=case.K, T=case.T, nu=2, lambda_=1.0, **PK))
        plain.set_noise(delta)
        plain.set_objective("push", (-1.0, -1.0))
        plain.set_world_point_raw(world)
        plain.rollout()
        torch.cuda.synchronize()
        assert not torch.equal(plain.buffer(L.BUF_TRAJ_COST), whole.buffer(L.BUF_TRAJ_COST))
        plain.close()
    finally:
        for e in shards + [whole]:
            e.close()


# ------------------------------------------------------------------ 11. refusals
def test_refusals():
    lib = L.load()
    e = HipEngine(make_config(K=2000, T=30, nu=2, **PK))
    panda = HipEngine(make_config(K=200, T=20, nu=9, env_type="panda_env", u_min=[-1.2] * 9, u_max=[1.2] * 9,
                                  noise_sigma_diag=[10.0] * 7 + [0.8, 0.8], lambda_=0.05, dt=0.01))
    sim = HipEngine(make_config(K=64, K_local=64, T=1, nu=2, sim_only=True, filter_u=False))
    batch = HipBatch(2)
    try:
        with pytest.raises(L.M3Error, match="point_env only"):
            panda.set_point_cost_weights(W_A)
        with pytest.raises(L.M3Error, match="point_env only"):
            panda.set_weighted_cost_instance(1)
        for name, bad in (("pull_vel", float("nan")), ("collision", float("inf")), ("nav_dist", -float("inf"))):
            with pytest.raises(L.M3Error, match=f"m3_set_point_cost_weights: {name} is not finite"):
                e.set_point_cost_weights({name: bad})
            assert e.point_cost_weights() == L.COST_WEIGHT_DEFAULTS          # a refused call changes nothing
        with pytest.raises(ValueError, match="unknown cost weight"):
            e.set_point_cost_weights({"push_alignment": 1.0})
        with pytest.raises(L.M3Error, match="-1"):
            e.set_weighted_cost_instance(2)
        # forced off with non-default weights: refused at the next command / rollout / batched command / cost call
        e.set_noise(_noise(2000, 30, 1))
        e.set_objective("push", (-1.0, -1.0))
        e.set_world_point_raw(_world(0, 0))
        e.command()
        torch.cuda.synchronize()
        before = (e.info().calls, e.buffer(L.BUF_MEAN).cpu().numpy().tobytes())
        e.set_point_cost_weights(W_A)
        e.set_weighted_cost_instance(0)
        for call in (e.command, e.rollout):
            with pytest.raises(L.M3Error, match="forced off"):
                call()
        arr = (C.c_void_p * 1)(e._h.value)
        assert lib.m3_batch_command(batch._b, arr, 1, None) == L_ERR["STATE"]
        assert "forced off" in lib.m3_batch_last_error(batch._b).decode()
        torch.cuda.synchronize()
        assert (e.info().calls, e.buffer(L.BUF_MEAN).cpu().numpy().tobytes()) == before
        e.set_weighted_cost_instance(-1)
        e.command()
        sim.buffer(L.BUF_SIM_WORLD)
        sim.set_objective("push", (-1.0, -1.0))
        sim.set_point_cost_weights(W_A)
        sim.set_weighted_cost_instance(0)
        with pytest.raises(L.M3Error, match="m3_cost: .*forced off"):
            sim.cost()
        sim.set_point_cost_weights(None)
        sim.cost()                              # default weights, forced off: the ordinary kernel
    finally:
        batch.close()
        for h in (e, panda, sim):
            h.close()
