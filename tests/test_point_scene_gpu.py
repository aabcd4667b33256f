"""The run-time point_env arena (m3_set_point_scene) on the GPU: the fused rollout, the command, the batched command and the
step mode of a handle with a custom arena against the CPU oracle with the same arena, bit for bit where the default arena is
held bit for bit (tests/test_hip_parity_point.py), and the run-time-scene build at the default values against the ordinary
kernels, byte for byte.  Inputs: tests/point_scene_fixture.py.  Every scene case first asserts, on the oracle alone, that
the custom arena changes at least a quarter of the samples.

The no-allocation check is tests/test_point_scene_no_alloc_gpu.py.

Run on an MI355X so far: everything but the section "episodes and shards" (three cases) and the no-allocation file."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, make_config  # noqa: E402
from tests import point_scene_fixture as X  # noqa: E402
from tests.test_batch_command_gpu import PK, Twin, _noise  # noqa: E402
from tests.test_hip_parity_point import raw_world  # noqa: E402

F = np.float32
TASKS = [("navigation", False), ("push", False), ("pull", False), ("push_pull", True)]
W_TUNED = dict(push_align=2.5, robot_box=2.0, nav_dist=0.5, pull_vel=1.0)


def _pair(oracle, task, mm, K, scene, T=X.T):
    """(HIP engine, oracle planner): the same config, noise table, objective; `scene`: field overrides or None"""
    delta = X.actions(K, T)
    ocfg = oracle.make_cfg(K, T, 2, task=task, goal=X.GOAL, multi_modal=mm, filter_u=False)
    opl = oracle.OraclePointPlanner(ocfg, delta, scene=X.oracle_scene(oracle, scene))
    eng = HipEngine(make_config(K=K, T=T, nu=2, multi_modal=mm, filter_u=False, **PK))
    eng.set_objective(task, X.GOAL)
    eng.set_noise(delta)
    if scene:
        eng.set_point_scene(scene)
    return eng, opl


def _assert_rollout_bits(eng, opl, label):
    st, ac = eng.states.cpu().numpy(), eng.actions.cpu().numpy()
    np.testing.assert_array_equal(ac.view(np.uint32), opl.last["actions"].view(np.uint32), err_msg=label)
    bad = np.argwhere(st.view(np.uint32) != opl.last["states"].view(np.uint32))
    assert bad.size == 0, f"{label}: first state mismatch at (k,t,c)={bad[0]} of {len(bad)}"
    np.testing.assert_array_equal(eng.cost_horizon.cpu().numpy().view(np.uint32), opl.last["cost_h"].view(np.uint32), err_msg=label)
    np.testing.assert_array_equal(eng.buffer(L.BUF_TRAJ_COST).cpu().numpy().view(np.uint32), opl.last["J"].view(np.uint32),
                                  err_msg=label)


def _changed_share(oracle, task, mm, K, w0):
    """on the oracle alone: the share of the samples whose robot states differ between the custom and the default arena"""
    out = []
    for scene in (X.CUSTOM, None):
        delta = X.actions(K, X.T)
        opl = oracle.OraclePointPlanner(oracle.make_cfg(K, X.T, 2, task=task, goal=X.GOAL, multi_modal=mm, filter_u=False), delta,
                                        scene=X.oracle_scene(oracle, scene))
        opl.command(w0)
        assert np.isfinite(opl.last["cost_h"]).all()
        out.append(opl.last["states"].copy())
    return float((out[0].view(np.uint32) != out[1].view(np.uint32)).reshape(K, -1).any(1).mean())


# ------------------------------------------------------------------ fused rollout vs the oracle
@pytest.mark.parametrize("K", [64, 100])
@pytest.mark.parametrize("task,mm", TASKS)
def test_rollout_in_the_custom_arena_equals_the_oracle(oracle, task, mm, K):
    worlds = X.start_worlds(oracle)
    eng, _ = _pair(oracle, task, mm, K, X.CUSTOM)
    try:
        for wi, w0 in enumerate(worlds):
            share = _changed_share(oracle, task, mm, K, w0)
            print(f"{task} K={K} world {X.WORLD_NAMES[wi]}: {share:.3f} of the samples differ between the arenas")
            assert share >= 0.25, (task, wi, share)
            opl = oracle.OraclePointPlanner(oracle.make_cfg(K, X.T, 2, task=task, goal=X.GOAL, multi_modal=mm, filter_u=False),
                                            X.actions(K, X.T), scene=X.oracle_scene(oracle, X.CUSTOM))
            eng.reset()
            eng.set_world_point_raw(raw_world(w0))
            eng.command(sync_host=True)
            opl.command(w0)
            _assert_rollout_bits(eng, opl, f"{task} K={K} world {X.WORLD_NAMES[wi]}")
    finally:
        eng.close()


# the smallest workgroup counts the launchers' rule (rollout_two_waves / rollout_three_waves, m3_internal.hpp: more than
# M3_SIMDS = 1024 wavefronts, more than 4 * M3_SIMDS) maps to the _occ2 and _occ3 builds; one sample per wavefront
# (m3_set_rollout_lanes 1) gets there at K = 1025 and K = 4097
@pytest.mark.parametrize("K,build", [(1025, "occ2"), (4097, "occ3")])
def test_rollout_through_the_two_and_three_wave_builds(oracle, K, build):
    w0 = X.start_worlds(oracle)[2]
    assert _changed_share(oracle, "push", False, K, w0) >= 0.25
    eng, opl = _pair(oracle, "push", False, K, X.CUSTOM)
    try:
        eng.set_rollout_lanes(1)
        eng.set_world_point_raw(raw_world(w0))
        eng.command(sync_host=True)
        opl.command(w0)
        _assert_rollout_bits(eng, opl, f"{build} K={K}")
    finally:
        eng.close()


def test_custom_arena_with_tuned_cost_weights_differs_from_the_default_weights_only_in_the_costs(oracle):
    """the scene build is the weighted build: tuned weights on top of the custom arena leave the first command's states and
    actions (which do not depend on the cost) at the oracle's bits and change the costs"""
    w0 = X.start_worlds(oracle)[2]
    assert _changed_share(oracle, "push", False, 64, w0) >= 0.25
    eng, opl = _pair(oracle, "push", False, 64, X.CUSTOM)
    try:
        eng.set_point_cost_weights(W_TUNED)
        eng.set_world_point_raw(raw_world(w0))
        eng.command(sync_host=True)
        opl.command(w0)
        np.testing.assert_array_equal(eng.states.cpu().numpy().view(np.uint32), opl.last["states"].view(np.uint32))
        np.testing.assert_array_equal(eng.actions.cpu().numpy().view(np.uint32), opl.last["actions"].view(np.uint32))
        tuned = eng.cost_horizon.cpu().numpy().copy()
        assert (tuned != opl.last["cost_h"]).mean() > 0.9
        # ... and equal the costs of the weighted default-arena kernel wherever the arena did not change the sample's states
        ref = HipEngine(make_config(K=64, T=X.T, nu=2, filter_u=False, **PK))
        ref.set_objective("push", X.GOAL); ref.set_noise(X.actions(64, X.T)); ref.set_point_cost_weights(W_TUNED)
        ref.set_world_point_raw(raw_world(w0))
        ref.command(sync_host=True)
        same = (ref.states.cpu().numpy().view(np.uint32) == eng.states.cpu().numpy().view(np.uint32)).all(axis=(1, 2))
        ref_cost = ref.cost_horizon.cpu().numpy()
        ref_traj = ref.buffer(L.BUF_TRAJ_COST).cpu().numpy().copy()
        ref.close()
        # (the oracle has no cost weights; the independent reference of the tuned costs is the parent's weighted kernel, which
        # tests/test_cost_weights_* hold to the numpy restatement -- on the samples that never meet what the arena changed)
        assert same.sum() >= 4, same.sum()
        np.testing.assert_array_equal(tuned[same].view(np.uint32), ref_cost[same].view(np.uint32))
        np.testing.assert_array_equal(eng.buffer(L.BUF_TRAJ_COST).cpu().numpy()[same].view(np.uint32), ref_traj[same].view(np.uint32))
    finally:
        eng.close()


# ------------------------------------------------------------------ the forced instance at the default values
@pytest.mark.parametrize("spec", [dict(K=200, T=15, task="navigation", goal=(2.0, -2.0)),
                                  dict(K=2000, T=30, task="push", goal=(-1.0, -1.0)),
                                  dict(K=2000, T=15, task="pull", goal=(0.0, 0.0)),
                                  dict(K=4000, T=30, task="push_pull", goal=(-3.75, -3.75), multi_modal=True)],
                         ids=["navigation", "push", "pull", "push_pull"])
def test_forced_scene_instance_at_default_values_is_the_ordinary_command(spec):
    t = Twin(0, **spec)
    try:
        t.A.set_point_scene_instance(1)
        for c in range(3):
            t.set_world(c)
            t.A.command()
            t.B.command()
            torch.cuda.synchronize()
            assert t.assert_same(f"call {c}") == c + 1
    finally:
        t.close()


# ------------------------------------------------------------------ commands vs the oracle planner
@pytest.mark.parametrize("task,mm", [("push", False), ("push_pull", True)])
def test_three_commands_in_the_custom_arena_vs_the_oracle_planner(oracle, task, mm):
    """What tests/test_hip_parity_point.py asks of the default arena, with its figures (that file has no helper or constant to
    import besides raw_world; conftest.assert_close_but_few is the helper it uses): test_command_traces_vs_reference_and_oracle
    -- control output vs the oracle atol 1e-3 on every command, the first command's rollout bit for bit, weights rtol 2e-3 atol
    1e-6 with frac 0 on the first command and 0.01, cap 1e-3 afterwards (a rollout or two may take another contact history once
    the plans differ in the last bits); test_rollout_bit_exact_with_contacts -- mean atol 1e-4, on the first command."""
    from tests.conftest import assert_close_but_few
    K, T = 256, 12
    delta = X.actions(K, T)
    ocfg = oracle.make_cfg(K, T, 2, task=task, goal=X.GOAL, multi_modal=mm)
    opl = oracle.OraclePointPlanner(ocfg, delta, scene=X.oracle_scene(oracle, X.CUSTOM))
    eng = HipEngine(make_config(K=K, T=T, nu=2, multi_modal=mm, **PK))
    try:
        eng.set_objective(task, X.GOAL); eng.set_noise(delta); eng.set_point_scene(X.CUSTOM)
        w0 = X.start_worlds(oracle)[2].copy()
        for call in range(3):
            w0[0] += 0.02 * call
            eng.set_world_point_raw(raw_world(w0))
            a_hip = eng.command(sync_host=True)
            a_orc = opl.command(w0)
            np.testing.assert_allclose(a_hip[:a_orc.shape[0]], a_orc, atol=1e-3, err_msg=f"call {call}")
            assert_close_but_few(eng.buffer(L.BUF_WEIGHTS).cpu().numpy(), opl.last["w"], rtol=2e-3, atol=1e-6,
                                 frac=0.0 if call == 0 else 0.01, cap=1e-3, err_msg=f"call {call} weights")
            if call == 0:
                _assert_rollout_bits(eng, opl, "first command")
                if not mm:
                    np.testing.assert_allclose(eng.buffer(L.BUF_MEAN).cpu().numpy(), opl.mean, atol=1e-4)
    finally:
        eng.close()


# ------------------------------------------------------------------ batched command
def test_batch_of_default_and_two_custom_arenas():
    """six handles in one m3_batch_command -- two default, two arena A, two arena B: each bit-identical to its own m3_command;
    the default handles and the scene handles are separate rollout launches, A and B share one"""
    twins = [Twin(i, K=256, T=12, task="push", goal=X.GOAL) for i in range(6)]
    batch = HipBatch(6)
    try:
        for i, t in enumerate(twins):
            sc = (None, X.CUSTOM, X.CUSTOM_B)[i // 2]
            if sc:
                t.A.set_point_scene(sc); t.B.set_point_scene(sc)
        for c in range(3):
            for t in twins:
                t.set_world(c)
            batch.command([t.A for t in twins])
            for t in twins:
                t.B.command()
            torch.cuda.synchronize()
            for t in twins:
                assert t.assert_same(f"call {c}") == c + 1
            assert batch.launches()[0] == 2
        # the arenas really differ: the A and B handles do not compute what the default handles compute
        s = [t.A.states.cpu().numpy() for t in twins]
        assert (s[0] != s[2]).any() or (s[0] != s[4]).any()
    finally:
        batch.close()
        for t in twins:
            t.close()


# ------------------------------------------------------------------ step mode
def test_step_mode_in_the_custom_arena_equals_the_oracle(oracle):
    from m3p2i_aip_amd import isaacgym_wrapper as wrapper
    n = 64
    worlds = np.repeat(X.start_worlds(oracle), [22, 21, 21], axis=0).astype(F)
    ref_default = worlds.copy()
    sim = wrapper.IsaacGymWrapper(wrapper.IsaacGymConfig(dt=0.05, point_scene=dict(X.CUSTOM)), "point_env", num_envs=n)
    try:
        assert sim._engine.point_scene()["wall"] == float(F(1.5))
        obs_row = [a.name for a in sim.env_cfg].index("obs")
        assert sim._root_state[0, obs_row, 0:2].cpu().tolist() == [-1.0, 0.5]
        from tests.test_batch_command_gpu import BOX_ACTOR, DYN_ACTOR
        sim._dof_state[:, 0] = torch.tensor(worlds[:, 0]); sim._dof_state[:, 2] = torch.tensor(worlds[:, 1])
        sim._dof_state[:, 1] = 0.0; sim._dof_state[:, 3] = 0.0
        for actor, o in ((BOX_ACTOR, oracle.W_B), (DYN_ACTOR, oracle.W_D)):
            sim._root_state[:, actor, 0:2] = torch.tensor(worlds[:, o:o + 2])
            sim._root_state[:, actor, 3:7] = torch.tensor([0.0, 0.0, 0.0, 1.0])
            sim._root_state[:, actor, 7:13] = 0.0
        sim.set_dof_state_tensor(sim._dof_state)
        sim.set_actor_root_state_tensor(sim._root_state)
        rng = np.random.default_rng(1)
        sc, sc0 = X.oracle_scene(oracle, X.CUSTOM), X.oracle_scene(oracle)
        e = sim._engine
        for t in range(8):
            u = rng.uniform(-3, 3, (n, 2)).astype(F)
            oracle.step_batch(sc, worlds, u)
            oracle.step_batch(sc0, ref_default, u)
            ud = torch.tensor(u, device="cuda:0")
            e._ck(e.lib.m3_sim_step_with_target(e._h, ud.data_ptr()))
            torch.cuda.synchronize()
            dof = sim._dof_state.cpu().numpy()
            got = np.stack([dof[:, 0], dof[:, 2], dof[:, 1], dof[:, 3]], 1)
            np.testing.assert_array_equal(got.view(np.uint32), worlds[:, [0, 1, 4, 5]].view(np.uint32), err_msg=f"step {t} robot")
            root = sim._root_state.cpu().numpy()
            for actor, o in ((BOX_ACTOR, oracle.W_B), (DYN_ACTOR, oracle.W_D)):
                np.testing.assert_array_equal(root[:, actor, 0:2].view(np.uint32), worlds[:, o:o + 2].view(np.uint32),
                                              err_msg=f"step {t} actor {actor} position")
                np.testing.assert_array_equal(root[:, actor, 7:9].view(np.uint32), worlds[:, o + 4:o + 6].view(np.uint32),
                                              err_msg=f"step {t} actor {actor} velocity")
                np.testing.assert_array_equal(root[:, actor, 12].view(np.uint32), worlds[:, o + 6].view(np.uint32))
        differs = (worlds[:, [0, 1, 4, 5]] != ref_default[:, [0, 1, 4, 5]]).any(1)
        assert differs.mean() >= 0.25, differs.mean()
    finally:
        sim.close() if hasattr(sim, "close") else None


# ------------------------------------------------------------------ episodes and shards
ARENA_EP = "point_scene={obs_x: 0.0, obs_y: 0.9, obs_hx: 0.3, obs_hy: 0.1, wall: 2.95, mu_rb: 0.4}"   # the obstacle between robot and box


def test_episodes_in_a_custom_arena_equal_the_serial_loop():
    """run_point_episodes with n = 4 (the arena on the world handle and, through planner._bind_world, on the four planners'
    handles: kb_rollout_point on PointSceneRT + k_episodes_post_s) against the serial closed_loop.run loop, report and trace bit for bit"""
    import band_stats as bs
    import closed_loop
    from m3p2i_aip_amd.episodes import run_point_episodes
    from tests.test_episodes_gpu import _same
    sc = "case2_halton_push_coll"
    small = ["mppi.num_samples=128", "mppi.horizon=12", "mppi.u_per_command=12"]
    eps = [("config_point", bs.overrides(sc, "default") + small + [ARENA_EP], bs.jitter_of(sc, 1 + i)) for i in range(4)]
    reps = run_point_episodes(eps, max_ticks=16, trace=True)
    for (cn, ov, j), r in zip(eps, reps):
        _same(r, closed_loop.run(cn, ov, ticks=16, jitter=j, trace=True))
    plain = run_point_episodes([("config_point", bs.overrides(sc, "default") + small, bs.jitter_of(sc, 1))], max_ticks=16, trace=True)[0]
    assert plain["trace"] != reps[0]["trace"]          # the arena is live: the robot meets the obstacle on its way to the box


def test_planner_takes_the_arena_of_its_wrapper_unless_told_not_to():
    from tests.test_cost_weights_gpu import _side
    t = _side(["task=push", "goal=[-1.0, -1.0]", "mppi.num_samples=128", ARENA_EP])
    try:
        p = t.motion_planner
        real_dof, real_root = t.sim._dof_state[0:1].clone(), t.sim._root_state[0:1].clone()
        t.first_plan(real_dof, real_root)
        assert p._engine.point_scene()["obs_y"] == float(F(0.9)) and t.sim._engine.point_scene()["wall"] == float(F(2.95))
        assert p.probe_result["fused"] is True     # the step-mode leg and the fused leg of the probe agree in the custom arena
        p.follow_sim_scene = False                 # an arena set by hand on the planner's engine now stays
        p._engine.set_point_scene(wall=3.5)
        nxt = p.command(t.sim._dof_state[0])
        assert torch.isfinite(nxt).all()
        assert p._engine.point_scene()["wall"] == 3.5 and p._engine.point_scene()["obs_y"] == 2.0
    finally:
        t.close()


def test_two_shards_equal_the_unsharded_handle_in_the_custom_arena(oracle):
    """as tests/test_cost_weights_gpu.py::test_two_shards_equal_the_unsharded_weighted_handle, same bound (bytes): the shards'
    rollouts side by side are the unsharded handle's"""
    from tests.sharded_update_driver import Case, HipBackend, smooth_noise
    case = Case("scene", 0, "single", (1024, 1024), None, T=20)
    be = HipBackend()
    shards = [be.engine(case, r) for r in range(2)]
    whole = HipEngine(make_config(K=case.K, T=case.T, nu=2, lambda_=1.0, **PK))
    plain = HipEngine(make_config(K=case.K, T=case.T, nu=2, lambda_=1.0, **PK))
    delta = smooth_noise(case.K, case.T, 2, 4)
    world = raw_world(X.start_worlds(oracle)[2])
    try:
        for e, lo, hi in [(shards[0], 0, 1024), (shards[1], 1024, 2048), (whole, 0, 2048), (plain, 0, 2048)]:
            e.set_noise(delta[lo:hi])
            e.set_objective("push", X.GOAL)
            e.set_world_point_raw(world)
            if e is not plain:
                e.set_point_scene(X.CUSTOM)
            e.rollout()
        torch.cuda.synchronize()
        for b in (L.BUF_TRAJ_COST, L.BUF_COST_HORIZON):
            cat = torch.cat([s.buffer(b) for s in shards], dim=-1).cpu().numpy()
            assert cat.tobytes() == whole.buffer(b).cpu().numpy().tobytes(), b
        cat = torch.cat([s.buffer(L.BUF_STATES) for s in shards], dim=1).cpu().numpy()
        assert cat.tobytes() == whole.buffer(L.BUF_STATES).cpu().numpy().tobytes()
        differs = (plain.buffer(L.BUF_STATES) != whole.buffer(L.BUF_STATES)).any(dim=0).any(dim=-1).float().mean().item()
        assert differs >= 0.25, differs
    finally:
        for e in shards + [whole, plain]:
            e.close()


# ------------------------------------------------------------------ refusals and round trip
def test_round_trip_and_refusals():
    lib = L.load()
    e = HipEngine(make_config(K=64, T=12, nu=2, **PK))
    try:
        assert e.point_scene() == {k: float(F(v)) for k, v in L.POINT_SCENE_DEFAULTS.items()}
        e.set_point_scene(X.CUSTOM)
        assert e.point_scene() == {k: float(F(v)) for k, v in X.scene_dict(X.CUSTOM).items()}
        e.reset()
        assert e.point_scene()["wall"] == 1.5                    # survives m3_reset
        e.set_point_scene(wall=2.0)                              # (missing keys: the defaults, not the last values)
        assert e.point_scene() == {k: float(F(v)) for k, v in X.scene_dict(dict(wall=2.0)).items()}
        e.set_point_scene(None)
        assert e.point_scene() == {k: float(F(v)) for k, v in L.POINT_SCENE_DEFAULTS.items()}
        for bad, field in ((dict(obs_x=float("nan")), "obs_x"), (dict(box_m=0.0), "box_m"), (dict(mu_rb=-0.1), "mu_rb"),
                           (dict(wall=0.2), "wall"), (dict(dyn_I=float("inf")), "dyn_I")):
            with pytest.raises(L.M3Error, match=field):
                e.set_point_scene(bad)
        assert e.point_scene() == {k: float(F(v)) for k, v in L.POINT_SCENE_DEFAULTS.items()}    # a refused call changes nothing
        # switch 0 with a custom arena: the next command is refused, the handle stays usable
        e.set_objective("push", X.GOAL); e.set_noise(_noise(64, 12, 3))
        e.set_point_scene(X.CUSTOM); e.set_point_scene_instance(0)
        with pytest.raises(L.M3Error, match="forced off"):
            e.command()
        e.set_point_scene_instance(-1)
        e.command(sync_host=True)
        with pytest.raises(L.M3Error):
            e.set_point_scene_instance(2)
    finally:
        e.close()
    p = HipEngine(make_config(K=64, T=12, nu=9, env_type="panda_env", u_min=[-2] * 9, u_max=[2] * 9, noise_sigma_diag=[1] * 9))
    try:
        sc = L.PointSceneFields()
        assert lib.m3_set_point_scene(p._h, None) == -5 and lib.m3_get_point_scene(p._h, C.byref(sc)) == -5
        assert lib.m3_set_point_scene_instance(p._h, 1) == -5
    finally:
        p.close()
