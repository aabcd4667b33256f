"""One arena per SAMPLE of the fused point_env rollout (m3_set_point_rollout_scenes) on the GPU: the rollout and the command of a
planner handle whose rows cycle default / CUSTOM / CUSTOM_B against the CPU oracle rolling each sample out in its own arena
(tests/rollout_scenes_fixture.py), bit for bit where the single custom arena is held bit for bit (tests/test_point_scene_gpu.py);
uniform rows against the single-scene kernels, byte for byte; life cycle, refusals, shards, and the planner whose fused path
is the step path on a wrapper with an arena per environment.  Every rollout case first asserts, on the oracle alone, that the
samples feel their own row: at least 0.8 of them differ from what the next and the previous row's arena give, 0.5 from the
default arena.

Run on an MI355X so far: sections 1 and 2 (the rollout of the four tasks at K = 64 and K = 100, the two- and three-wave builds);
sections 3 to 10 have not been run on a GPU."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, make_config  # noqa: E402
from tests import point_scene_fixture as X  # noqa: E402
from tests import rollout_scenes_fixture as R  # noqa: E402
from tests.test_batch_command_gpu import PK, Twin, _noise  # noqa: E402
from tests.test_hip_parity_point import raw_world  # noqa: E402
from tests.test_point_scene_gpu import TASKS, W_TUNED, _assert_rollout_bits  # noqa: E402

F = np.float32


def _pair(oracle, task, mm, K, rows, T=X.T, **kw):
    """(HIP engine with the rows set, stitched oracle planner): the same config, noise table, objective"""
    kw = kw or dict(filter_u=False)
    delta = X.actions(K, T)
    opl = R.make_stitched(oracle, oracle.make_cfg(K, T, 2, task=task, goal=X.GOAL, multi_modal=mm, **kw), delta, rows)
    eng = HipEngine(make_config(K=K, T=T, nu=2, multi_modal=mm, **kw, **PK))
    eng.set_objective(task, X.GOAL)
    eng.set_noise(delta)
    eng.set_point_rollout_scenes(rows)
    return eng, opl


# ------------------------------------------------------------------ 1: fused rollout vs the stitched oracle
@pytest.mark.parametrize("K", [64, 100])
@pytest.mark.parametrize("task,mm", TASKS)
def test_rollout_with_an_arena_per_sample_equals_the_oracle(oracle, task, mm, K):
    rows = R.cycle_rows(K)
    eng, _ = _pair(oracle, task, mm, K, rows)
    try:
        assert eng.point_rollout_scenes_set()
        for wi, w0 in enumerate(X.start_worlds(oracle)):
            label = f"{task} K={K} world {X.WORLD_NAMES[wi]}"
            R.assert_rows_matter(oracle, task, mm, K, w0, label)
            opl = R.make_stitched(oracle, oracle.make_cfg(K, X.T, 2, task=task, goal=X.GOAL, multi_modal=mm, filter_u=False),
                                  X.actions(K, X.T), rows)
            eng.reset()
            eng.set_world_point_raw(raw_world(w0))
            eng.command(sync_host=True)
            opl.command(w0)
            _assert_rollout_bits(eng, opl, label)
    finally:
        eng.close()


# ------------------------------------------------------------------ 2: the two- and three-wave builds
# (the smallest sizes the launch rule sends to the occ2 / occ3 builds with one sample per wavefront: tests/test_point_scene_gpu.py)
@pytest.mark.parametrize("K,build", [(1025, "occ2"), (4097, "occ3")])
def test_rollout_through_the_two_and_three_wave_builds(oracle, K, build):
    w0 = X.start_worlds(oracle)[2]
    R.assert_rows_matter(oracle, "push", False, K, w0, f"{build} K={K}")
    eng, opl = _pair(oracle, "push", False, K, R.cycle_rows(K))
    try:
        eng.set_rollout_lanes(1)
        eng.set_world_point_raw(raw_world(w0))
        eng.command(sync_host=True)
        opl.command(w0)
        _assert_rollout_bits(eng, opl, f"{build} K={K}")
    finally:
        eng.close()


# ------------------------------------------------------------------ 3: GPU against GPU
@pytest.mark.parametrize("task,mm", TASKS)
@pytest.mark.parametrize("arena", ["custom", "default"])
def test_uniform_rows_are_the_single_scene_command(task, mm, arena):
    """rows all CUSTOM: the bytes of a handle with set_point_scene(CUSTOM); rows all default: the bytes of an untouched handle
    -- actions, states, costs, BUF_TRAJ_COST, the plan and every other buffer, over three warm-started commands"""
    t = Twin(0, K=100, T=X.T, task=task, goal=X.GOAL, multi_modal=mm, filter_u=False)
    try:
        t.A.set_point_rollout_scenes([X.CUSTOM if arena == "custom" else None] * 100)
        if arena == "custom":
            t.B.set_point_scene(X.CUSTOM)
        for c in range(3):
            t.set_world(c)
            t.A.command()
            t.B.command()
            torch.cuda.synchronize()
            assert t.assert_same(f"{arena} call {c}") == c + 1
    finally:
        t.close()


# ------------------------------------------------------------------ 4: commands vs the stitched oracle planner
@pytest.mark.parametrize("task,mm", [("push", False), ("push_pull", True)])
def test_three_commands_with_an_arena_per_sample_vs_the_oracle_planner(oracle, task, mm):
    """the figures of tests/test_point_scene_gpu.py::test_three_commands_in_the_custom_arena_vs_the_oracle_planner: control output
    atol 1e-3 on every command, the first command's rollout bit for bit and mean atol 1e-4, weights rtol 2e-3 atol 1e-6 with
    frac 0 on the first command and 0.01, cap 1e-3 afterwards"""
    from tests.conftest import assert_close_but_few
    K, T = 256, 12
    rows = R.cycle_rows(K)
    w0 = X.start_worlds(oracle)[2].copy()
    R.assert_rows_matter(oracle, task, mm, K, w0, f"{task} K={K} T={T}", T=T)
    eng, opl = _pair(oracle, task, mm, K, rows, T=T, filter_u=True)   # (the config of the test whose figures these are)
    try:
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


# ------------------------------------------------------------------ 5: life cycle
def test_life_cycle(oracle):
    K = 64
    w0 = X.start_worlds(oracle)[2]
    rows_a, rows_b = R.cycle_rows(K), R.cycle_rows(K, 1)
    R.assert_rows_matter(oracle, "push", False, K, w0, "rows B", rows=rows_b)
    eng, _ = _pair(oracle, "push", False, K, rows_a)
    never = HipEngine(make_config(K=K, T=X.T, nu=2, filter_u=False, **PK))
    try:
        never.set_objective("push", X.GOAL); never.set_noise(X.actions(K, X.T))
        eng.set_world_point_raw(raw_world(w0))
        eng.command(sync_host=True)
        # rows B, reset, command: the oracle under B
        eng.set_point_rollout_scenes(rows_b)
        eng.reset()
        assert eng.point_rollout_scenes_set()                   # the rows survive m3_reset
        eng.command(sync_host=True)
        opl = R.make_stitched(oracle, oracle.make_cfg(K, X.T, 2, task="push", goal=X.GOAL, filter_u=False), X.actions(K, X.T), rows_b)
        opl.command(w0)
        _assert_rollout_bits(eng, opl, "rows B after a reset")
        # the getter round-trips every field
        for i in (0, 1, K - 1):
            assert eng.point_rollout_scene(i) == {k: float(F(v)) for k, v in X.scene_dict(rows_b[i]).items()}, i
        # cleared: byte for byte the handle that never had rows
        eng.set_point_rollout_scenes(None)
        assert not eng.point_rollout_scenes_set()
        with pytest.raises(L.M3Error):
            eng.point_rollout_scene(0)
        eng.reset()
        for c in range(3):
            w = w0.copy(); w[0] += 0.02 * c
            for e in (eng, never):
                e.set_world_point_raw(raw_world(w))
                e.command()
            torch.cuda.synchronize()
            for b in (L.BUF_ACTION_OUT, L.BUF_MEAN, L.BUF_BEST, L.BUF_WEIGHTS, L.BUF_TRAJ_COST, L.BUF_COST_HORIZON, L.BUF_STATES,
                      L.BUF_ACTIONS, L.BUF_PENDING_FORCE):
                assert eng.buffer(b).cpu().numpy().tobytes() == never.buffer(b).cpu().numpy().tobytes(), (c, b)
            assert bytes(eng.info()) == bytes(never.info())
        # m3_set_point_scene after rows clears them: the last call wins
        eng.set_point_rollout_scenes(rows_a)
        assert eng.point_rollout_scenes_set()
        eng.set_point_scene(X.CUSTOM)
        assert not eng.point_rollout_scenes_set()
    finally:
        eng.close()
        never.close()


# ------------------------------------------------------------------ 6: tuned cost weights on top of rows
def test_rows_with_tuned_cost_weights_differ_from_the_default_weights_only_in_the_costs(oracle):
    """the per-sample build is a weighted build: tuned weights leave the first command's states and actions (which do not
    depend on the cost) at the stitched oracle's bits and change the costs"""
    w0 = X.start_worlds(oracle)[2]
    R.assert_rows_matter(oracle, "push", False, 64, w0, "push K=64")
    eng, opl = _pair(oracle, "push", False, 64, R.cycle_rows(64))
    try:
        eng.set_point_cost_weights(W_TUNED)
        eng.set_world_point_raw(raw_world(w0))
        eng.command(sync_host=True)
        opl.command(w0)
        np.testing.assert_array_equal(eng.states.cpu().numpy().view(np.uint32), opl.last["states"].view(np.uint32))
        np.testing.assert_array_equal(eng.actions.cpu().numpy().view(np.uint32), opl.last["actions"].view(np.uint32))
        assert (eng.cost_horizon.cpu().numpy() != opl.last["cost_h"]).mean() > 0.9
    finally:
        eng.close()


# ------------------------------------------------------------------ 7: refusals, none of which launches anything
def test_refusals():
    lib = L.load()
    K = 64
    rows = R.cycle_rows(K)
    arr = (L.PointSceneFields * K)(*[L.PointSceneFields(**X.scene_dict(r)) for r in rows])
    sim = HipEngine(make_config(K=K, T=1, nu=2, sim_only=True, filter_u=False, **PK))
    try:
        assert lib.m3_set_point_rollout_scenes(sim._h, arr, K) == -4
        assert b"m3_set_point_scene_rows" in lib.m3_last_error(sim._h)
    finally:
        sim.close()
    p = HipEngine(make_config(K=64, T=12, nu=9, env_type="panda_env", u_min=[-2] * 9, u_max=[2] * 9, noise_sigma_diag=[1] * 9))
    try:
        sc = L.PointSceneFields()
        assert lib.m3_set_point_rollout_scenes(p._h, arr, K) == -5
        assert lib.m3_get_point_rollout_scene(p._h, 0, C.byref(sc)) == -5
    finally:
        p.close()
    e = HipEngine(make_config(K=K, T=12, nu=2, **PK))
    try:
        e.set_objective("push", X.GOAL); e.set_noise(_noise(K, 12, 3))
        assert lib.m3_set_point_scene_rows(e._h, arr, K) == -4             # the per-environment call stays a sim_only call
        with pytest.raises(L.M3Error, match="K_local"):
            e.set_point_rollout_scenes(rows[:-1])
        assert not e.point_rollout_scenes_set()
        e.set_point_rollout_scenes(rows)
        bad = list(rows)
        bad[3] = dict(box_m=float("nan"))
        with pytest.raises(L.M3Error, match=r"row 3.*box_m"):
            e.set_point_rollout_scenes(bad)
        for i in range(5):                                                   # a refused call changes nothing
            assert e.point_rollout_scene(i) == {k: float(F(v)) for k, v in X.scene_dict(rows[i]).items()}, i
        calls = e.info().calls
        e.set_point_scene_instance(0)
        with pytest.raises(L.M3Error, match="forced off"):
            e.command()
        assert e.info().calls == calls
        e.set_point_scene_instance(-1)
        e.command(sync_host=True)
    finally:
        e.close()
    # the batched command: not with such a handle -- and with the other two afterwards
    twins = [Twin(i, K=K, T=12, task="push", goal=X.GOAL) for i in range(3)]
    batch = HipBatch(3)
    try:
        twins[1].A.set_point_rollout_scenes(rows)
        for t in twins:
            t.set_world(0)
        before = [t.A.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes() for t in twins]
        with pytest.raises(L.M3Error, match=r"error -5: .*handle 1.*m3_set_point_rollout_scenes"):
            batch.command([t.A for t in twins])
        torch.cuda.synchronize()
        assert [t.A.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes() for t in twins] == before
        assert all(t.A.info().calls == 0 for t in twins)
        batch.command([twins[0].A, twins[2].A])
        twins[0].B.command(); twins[2].B.command()
        torch.cuda.synchronize()
        assert twins[0].assert_same("after the refusal") == 1 and twins[2].assert_same("after the refusal") == 1
        assert batch.launches()[0] == 1
    finally:
        batch.close()
        for t in twins:
            t.close()


# ------------------------------------------------------------------ 8: shards
def test_two_shards_equal_the_unsharded_handle_with_all_rows(oracle):
    """built like tests/test_point_scene_gpu.py::test_two_shards_equal_the_unsharded_handle_in_the_custom_arena: each shard gets
    its slice of the 128 rows; side by side their rollouts are the bytes of the unsharded handle's"""
    from tests.sharded_update_driver import Case, HipBackend, smooth_noise
    case = Case("rollout_scenes", 0, "single", (64, 64), None, T=12)
    assert case.K == 128
    rows = R.cycle_rows(128)
    shards = [HipBackend().engine(case, r) for r in range(2)]
    whole = HipEngine(make_config(K=case.K, T=case.T, nu=2, lambda_=1.0, **PK))
    plain = HipEngine(make_config(K=case.K, T=case.T, nu=2, lambda_=1.0, **PK))
    delta = smooth_noise(case.K, case.T, 2, 4)
    world = raw_world(X.start_worlds(oracle)[2])
    try:
        for e, lo, hi in [(shards[0], 0, 64), (shards[1], 64, 128), (whole, 0, 128), (plain, 0, 128)]:
            e.set_noise(delta[lo:hi])
            e.set_objective("push", X.GOAL)
            e.set_world_point_raw(world)
            if e is not plain:
                e.set_point_rollout_scenes(rows[lo:hi])
            e.rollout()
        torch.cuda.synchronize()
        for b in (L.BUF_TRAJ_COST, L.BUF_COST_HORIZON):
            cat = torch.cat([s.buffer(b) for s in shards], dim=-1).cpu().numpy()
            assert cat.tobytes() == whole.buffer(b).cpu().numpy().tobytes(), b
        for b in (L.BUF_STATES, L.BUF_ACTIONS):
            cat = torch.cat([s.buffer(b) for s in shards], dim=1).cpu().numpy()
            assert cat.tobytes() == whole.buffer(b).cpu().numpy().tobytes(), b
        # (64 is not a multiple of three: shard 1's row 0 is row 64 of the cycle, not row 0)
        differs = (plain.buffer(L.BUF_STATES) != whole.buffer(L.BUF_STATES)).any(dim=0).any(dim=-1).float().mean().item()
        assert differs >= 0.25, differs
    finally:
        for e in shards + [whole, plain]:
            e.close()


# ------------------------------------------------------------------ 9: fused is the step path
def _side_with_rows(follow):
    """a planner with fused=None whose K-env wrapper carries the cycle's arenas, one per environment"""
    import m3p2i_aip.utils.isaacgym_utils.isaacgym_wrapper as wrapper
    from tests.test_cost_weights_gpu import _side
    K = 64
    t = _side(["task=push", "goal=[-1.0, -1.0]", f"mppi.num_samples={K}", "mppi.horizon=12", "mppi.u_per_command=12"])
    t.sim.stop_sim()
    t.sim = wrapper.IsaacGymWrapper(t.cfg.isaacgym, t.cfg.env_type, num_envs=K, viewer=False, device=t.cfg.mppi.device,
                                    point_scenes=R.cycle_rows(K))
    t.motion_planner.attach(sim=t.sim)
    t.motion_planner.follow_sim_scene = follow
    return t


@pytest.mark.parametrize("follow", [True, False])
def test_fused_path_is_the_step_path_on_a_wrapper_with_an_arena_per_environment(follow):
    t = _side_with_rows(follow)
    try:
        p = t.motion_planner
        assert p._fused is None and t.sim.point_scenes is not None and t.sim.num_envs == p.K_local
        t.first_plan(t.sim._dof_state[0:1].clone(), t.sim._root_state[0:1].clone())
        print(f"follow_sim_scene={follow}: probe {p.probe_result}")
        assert p.probe_result["fused"] is follow
        assert p._engine.point_rollout_scenes_set() is follow
    finally:
        t.close()


# ------------------------------------------------------------------ 10: never the two-wavefront form
def test_rows_never_take_the_two_wavefront_form(oracle):
    K = 64
    eng = HipEngine(make_config(K=K, T=X.T, nu=2, filter_u=False, **PK))
    try:
        eng.set_objective("navigation", X.GOAL); eng.set_noise(X.actions(K, X.T))
        eng.set_world_point_raw(raw_world(X.start_worlds(oracle)[0]))
        eng._ck(eng.lib.m3_set_point_rollout_form(eng._h, 1))
        eng.rollout()
        assert eng.lib.m3_point_rollout_form_used(eng._h) == 1
        eng.set_point_rollout_scenes(R.cycle_rows(K))
        eng.rollout()
        assert eng.lib.m3_point_rollout_form_used(eng._h) == 0
        eng.set_point_rollout_scenes(None)
        eng.rollout()
        torch.cuda.synchronize()
        assert eng.lib.m3_point_rollout_form_used(eng._h) == 1
    finally:
        eng.close()
