"""One panda_env workspace per sample of the fused rollout (m3_set_panda_rollout_scenes) and per environment of a sim_only handle
(m3_set_panda_scene_rows) on the GPU (include/m3p2i_hip.h).

The reference of every rollout case is the stitched oracle of tests/panda_rollout_scenes_ref.py (oracle calls only; pinned to
oracle.panda.rollout by tests/test_panda_scene_rows_cpu.py), compared as bytes.  The rows are 5-cycles of workspaces, row i =
cycle[i % 5]: 5 is coprime to every samples-per-wavefront count of the three kernel forms with and without shadow slots (3, 4, 8,
62, 63, 64), so a kernel that indexed the table by slot, lane or wavefront cannot pass; each case first asserts, on the oracle
alone, that every pair of scenes of its cycle changes the costs of at least 0.8 of the samples.
Shapes: K = 64 and K = 61 (the ragged last wavefront), T = 20; step mode 65 environments x 25 steps."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, HipPandaEpisodes, make_config  # noqa: E402
from tests import panda_rollout_scenes_ref as R  # noqa: E402
from tests import panda_scene_fixture as X  # noqa: E402

F = np.float32
PK = dict(u_min=X.UMIN, u_max=X.UMAX, noise_sigma_diag=X.SIG, lambda_=0.05, pre_height_diff=0.05, dt=0.01)
GOAL = np.array(X.GOAL, F)
ORACLE_COLS = list(range(0, 47)) + [51, 52, 53] + list(range(57, 84))     # the oracle's columns of the 77 SoA rows of step mode
COMMAND_BUFS = [L.BUF_STATES, L.BUF_ACTIONS, L.BUF_COST_HORIZON, L.BUF_TRAJ_COST, L.BUF_WEIGHTS, L.BUF_MEAN, L.BUF_ACTION_OUT,
                L.BUF_TOP_IDX, L.BUF_TOP_TRAJS]
ERR_STATE, ERR_SHAPE, ERR_UNSUPPORTED = -4, -3, -5     # (include/m3p2i_hip.h)
TUNED = (("pick_ori", 25.0), ("collision", 500.0), ("pick_goal", 7.5))


@pytest.fixture(scope="module")
def P(oracle):
    import oracle.panda as P
    P.lib()
    return P


def planner_engine(K, task, grip, rows=None, lps=0, cost_kernel=True, mm=False, **kw):
    eng = HipEngine(make_config(K=K, T=X.T, nu=9, env_type="panda_env", multi_modal=mm, **{**PK, **kw}))
    eng.set_objective(task, GOAL, gripper_cmd=grip)
    eng.set_panda_lanes_per_sample(lps)
    eng.set_panda_reach_cost_kernel(cost_kernel)
    k0 = kw.get("k_offset", 0)
    eng.set_noise(X.delta_of(K)[k0:k0 + kw.get("K_local", K)])
    if rows is not None:
        eng.set_panda_rollout_scenes(rows)
    return eng


def assert_rollout_equals(eng, ref, label):
    st = eng.states.cpu().numpy()
    assert np.isfinite(st).all()
    np.testing.assert_array_equal(eng.actions.cpu().numpy().view(np.uint32), ref["actions"].view(np.uint32), err_msg=label)
    np.testing.assert_array_equal(st.view(np.uint32), ref["states"].view(np.uint32), err_msg=label)
    ch = eng.cost_horizon.cpu().numpy()
    bad = np.argwhere(ch.view(np.uint32) != ref["cost_h"].view(np.uint32))
    assert bad.size == 0, f"{label}: {len(bad)} cost mismatches, first {bad[0]}: {ch[tuple(bad[0])]!r} vs {ref['cost_h'][tuple(bad[0])]!r}"
    np.testing.assert_array_equal(eng.buffer(L.BUF_TRAJ_COST).cpu().numpy().view(np.uint32), ref["J"].view(np.uint32), err_msg=label)


def assert_cycle_shows(cycle, K):
    for pair, s in R.pair_shares(cycle, K).items():
        assert s >= 0.8, (cycle, K, pair, s)


def run_cycle_case(P, cycle, lps, K=X.K, cost_kernel=True, mm=False, lanes=0, weights=None):
    assert_cycle_shows(cycle, K)
    world, task, grip, _ = R.CYCLES[cycle]
    ref = R.cycle_reference(cycle, K, mm, weights)
    eng = planner_engine(K, task, grip, R.cycle_rows(cycle, K), lps, cost_kernel, mm)
    try:
        if lanes:
            eng.set_rollout_lanes(lanes)
        if weights is not None:
            eng.set_panda_cost_weights(dict(weights))
        eng.set_world_panda_raw(P.raw57(X.world_of(world)))
        eng.command(sync_host=True)
        assert eng.panda_lanes_per_sample_used() == lps
        assert eng.panda_rollout_scenes_set() and eng.panda_scene_instance_used()
        assert eng.panda_weighted_cost_instance_used() == (weights is not None)     # (what the WEIGHTS needed)
        assert_rollout_equals(eng, ref, f"{cycle} K {K} lps {lps} cost kernel {cost_kernel} mm {mm} lanes {lanes}")
        return eng.cost_horizon.cpu().numpy()
    finally:
        eng.close()


# ------------------------------------------------------------------ 1. rollout parity with the stitched reference
@pytest.mark.parametrize("lps", [1, 8, 16])
def test_pick_cycle_in_every_lane_form(P, lps):
    run_cycle_case(P, "pick", lps)


# reach: quirk Q8 in both realisations -- the shadow slots, and the record + reach-cost kernel behind a many-lane rollout
@pytest.mark.parametrize("lps,cost_kernel", [(1, False), (8, False), (8, True), (16, False), (16, True)])
def test_reach_cycle_in_every_lane_form_and_both_realisations_of_q8(P, lps, cost_kernel):
    run_cycle_case(P, "reach", lps, cost_kernel=cost_kernel)


@pytest.mark.parametrize("lps,cost_kernel", [(1, False), (8, True), (16, False)])
def test_reach_cycle_multi_modal(P, lps, cost_kernel):
    run_cycle_case(P, "reach", lps, cost_kernel=cost_kernel, mm=True)


@pytest.mark.parametrize("cycle,lps,cost_kernel", [("pick", 1, True), ("pick", 8, True), ("pick", 16, True), ("reach", 1, False),
                                                   ("reach", 16, True)])
def test_a_ragged_last_wavefront(P, cycle, lps, cost_kernel):
    run_cycle_case(P, cycle, lps, K=X.K_RAGGED, cost_kernel=cost_kernel)


def test_fewer_samples_per_wavefront_than_the_default(P):
    run_cycle_case(P, "pick", 1, lanes=32)            # (m3_set_rollout_lanes: a power of two, coprime to 5 too)
    run_cycle_case(P, "reach", 16, cost_kernel=False, lanes=2)


def test_tuned_weights_on_the_pick_cycle(P):
    tuned = run_cycle_case(P, "pick", 16, weights=TUNED)
    assert tuned.tobytes() != R.cycle_reference("pick")["cost_h"].tobytes()              # the weights show


@pytest.mark.parametrize("cycle,lps,cost_kernel", [("pick", 8, True), ("reach", 16, True)])
def test_two_warm_started_commands(P, cycle, lps, cost_kernel):
    """the second command's rollout, which starts from the first one's update: its STATES, COST_HORIZON and TRAJ_COST are the
    stitched reference's under its own ACTIONS"""
    K = X.K
    world, task, grip, _ = R.CYCLES[cycle]
    rows = R.cycle_rows(cycle, K)
    cfg = P.make_cfg(K, X.T, multi_modal=False, task=task, goal=GOAL, gripper_cmd=grip)
    eng = planner_engine(K, task, grip, rows, lps, cost_kernel)
    try:
        w0 = X.world_of(world)
        eng.set_world_panda_raw(P.raw57(w0))
        eng.command(sync_host=True)
        assert_rollout_equals(eng, R.cycle_reference(cycle), f"{cycle} first command")
        first = eng.actions.cpu().numpy().copy()
        eng.command(sync_host=True)
        u = eng.actions.cpu().numpy()
        assert (u != first).any(axis=(1, 2)).mean() > 0.9                              # a warm start: the mean moved
        assert_rollout_equals(eng, R.stitched_rollout(P, cfg, task, rows, w0, u, scaled=True), f"{cycle} second command")
    finally:
        eng.close()


@pytest.mark.parametrize("task,grip,world,lps,cost_kernel,mm", [("pick", 2, 40, 1, True, False), ("pick", 2, 40, 8, True, False),
                                                                ("reach", 2, 41, 16, True, False), ("reach", 2, 41, 1, False, True),
                                                                ("reach", 2, 41, 16, False, True)])
def test_rows_that_equal_one_scene_are_the_weighted_family_in_that_scene(P, task, grip, world, lps, cost_kernel, mm):
    """k_rollout_panda_v with K equal rows against k_rollout_panda_w (forced) on m3_set_panda_scene with that scene: every
    output buffer of two commands, byte for byte"""
    K = X.K
    a = planner_engine(K, task, grip, [X.COMBINED] * K, lps, cost_kernel, mm)
    b = planner_engine(K, task, grip, None, lps, cost_kernel, mm)
    try:
        b.set_panda_scene(X.COMBINED)
        b.set_panda_weighted_cost_instance(1)
        for e in (a, b):
            e.set_world_panda_raw(P.raw57(X.world_of(world)))
        for call in range(2):
            pa, pb = a.command(sync_host=True), b.command(sync_host=True)
            assert a.panda_rollout_scenes_set() and not b.panda_rollout_scenes_set()
            assert a.panda_scene_instance_used() and b.panda_scene_instance_used()
            assert not a.panda_weighted_cost_instance_used() and b.panda_weighted_cost_instance_used()
            assert a.panda_lanes_per_sample_used() == b.panda_lanes_per_sample_used() == lps
            assert np.asarray(pa).tobytes() == np.asarray(pb).tobytes(), call
            for buf in COMMAND_BUFS:
                assert a.buffer(buf).cpu().numpy().tobytes() == b.buffer(buf).cpu().numpy().tobytes(), (call, buf)
            assert bytes(a.info()) == bytes(b.info()), call
        assert np.ptp(a.states.cpu().numpy(), axis=0).max() > 0 and np.ptp(a.cost_horizon.cpu().numpy()) > 0
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------ 2. a shard
def test_a_shard_with_its_slice_of_the_rows_leaves_its_rows_of_the_unsharded_result(P):
    K, Kl, k0 = X.K, 32, 32
    assert_cycle_shows("pick", K)
    world, task, grip, _ = R.CYCLES["pick"]
    rows = R.cycle_rows("pick", K)
    full = planner_engine(K, task, grip, rows)
    part = planner_engine(K, task, grip, rows[k0:], K_local=Kl, k_offset=k0)
    try:
        with pytest.raises(L.M3Error, match="m3_set_panda_rollout_scenes: n is 64, the handle's K_local 32"):
            part.set_panda_rollout_scenes(rows)                                         # its own K_local rows, not the global list
        for e in (full, part):
            e.set_world_panda_raw(P.raw57(X.world_of(world)))
            e.rollout()
        torch.cuda.synchronize()
        ref = R.cycle_reference("pick")
        for name, buf in (("actions", lambda e: e.actions), ("states", lambda e: e.states)):
            whole, mine = buf(full).cpu().numpy(), buf(part).cpu().numpy()
            assert whole[k0:].tobytes() == mine.tobytes() == ref[name][k0:].tobytes(), name
        # (pick: no quirk Q8, so the shard's costs are the unsharded handle's too)
        assert full.buffer(L.BUF_TRAJ_COST).cpu().numpy()[k0:].tobytes() == part.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes()
        assert part.panda_rollout_scene(0) == L.panda_scene_dict(L.panda_scene_fields(rows[k0]))
    finally:
        full.close(); part.close()


# ------------------------------------------------------------------ 3. step mode on a sim_only handle
STEP_CYCLE = (None, "table_z", "mu", "base", "COMBINED")


def _load_worlds(sim, P, w):
    n = len(w)
    ia, ib, io = (int(sim._get_actor_index_by_name(x)) for x in ("cubeA", "cubeB", "dyn-obs"))
    dof = torch.zeros(n, 18)
    dof[:, 0::2] = torch.from_numpy(w[:, P.W_Q:P.W_Q + 9])
    dof[:, 1::2] = torch.from_numpy(w[:, P.W_QD:P.W_QD + 9])
    root = sim._root_state.clone().cpu()
    root[:, ia, :] = torch.from_numpy(w[:, P.W_CUBEA:P.W_CUBEA + 13])
    root[:, ib, :] = torch.from_numpy(w[:, P.W_CUBEB:P.W_CUBEB + 13])
    root[:, io, :] = torch.from_numpy(w[:, P.W_OBS:P.W_OBS + 13])
    sim._dof_state[:] = dof.to("cuda:0")
    sim._root_state[:] = root.to("cuda:0")
    sim.set_dof_state_tensor(sim._dof_state)
    sim.set_actor_root_state_tensor(sim._root_state)


def test_step_mode_cost_and_link_poses_per_row_then_null(P):
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    from tests.test_device_dynamics_on_host import random_panda_worlds
    n, steps = X.STEP_ENVS, X.STEP_STEPS
    fields = [R.fields_of(s) for s in STEP_CYCLE]
    scene_of = np.arange(n) % 5
    osc = [X.oracle_scene(P, f) for f in fields]
    rng = np.random.default_rng(70)
    w = random_panda_worlds(P, P.default_scene(), n, rng)
    start = w.copy()
    sim = IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=n, device="cuda:0", panda_scenes=[fields[g] for g in scene_of])
    plain = IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=n, device="cuda:0")
    try:
        eng = sim._engine
        assert eng.panda_scene_rows_set() and sim.panda_scene is None and len(sim.panda_scenes) == n
        assert eng.panda_scene_row(3) == L.panda_scene_dict(L.panda_scene_fields(fields[3])) == sim.panda_scenes[3]
        r0 = int(sim.bodies_per_env) - 11
        rb = sim._rigid_body_state.cpu().numpy()
        assert np.allclose(rb[3, r0, :3], X.PROBES["base"][0]["base"]) and np.allclose(rb[0, r0, :3], X.DEFAULTS["base"])
        _load_worlds(sim, P, w)
        w[:, P.W_HELD:] = 0.0
        w[:, P.W_RELQ + 3] = 1.0
        w[:, P.W_AWAKE:P.W_AWAKE + 2] = 1.0
        for i in range(n):
            row = np.ascontiguousarray(w[i])
            P.infer_state(osc[scene_of[i]], row)
            w[i] = row
        grip = rng.integers(0, 3, n)
        us = []
        for t in range(steps):
            u = rng.uniform(-2, 2, (n, 9)).astype(F)
            u[:, 7:] = rng.uniform(-1.5, 1.5, (n, 2))
            u[grip == 1, 7:] = 1.5
            u[grip == 2, 7:] = -1.5
            us.append(u)
            for g in range(5):                                # the oracle: step_batch per group of equal scenes
                idx = np.flatnonzero(scene_of == g)
                sub = np.ascontiguousarray(w[idx])
                P.step_batch(osc[g], sub, np.ascontiguousarray(u[idx]))
                w[idx] = sub
            sim.set_dof_velocity_target_tensor(torch.from_numpy(u).to("cuda:0"))
            sim.step()
            assert eng.panda_scene_instance_used()
            got = eng.buffer(L.BUF_SIM_WORLD).cpu().numpy().reshape(77, n).T
            neq = got.view(np.uint32) != w[:, ORACLE_COLS].view(np.uint32)
            if neq.any():
                r, c = np.argwhere(neq)[0]
                raise AssertionError(f"step {t} environment {r} row {c}: oracle {w[r, ORACLE_COLS[c]]!r} device {got[r, c]!r} "
                                     f"({int(neq.sum())} values differ)")
        assert np.isfinite(w[:, ORACLE_COLS]).all()
        # the pushed link poses: the forward kinematics in each row's base
        rb = sim._rigid_body_state.cpu().numpy()
        for e in (0, 1, 2, 3, 4, 31, 63, 64):
            Lk = P.fk(osc[scene_of[e]], w[e, :9])
            want = np.concatenate([Lk["pos"], Lk["quat"]], axis=1).astype(F)
            np.testing.assert_array_equal(rb[e, r0:r0 + 11, :7], want)
        # m3_cost per row: pick (reads the contact forces) and reach (quirk Q8: environment 0's cube, as row 0's workspace left it)
        obs = np.stack([P.observe(osc[scene_of[e]], w[e]) for e in range(n)])
        for task, g in (("pick", 2), ("reach", 1)):
            cfg = P.make_cfg(n, X.T, multi_modal=False, task=task, goal=GOAL, gripper_cmd=g)
            o = obs.copy()
            if task == "reach":
                o[:, 17:20], o[:, 20:24] = obs[0, 10:13], obs[0, 13:17]
            eng.set_objective(task, GOAL, gripper_cmd=g)
            got = eng.cost().cpu().numpy()
            np.testing.assert_array_equal(got.view(np.uint32), P.cost_obs(cfg, o).view(np.uint32), err_msg=task)
            assert not eng.panda_weighted_cost_instance_used()
        # NULL: the bytes of a handle that never had rows
        eng.set_panda_scene_rows(None)
        assert not eng.panda_scene_rows_set()
        with pytest.raises(L.M3Error):
            eng.panda_scene_row(0)
        for s in (sim, plain):
            _load_worlds(s, P, start)
            for t in range(3):
                s.set_dof_velocity_target_tensor(torch.from_numpy(us[t]).to("cuda:0"))
                s.step()
        assert not eng.panda_scene_instance_used()
        plain._engine.set_objective("reach", GOAL, gripper_cmd=1)
        # (bodies 3 ..: the plate, the cubes, the robot's links -- the rows of the table and the shelf stand still show the poses
        # the wrapper was built with)
        for a, b in ((eng.buffer(L.BUF_SIM_WORLD), plain._engine.buffer(L.BUF_SIM_WORLD)),
                     (sim._rigid_body_state[:, 3:], plain._rigid_body_state[:, 3:]),
                     (sim._net_contact_force, plain._net_contact_force), (eng.cost(), plain._engine.cost())):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    finally:
        sim.stop_sim(); plain.stop_sim()


# ------------------------------------------------------------------ 4. life cycle and refusals (nothing is launched)
def _array(rows):
    arr = (L.PandaSceneFields * len(rows))()
    for i, r in enumerate(rows):
        arr[i] = L.panda_scene_fields(r)
    return arr


def test_life_cycle_and_refusals(P):
    K = X.K
    rows = R.cycle_rows("reach", K)
    eng = planner_engine(K, "reach", 2)
    world = HipEngine(make_config(K=K, T=1, nu=9, env_type="panda_env", dt=0.01, sim_only=True, filter_u=False))
    pt = HipEngine(make_config(K=64, T=10, nu=2, env_type="point_env"))
    try:
        lib, d = eng.lib, L.PandaSceneFields()
        eng.set_world_panda_raw(P.raw57(X.world_of(41)))
        eng.command(sync_host=True)
        calls, J = eng.info().calls, eng.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes()
        # the wrong environment, the wrong handle kind, the wrong n, a bad field in row 3
        for setter in (pt.set_panda_scene_rows, pt.set_panda_rollout_scenes):
            with pytest.raises(L.M3Error, match="m3_set_panda_(scene_rows|rollout_scenes): panda_env only"):
                setter(rows)
        assert lib.m3_set_panda_rollout_scenes(pt._h, _array(rows), K) == ERR_UNSUPPORTED
        assert lib.m3_get_panda_rollout_scene(pt._h, 0, C.byref(d)) == ERR_UNSUPPORTED
        with pytest.raises(L.M3Error, match="m3_set_panda_scene_rows: sim_only handles only .*m3_set_panda_rollout_scenes"):
            eng.set_panda_scene_rows(rows)
        with pytest.raises(L.M3Error, match="m3_set_panda_rollout_scenes: planner handles only .*m3_set_panda_scene_rows"):
            world.set_panda_rollout_scenes(rows)
        assert lib.m3_set_panda_scene_rows(eng._h, _array(rows), K) == ERR_STATE
        with pytest.raises(L.M3Error, match="m3_set_panda_rollout_scenes: n is 63, the handle's K_local 64"):
            eng.set_panda_rollout_scenes(rows[:63])
        assert lib.m3_set_panda_rollout_scenes(eng._h, _array(rows), K - 1) == ERR_SHAPE
        for bad, msg in ((dict(table=(0.0, 0.0, 1.0, 0.6, 0.6, 0.0)), r"row 3: table\[5\] must be > 0"),
                         (dict(mu=float("nan")), "row 3: mu is not finite"), (dict(cube_m=-1.0), "row 3: cube_m must be > 0")):
            with pytest.raises(L.M3Error, match="m3_set_panda_rollout_scenes: " + msg):
                eng.set_panda_rollout_scenes(rows[:3] + [bad] + rows[4:])
            assert not eng.panda_rollout_scenes_set()                                   # every check before any state changes
        assert lib.m3_get_panda_rollout_scene(eng._h, 0, C.byref(d)) == ERR_STATE       # off: no row to read
        # set / get, survive m3_reset, m3_set_panda_scene afterwards wins, NULL clears
        eng.set_panda_rollout_scenes(rows)
        assert eng.panda_rollout_scenes_set()
        for i in (0, 1, 4, 63):
            assert eng.panda_rollout_scene(i) == L.panda_scene_dict(L.panda_scene_fields(rows[i]))
        assert lib.m3_get_panda_rollout_scene(eng._h, K, C.byref(d)) != 0 and lib.m3_get_panda_rollout_scene(eng._h, -1, C.byref(d)) != 0
        eng.reset()
        assert eng.panda_rollout_scenes_set() and eng.panda_rollout_scene(3) == L.panda_scene_dict(L.panda_scene_fields(rows[3]))
        eng.set_panda_scene(mu=0.5)
        assert not eng.panda_rollout_scenes_set()                                       # the last call wins
        eng.set_panda_rollout_scenes(rows)
        assert eng.panda_rollout_scenes_set() and eng.panda_scene()["mu"] == 0.5        # ... in both directions
        eng.set_panda_rollout_scenes(None)
        assert not eng.panda_rollout_scenes_set()
        eng.set_panda_scene(None)
        # the scene instance forced off with rows on: M3_ERR_STATE, nothing ran
        eng.set_panda_rollout_scenes(rows)
        eng.set_panda_scene_instance(0)
        eng.set_world_panda_raw(P.raw57(X.world_of(41)))
        calls = eng.info().calls
        J = eng.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes()
        for run in (eng.command, eng.rollout):
            with pytest.raises(L.M3Error, match="forced off .*m3_set_panda_rollout_scenes"):
                run()
        torch.cuda.synchronize()
        assert eng.info().calls == calls and eng.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes() == J
        eng.set_panda_scene_instance(-1)
        eng.command(sync_host=True)
        assert eng.info().calls == calls + 1 and eng.panda_scene_instance_used()
        # the world handle: rows per environment; m3_set_panda_scene afterwards wins there too
        world.set_panda_scene_rows(rows)
        assert world.panda_scene_rows_set() and world.panda_scene_row(1) == L.panda_scene_dict(L.panda_scene_fields(rows[1]))
        world.set_panda_scene(None)
        assert not world.panda_scene_rows_set()
    finally:
        eng.close(); world.close(); pt.close()


def test_batch_refuses_a_handle_with_rows_and_then_works_without_it(P):
    engs = [planner_engine(X.K, "pick", 2) for _ in range(3)]
    batch = HipBatch(3)
    try:
        for e in engs:
            e.set_world_panda_raw(P.raw57(X.world_of(40)))
        batch.command(engs)
        torch.cuda.synchronize()
        engs[1].set_panda_rollout_scenes([None] * X.K)                       # even K default rows: keyed on the flag
        before = [e.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes() for e in engs]
        infos = [bytes(e.info()) for e in engs]
        with pytest.raises(L.M3Error, match="m3_batch_command: handle 1: .*m3_set_panda_rollout_scenes"):
            batch.command(engs)
        torch.cuda.synchronize()
        assert [e.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes() for e in engs] == before
        assert [bytes(e.info()) for e in engs] == infos                      # nothing was launched
        batch.command([engs[0], engs[2]])                                    # the same batch without that handle
        torch.cuda.synchronize()
        assert engs[0].info().calls == 2 and engs[2].info().calls == 2 and engs[1].info().calls == 1
        engs[1].set_panda_rollout_scenes(None)                               # ... and with it again, once its rows are off
        batch.command(engs)
        torch.cuda.synchronize()
        assert [e.info().calls for e in engs] == [3, 2, 3]
    finally:
        batch.close()
        for e in engs:
            e.close()


def test_panda_episodes_refuse_rows_on_the_world_and_on_a_planner(P):
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    n = 2
    world = IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=n, device="cuda:0")
    planners = [planner_engine(X.K, "reach", 1) for _ in range(n)]
    try:
        for e in planners:
            e.set_action_out(torch.zeros(X.T, 9, device="cuda:0"))
        planners[1].set_panda_rollout_scenes([None] * X.K)
        with pytest.raises(L.M3Error, match="m3_panda_episodes_create: planner 1: .*m3_set_panda_rollout_scenes"):
            HipPandaEpisodes(world._engine, planners, max_ticks=4)
        planners[1].set_panda_rollout_scenes(None)
        world._engine.set_panda_scene_rows([None, dict(mu=0.5)])
        with pytest.raises(L.M3Error, match="m3_panda_episodes_create: the world: .*m3_set_panda_scene_rows"):
            HipPandaEpisodes(world._engine, planners, max_ticks=4)
        world._engine.set_panda_scene_rows(None)
        eps = HipPandaEpisodes(world._engine, planners, max_ticks=4)
        try:
            planners[0].set_panda_rollout_scenes([None] * X.K)               # set after create: the tick is refused, not run
            with pytest.raises(L.M3Error, match="m3_panda_episodes_observe: planner 0: .*m3_set_panda_rollout_scenes"):
                eps.observe()
            planners[0].set_panda_rollout_scenes(None)
            world._engine.set_panda_scene_rows([None, None])
            with pytest.raises(L.M3Error, match="m3_panda_episodes_observe: the world: .*m3_set_panda_scene_rows"):
                eps.observe()
        finally:
            eps.close()
    finally:
        world.stop_sim()
        for e in planners:
            e.close()


# ------------------------------------------------------------------ 5. Python end to end
def test_planner_takes_the_rows_of_its_wrapper_and_keeps_the_fused_path(P):
    from tests.test_planner_api_panda_gpu import Tamp, make_cfg
    K, T = X.K, X.T
    rows = R.cycle_rows("reach", K)

    class TampR(Tamp):
        def __init__(self, cfg):
            from m3p2i_aip_amd import isaacgym_wrapper as wrapper
            from m3p2i_aip_amd.cost_functions import Objective
            from m3p2i_aip_amd.planner import M3P2I
            self.sim = wrapper.IsaacGymWrapper(cfg.isaacgym, cfg.env_type, num_envs=cfg.mppi.num_samples, viewer=False,
                                               device=cfg.mppi.device, panda_scenes=rows)
            self.cfg, self.objective = cfg, Objective(cfg)
            self.motion_planner = M3P2I(cfg, dynamics=self.dynamics, running_cost=self.running_cost)

    tamp = TampR(make_cfg(K, T, fused=None))
    try:
        pl = tamp.motion_planner
        assert pl.has_panda_rollout_scenes
        pl.set_noise(X.delta_of(K).copy())
        pl.update_gripper_command("reach")
        tamp.objective.update_objective("reach", torch.tensor(list(X.GOAL)))
        a = pl.command(tamp.sim._dof_state[0])
        assert torch.isfinite(a).all()
        # the probe compared like with like -- the fused rollout in K workspaces, the step path on the wrapper's K workspaces
        assert pl.probe_result["fused"] is True and pl.probe_result["max_abs_diff"] == 0.0
        assert pl._engine.lib.m3_panda_rollout_scenes_set(pl._engine._h) == 1
        assert tamp.sim._engine.lib.m3_panda_scene_rows_set(tamp.sim._engine._h) == 1
        assert pl._engine.panda_rollout_scene(3) == tamp.sim.panda_scenes[3] == tamp.sim._engine.panda_scene_row(3)
        J = pl._engine.buffer(L.BUF_TRAJ_COST).cpu().numpy()
        assert np.isfinite(J).all() and np.ptp(J) > 0
        pl.command(tamp.sim._dof_state[0])
        assert pl._engine.panda_rollout_scenes_set() and pl._engine.panda_scene_instance_used()
    finally:
        tamp.sim.stop_sim()
