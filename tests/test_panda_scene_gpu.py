"""The run-time panda_env workspace on the GPU (m3_set_panda_scene, include/m3p2i_hip.h).

The reference of every case is the unchanged CPU oracle in the same workspace (oracle/panda_chain.c carries the whole workspace
as run-time fields), bit for bit.  Every rollout case first asserts, on the oracle alone, that its probe scene changes the costs
of most samples in its world (tests/panda_scene_fixture.py: share) -- a scene that shows nowhere would pass while testing nothing.
Shapes: rollouts K = 64, T = 20 (one wavefront at one lane per sample, sixteen at sixteen), K = 61 once per form; step mode 65
environments (two wavefronts, the second with one lane) x 25 steps."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, HipPandaEpisodes, make_config  # noqa: E402
from tests import panda_scene_fixture as X  # noqa: E402

F = np.float32
PK = dict(u_min=X.UMIN, u_max=X.UMAX, noise_sigma_diag=X.SIG, lambda_=0.05, pre_height_diff=0.05, dt=0.01)
GOAL = np.array(X.GOAL, F)
# the oracle's world columns of the 77 SoA rows of step mode (no orientation / angular velocity of the plate)
ORACLE_COLS = list(range(0, 47)) + [51, 52, 53] + list(range(57, 84))


@pytest.fixture(scope="module")
def P(oracle):
    import oracle.panda as P
    P.lib()
    return P


def planner_engine(K, task, grip, scene=None, lps=0, cost_kernel=True, **kw):
    eng = HipEngine(make_config(K=K, T=X.T, nu=9, env_type="panda_env", **{**PK, **kw}))
    eng.set_objective(task, GOAL, gripper_cmd=grip)
    eng.set_panda_lanes_per_sample(lps)
    eng.set_panda_reach_cost_kernel(cost_kernel)
    eng.set_noise(X.delta_of(K))
    if scene is not None:
        eng.set_panda_scene(scene)
    return eng


def assert_rollout_equals_oracle(P, eng, ref, label):
    st = eng.states.cpu().numpy()
    assert np.isfinite(st).all()
    np.testing.assert_array_equal(eng.actions.cpu().numpy().view(np.uint32), ref["actions"].view(np.uint32), err_msg=label)
    np.testing.assert_array_equal(st.view(np.uint32), ref["states"].view(np.uint32), err_msg=label)
    ch = eng.cost_horizon.cpu().numpy()
    bad = np.argwhere(ch.view(np.uint32) != ref["cost_h"].view(np.uint32))
    assert bad.size == 0, f"{label}: {len(bad)} cost mismatches, first {bad[0]}: {ch[tuple(bad[0])]!r} vs {ref['cost_h'][tuple(bad[0])]!r}"
    np.testing.assert_array_equal(eng.buffer(L.BUF_TRAJ_COST).cpu().numpy().view(np.uint32), ref["J"].view(np.uint32), err_msg=label)


def run_rollout_case(P, scene_name, world, task, grip, lps, K=X.K, cost_kernel=True, want_instance=1):
    assert X.share(scene_name, world, task, grip, K) >= 0.8 or (scene_name == "COMBINED" and world in X.qualifying_fuzz_worlds()
                                                                 and X.share(scene_name, world, task, grip, K) >= 0.5)
    ref = X.oracle_rollout(scene_name, world, task, grip, K)
    eng = planner_engine(K, task, grip, X.SCENES[scene_name], lps, cost_kernel)
    try:
        eng.set_world_panda_raw(P.raw57(X.world_of(world)))
        eng.command(sync_host=True)
        assert eng.panda_lanes_per_sample_used() == lps
        assert int(eng.panda_scene_instance_used()) == want_instance
        assert_rollout_equals_oracle(P, eng, ref, f"{scene_name} world {world} {task} lps {lps}")
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. the rollout against the oracle in the scene
@pytest.mark.parametrize("lps", [1, 8, 16])
@pytest.mark.parametrize("name", list(X.PROBES))
def test_rollout_in_each_probe_scene_equals_the_oracle(P, name, lps):
    _, world, task, grip, masses_only = X.PROBES[name]
    run_rollout_case(P, name, world, task, grip, lps, want_instance=0 if masses_only else 1)


def test_combined_shows_in_at_least_30_of_the_42_fuzz_worlds(P):
    assert len(X.qualifying_fuzz_worlds()) >= 30


@pytest.mark.parametrize("lps", [1, 8, 16])
@pytest.mark.parametrize("j", range(12))
def test_rollout_in_combined_on_fuzz_worlds_equals_the_oracle(P, j, lps):
    q = X.qualifying_fuzz_worlds()
    assert len(q) >= 30
    world = q[(j * len(q)) // 12]          # twelve of them, spread over the list (and so over the four tasks)
    task, grip = X.FUZZ_TASKS[world % 4]
    run_rollout_case(P, "COMBINED", world, task, grip, lps, cost_kernel=(j % 2 == 0))


@pytest.mark.parametrize("lps", [1, 8, 16])
def test_rollout_with_a_ragged_last_wavefront(P, lps):
    run_rollout_case(P, "COMBINED", 41, "reach", 2, lps, K=X.K_RAGGED)


# ------------------------------------------------------------------ 5. the forced instance at the default values
COMMAND_BUFS = [L.BUF_STATES, L.BUF_ACTIONS, L.BUF_COST_HORIZON, L.BUF_TRAJ_COST, L.BUF_WEIGHTS, L.BUF_MEAN, L.BUF_ACTION_OUT,
                L.BUF_TOP_IDX, L.BUF_TOP_TRAJS]


@pytest.mark.parametrize("task,grip,world", [("reach", 1, 36), ("pick", 2, 40)])
def test_forced_instance_at_default_values_is_the_untouched_handle(P, task, grip, world):
    a, b = planner_engine(X.K, task, grip), planner_engine(X.K, task, grip)
    try:
        b.set_panda_scene_instance(1)
        for e in (a, b):
            e.set_world_panda_raw(P.raw57(X.world_of(world)))
        for call in range(3):
            pa, pb = a.command(sync_host=True), b.command(sync_host=True)
            assert not a.panda_scene_instance_used() and b.panda_scene_instance_used()
            assert a.panda_lanes_per_sample_used() == b.panda_lanes_per_sample_used()
            assert np.asarray(pa).tobytes() == np.asarray(pb).tobytes(), call
            for buf in COMMAND_BUFS:
                assert a.buffer(buf).cpu().numpy().tobytes() == b.buffer(buf).cpu().numpy().tobytes(), (call, buf)
            assert bytes(a.info()) == bytes(b.info()), call
        assert b.panda_scene() == a.panda_scene()
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------ 6. the masses stay on today's kernels, batched
def test_cube_mass_inside_a_batch_of_three(P):
    world = P.raw57(X.world_of(40))
    scenes = [None, dict(cube_m=0.4), None]
    A = [planner_engine(X.K, "pick", 2, s) for s in scenes]
    B = [planner_engine(X.K, "pick", 2, s) for s in scenes]
    batch = HipBatch(3)
    try:
        for e in A + B:
            e.set_world_panda_raw(world)
        for call in range(2):
            batch.command(A)
            assert batch.launches() == (1, 1)                # one rollout launch, one update launch for the three
            for e in B:
                e.command()
            torch.cuda.synchronize()
            for i, (x, y) in enumerate(zip(A, B)):
                assert not x.panda_scene_instance_used() and not y.panda_scene_instance_used()
                for buf in COMMAND_BUFS:
                    assert x.buffer(buf).cpu().numpy().tobytes() == y.buffer(buf).cpu().numpy().tobytes(), (call, i, buf)
                assert bytes(x.info()) == bytes(y.info())
            if call == 0:
                # the heavier cube shows, and is the oracle's: handles 0 and 2 are the default scene
                J = [e.buffer(L.BUF_TRAJ_COST).cpu().numpy() for e in A]
                assert J[0].tobytes() == J[2].tobytes() and J[0].tobytes() != J[1].tobytes()
                assert_rollout_equals_oracle(P, A[1], X.oracle_rollout("cube_m", 40, "pick", 2), "cube_m in the batch")
                assert_rollout_equals_oracle(P, A[0], X.oracle_rollout(None, 40, "pick", 2), "default in the batch")
    finally:
        batch.close()
        for e in A + B:
            e.close()


# ------------------------------------------------------------------ 7. step mode on a sim_only handle
def test_step_mode_cost_and_link_poses_in_combined(P):
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    from tests.test_device_dynamics_on_host import random_panda_worlds
    n, steps = X.STEP_ENVS, X.STEP_STEPS
    sc = X.oracle_scene(P, X.COMBINED)
    rng = np.random.default_rng(70)
    w = random_panda_worlds(P, P.default_scene(), n, rng)
    sim = IsaacGymWrapper(IsaacGymConfig(dt=0.01, panda_scene=dict(X.COMBINED)), "panda_env", num_envs=n, device="cuda:0")
    try:
        eng = sim._engine
        assert eng.panda_scene() == L.panda_scene_dict(L.panda_scene_fields(X.COMBINED)) and sim.panda_scene is not None
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
        # what a load from the wrapper's tensors starts from: the 57 raw floats, nothing derived (no latch, no relative pose, no
        # warm start, no forces) -- then the grasp and sleep state inferred from the geometry, in the scene
        w[:, P.W_HELD:] = 0.0
        w[:, P.W_RELQ + 3] = 1.0
        w[:, P.W_AWAKE:P.W_AWAKE + 2] = 1.0
        for i in range(n):
            row = np.ascontiguousarray(w[i])
            P.infer_state(sc, row)
            w[i] = row
        grip = rng.integers(0, 3, n)
        for t in range(steps):
            u = rng.uniform(-2, 2, (n, 9)).astype(F)
            u[:, 7:] = rng.uniform(-1.5, 1.5, (n, 2))
            u[grip == 1, 7:] = 1.5
            u[grip == 2, 7:] = -1.5
            P.step_batch(sc, w, u)
            sim.set_dof_velocity_target_tensor(torch.from_numpy(u).to("cuda:0"))
            sim.step()                                       # m3_sim_step_with_target
            assert eng.panda_scene_instance_used()
            got = eng.buffer(L.BUF_SIM_WORLD).cpu().numpy().reshape(77, n).T
            neq = got.view(np.uint32) != w[:, ORACLE_COLS].view(np.uint32)
            if neq.any():
                r, c = np.argwhere(neq)[0]
                raise AssertionError(f"step {t} environment {r} row {c}: oracle {w[r, ORACLE_COLS[c]]!r} device {got[r, c]!r} "
                                     f"({int(neq.sum())} values differ)")
        assert np.isfinite(w[:, ORACLE_COLS]).all()
        # the pushed link poses: the forward kinematics in the moved base
        rb = sim._rigid_body_state.cpu().numpy()
        r0 = int(sim.bodies_per_env) - 11
        for e in (0, 1, 31, 63, 64):
            Lk = P.fk(sc, w[e, :9])
            want = np.concatenate([Lk["pos"], Lk["quat"]], axis=1).astype(F)
            np.testing.assert_array_equal(rb[e, r0:r0 + 11, :7], want)      # (values, as tests/test_planner_api_panda_gpu.py
            #                                                               compares them: a zero component's sign is not pinned)
        assert np.allclose(rb[0, r0, :3], X.COMBINED["base"])
        # m3_cost: pick (reads the contact forces) and reach (quirk Q8: environment 0's cube)
        obs = np.stack([P.observe(sc, w[e]) for e in range(n)])
        for task, g in (("pick", 2), ("reach", 1)):
            cfg = P.make_cfg(n, X.T, multi_modal=False, task=task, goal=GOAL, gripper_cmd=g)
            o = obs.copy()
            if task == "reach":
                o[:, 17:20], o[:, 20:24] = obs[0, 10:13], obs[0, 13:17]
            eng.set_objective(task, GOAL, gripper_cmd=g)
            got = eng.cost().cpu().numpy()
            np.testing.assert_array_equal(got.view(np.uint32), P.cost_obs(cfg, o).view(np.uint32), err_msg=task)
    finally:
        sim.stop_sim()


# ------------------------------------------------------------------ 8. reach in COMBINED: shadow slots and the cost kernel
def test_reach_cost_kernel_equals_the_shadow_slots_in_combined(P):
    from tests.panda_worlds import grasp_world
    K = X.K
    sc = X.oracle_scene(P, X.COMBINED)
    w0 = grasp_world(P, sc, close_gripper=False, lift=0.0)       # the open gripper around the cube, built in the scene
    delta = X.delta_of(K)
    cfg = P.make_cfg(K, X.T, multi_modal=False, task="reach", goal=GOAL, gripper_cmd=2)
    opl = P.OraclePandaPlanner(cfg, delta, sc)
    opl.command(w0)
    dflt = P.OraclePandaPlanner(cfg, delta, P.default_scene())
    dflt.command(w0)
    assert (opl.last["cost_h"] != dflt.last["cost_h"]).any(axis=1).mean() >= 0.8          # the scene shows in this world
    a = planner_engine(K, "reach", 2, X.COMBINED, lps=16, cost_kernel=True)
    b = planner_engine(K, "reach", 2, X.COMBINED, lps=0, cost_kernel=False)
    bufs = [L.BUF_TRAJ_COST, L.BUF_COST_HORIZON, L.BUF_STATES, L.BUF_ACTIONS, L.BUF_MEAN, L.BUF_WEIGHTS, L.BUF_TOP_TRAJS]
    try:
        for e in (a, b):
            e.set_world_panda_raw(P.raw57(w0))
        for call in range(3):
            pa, pb = a.command(sync_host=True), b.command(sync_host=True)
            assert a.panda_lanes_per_sample_used() == 16 and b.panda_lanes_per_sample_used() in (1, 8)
            assert a.panda_scene_instance_used() and b.panda_scene_instance_used()
            assert np.asarray(pa).tobytes() == np.asarray(pb).tobytes()
            for buf in bufs:
                assert torch.equal(a.buffer(buf), b.buffer(buf)), (call, buf)
            if call == 0:
                ref = {n: opl.last[n] for n in ("actions", "states", "cost_h", "J")}
                assert_rollout_equals_oracle(P, a, ref, "cost kernel")
                assert_rollout_equals_oracle(P, b, ref, "shadow slots")
        ch = a.cost_horizon.cpu().numpy()
        assert np.isfinite(ch).all() and ch.std() > 0
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------ 9. life cycle and refusals (nothing is launched)
def _bits(d):
    return bytes(L.panda_scene_fields(d))


def test_life_cycle_and_refusals(P):
    eng = planner_engine(X.K, "reach", 1)
    pt = HipEngine(make_config(K=64, T=10, nu=2, env_type="point_env"))
    try:
        lib, h = eng.lib, eng._h
        d = L.PandaSceneFields()
        lib.m3_default_panda_scene(C.byref(d))
        assert bytes(d) == _bits(None) and _bits(eng.panda_scene()) == _bits(None)
        eng.set_panda_scene(X.COMBINED)
        assert _bits(eng.panda_scene()) == _bits(X.COMBINED)                 # set / get round trip
        eng.reset()
        assert _bits(eng.panda_scene()) == _bits(X.COMBINED)                 # survives m3_reset
        # a refused value names its field and changes nothing
        for bad, msg in ((dict(mu=float("nan")), "m3_set_panda_scene: mu is not finite"),
                         (dict(table=(0.0, 0.0, 1.0, 0.6, 0.6, 0.0)), r"m3_set_panda_scene: table\[5\] must be > 0"),
                         (dict(cube_m=-1.0), "m3_set_panda_scene: cube_m must be > 0"),
                         (dict(mu=-0.1), "m3_set_panda_scene: mu must be >= 0"),
                         (dict(base=(0.0, float("inf"), 1.0)), r"m3_set_panda_scene: base\[1\] is not finite")):
            with pytest.raises(L.M3Error, match=msg):
                eng.set_panda_scene(bad)
            assert _bits(eng.panda_scene()) == _bits(X.COMBINED)
        assert lib.m3_set_panda_scene(h, None) == 0 and _bits(eng.panda_scene()) == _bits(None)     # NULL: the defaults
        eng.set_panda_scene(mu=0.0)                                          # frictionless is legal
        with pytest.raises(L.M3Error, match="-1 .*0 or 1"):
            eng.set_panda_scene_instance(2)
        # a point_env handle is refused
        with pytest.raises(L.M3Error, match="m3_set_panda_scene: panda_env only"):
            pt.set_panda_scene(mu=0.5)
        with pytest.raises(L.M3Error, match="panda_env only"):
            pt.set_panda_scene_instance(1)
        assert lib.m3_get_panda_scene(pt._h, C.byref(d)) != 0
        # forced off with a geometry scene: M3_ERR_STATE, nothing ran
        eng.set_panda_scene(X.PROBES["table_z"][0])
        eng.set_panda_scene_instance(0)
        eng.set_world_panda_raw(P.raw57(X.world_of(41)))
        calls = eng.info().calls
        for run in (eng.command, eng.rollout):
            with pytest.raises(L.M3Error, match="forced off .*m3_set_panda_scene"):
                run()
        assert eng.info().calls == calls
        eng.set_panda_scene(cube_m=0.4)                                      # the masses alone: nothing to refuse
        eng.command(sync_host=True)
        assert not eng.panda_scene_instance_used() and eng.info().calls == calls + 1
    finally:
        eng.close(); pt.close()


def test_batch_refuses_a_geometry_scene_and_then_works_without_it(P):
    engs = [planner_engine(X.K, "pick", 2) for _ in range(3)]
    batch = HipBatch(3)
    try:
        for e in engs:
            e.set_world_panda_raw(P.raw57(X.world_of(40)))
        batch.command(engs)
        torch.cuda.synchronize()
        engs[1].set_panda_scene(X.PROBES["table_z"][0])
        before = [e.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes() for e in engs]
        infos = [bytes(e.info()) for e in engs]
        with pytest.raises(L.M3Error, match="handle 1: .*m3_set_panda_scene") as ei:
            batch.command(engs)
        assert "m3p2i_hip error" in str(ei.value)
        torch.cuda.synchronize()
        assert [e.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes() for e in engs] == before
        assert [bytes(e.info()) for e in engs] == infos                      # nothing was launched
        engs[1].set_panda_scene_instance(0)                                  # forced off: refused too, for the other reason
        with pytest.raises(L.M3Error, match="handle 1: .*forced off"):
            batch.command(engs)
        batch.command([engs[0], engs[2]])                                    # the same batch without that handle
        torch.cuda.synchronize()
        assert engs[0].info().calls == 2 and engs[2].info().calls == 2 and engs[1].info().calls == 1
    finally:
        batch.close()
        for e in engs:
            e.close()


def test_panda_episodes_refuse_a_geometry_scene(P):
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    n = 2
    world = IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=n, device="cuda:0")
    planners = [planner_engine(X.K, "reach", 1) for _ in range(n)]
    try:
        for e in planners:
            e.set_action_out(torch.zeros(X.T, 9, device="cuda:0"))
        planners[1].set_panda_scene(X.PROBES["base"][0])
        with pytest.raises(L.M3Error, match="planner 1: .*m3_set_panda_scene"):
            HipPandaEpisodes(world._engine, planners, max_ticks=4)
        planners[1].set_panda_scene(None)
        world._engine.set_panda_scene(X.PROBES["mu"][0])
        with pytest.raises(L.M3Error, match="the world: .*m3_set_panda_scene"):
            HipPandaEpisodes(world._engine, planners, max_ticks=4)
        world._engine.set_panda_scene(obs_m=0.2)                            # the masses alone are welcome
        eps = HipPandaEpisodes(world._engine, planners, max_ticks=4)
        try:
            planners[0].set_panda_scene(X.PROBES["table_z"][0])              # set after create: the tick is refused, not run
            with pytest.raises(L.M3Error, match="planner 0: .*m3_set_panda_scene"):
                eps.observe()
        finally:
            eps.close()
    finally:
        world.stop_sim()
        for e in planners:
            e.close()


# ------------------------------------------------------------------ 10. Python end to end
def test_planner_follows_a_wrapper_built_from_actors(P):
    from m3p2i_aip_amd import scenes
    from tests.test_planner_api_panda_gpu import Tamp, make_cfg
    K, T = X.K, X.T
    goal = torch.tensor(list(X.GOAL))

    def actors(lower_table):
        acts = [scenes.Actor(**vars(a)) for a in scenes.PANDA_ENV]
        by = {a.name: a for a in acts}
        if lower_table:
            by["table"].init_pos = [0.0, 0.0, 0.99]
        by["cubeA"].init_pos = [0.2, -0.2, 1.04]          # the cubes resting on the lowered table
        by["cubeB"].init_pos = [0.2, 0.2, 1.04]
        return acts

    class TampA(Tamp):
        def __init__(self, cfg, acts):
            from m3p2i_aip_amd import isaacgym_wrapper as wrapper
            from m3p2i_aip_amd.cost_functions import Objective
            from m3p2i_aip_amd.planner import M3P2I
            self.sim = wrapper.IsaacGymWrapper(cfg.isaacgym, cfg.env_type, num_envs=cfg.mppi.num_samples, viewer=False,
                                               device=cfg.mppi.device, actors=acts)
            self.cfg, self.objective = cfg, Objective(cfg)
            self.motion_planner = M3P2I(cfg, dynamics=self.dynamics, running_cost=self.running_cost)

    outs = []
    for follow in (True, False):
        tamp = TampA(make_cfg(K, T, fused=None if follow else True), actors(lower_table=follow))
        pl = tamp.motion_planner
        assert (tamp.sim.panda_scene is not None) == follow
        if not follow:                                      # the same workspace set by hand on the planner's own engine
            pl.follow_sim_scene = False
            pl._engine.set_panda_scene(table=(0.0, 0.0, 0.99, 0.6, 0.6, 0.025))
        pl.set_noise(X.delta_of(K).copy())
        pl.update_gripper_command("reach")                  # (the reach cost moves with the gripper: the samples' costs differ)
        tamp.objective.update_objective("reach", goal)
        a = pl.command(tamp.sim._dof_state[0]).cpu().numpy()
        if follow:
            assert pl.probe_result["fused"] is True and pl.probe_result["max_abs_diff"] == 0.0      # the fused path is taken
            assert tamp.sim.panda_scene["table"][2] == float(F(0.99))
        assert pl._engine.panda_scene_instance_used()
        assert pl._engine.panda_scene()["table"][2] == float(F(0.99))
        outs.append((a, pl._engine.buffer(L.BUF_TRAJ_COST).cpu().numpy().copy()))
        tamp.sim.stop_sim()
    assert outs[0][0].tobytes() == outs[1][0].tobytes()
    assert outs[0][1].tobytes() == outs[1][1].tobytes() and np.ptp(outs[0][1]) > 0
