"""One point_env arena per environment (m3_set_point_scene_rows) on the GPU: the step mode and the lockstep episodes of a world
whose rows carry different arenas, against the CPU oracle / the serial closed loop with the row's own arena, bit for bit.
Recipe and oracle results: tests/test_point_scene_rows_cpu.py (65 rows: two workgroups, the second with one live lane; arena
i % 3 of default / CUSTOM / CUSTOM_B; on the oracle alone every row differs from what the other two arenas give it).
The no-allocation guarantee of the step and tick paths is stated next to the allocation in m3_set_point_scene_rows."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipEngine, make_config  # noqa: E402
from tests import point_scene_fixture as X  # noqa: E402
from tests import test_point_scene_rows_cpu as R  # noqa: E402
from tests.test_batch_command_gpu import BOX_ACTOR, DYN_ACTOR, PK  # noqa: E402
from tests.test_point_scene_gpu import ARENA_EP  # noqa: E402

F = np.float32
N, STEPS = R.N, R.STEPS


def _f32(d):
    return {k: float(F(v)) for k, v in d.items()}


def _world(oracle, **kw):
    """a 65-env wrapper with the recipe's start worlds in its views"""
    from m3p2i_aip_amd import isaacgym_wrapper as wrapper
    sim = wrapper.IsaacGymWrapper(wrapper.IsaacGymConfig(dt=0.05, **kw.pop("cfg", {})), "point_env", num_envs=N, **kw)
    worlds = R.row_worlds(oracle)
    sim._dof_state[:, 0] = torch.tensor(worlds[:, 0]); sim._dof_state[:, 2] = torch.tensor(worlds[:, 1])
    sim._dof_state[:, 1] = 0.0; sim._dof_state[:, 3] = 0.0
    for actor, o in ((BOX_ACTOR, oracle.W_B), (DYN_ACTOR, oracle.W_D)):
        sim._root_state[:, actor, 0:2] = torch.tensor(worlds[:, o:o + 2])
        sim._root_state[:, actor, 3:7] = torch.tensor([0.0, 0.0, 0.0, 1.0])
        sim._root_state[:, actor, 7:13] = 0.0
    sim.set_dof_state_tensor(sim._dof_state)
    sim.set_actor_root_state_tensor(sim._root_state)
    return sim


def _step(sim, u):
    e = sim._engine
    ud = torch.tensor(u, device="cuda:0")
    e._ck(e.lib.m3_sim_step_with_target(e._h, ud.data_ptr()))
    torch.cuda.synchronize()


def _views(sim):
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in (sim._dof_state, sim._root_state, sim._rigid_body_state, sim._net_contact_force)]


# ------------------------------------------------------------------ step mode
def test_step_mode_with_an_arena_per_row_equals_the_oracle_row_by_row(oracle):
    own, a, b = R.oracle_rows(oracle)
    differs = (own[-1][:, R.COLS].view(np.uint32) != a[-1][:, R.COLS].view(np.uint32)).any(1) & \
              (own[-1][:, R.COLS].view(np.uint32) != b[-1][:, R.COLS].view(np.uint32)).any(1)
    assert differs.mean() >= 0.5
    rows = [R.ARENAS[k] for k in R.arena_of_row()]
    sim = _world(oracle, point_scenes=rows)
    try:
        assert sim._engine.point_scene_rows_set() and sim.point_scene is None and len(sim.point_scenes) == N
        obs_row = [x.name for x in sim.env_cfg].index("obs")
        root0 = sim._root_state.cpu().numpy()
        for i in range(N):      # row i shows arena i
            sd = X.scene_dict(rows[i])
            assert root0[i, obs_row, 0:2].tolist() == [float(F(sd["obs_x"])), float(F(sd["obs_y"]))], i
            assert sim._engine.point_scene_row(i) == _f32(sd), i
        u = R.row_actions()
        for t in range(STEPS):
            _step(sim, u[t])
            worlds = own[t]
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
            assert (root[:, obs_row] == root0[:, obs_row]).all()
    finally:
        sim.stop_sim()


def test_rows_of_one_arena_are_the_single_arena_path(oracle):
    single = _world(oracle, cfg=dict(point_scene=dict(X.CUSTOM)))
    rows = _world(oracle, point_scenes=[X.CUSTOM] * N)
    try:
        assert not single._engine.point_scene_rows_set() and rows._engine.point_scene_rows_set()
        assert _views(single) == _views(rows)       # (the wrapper writes the same poses either way)
        u = R.row_actions()
        for t in range(STEPS):
            _step(single, u[t])
            _step(rows, u[t])
        assert _views(single) == _views(rows)
        own = R.oracle_rows(oracle)[0]                # (and the steps did something)
        assert (single._dof_state.cpu().numpy()[:, [0, 2]] != R.row_worlds(oracle)[:, 0:2]).any() and own is not None
    finally:
        single.stop_sim()
        rows.stop_sim()


# ------------------------------------------------------------------ episodes
SC = "case2_halton_push_coll"
SMALL = ["mppi.num_samples=128", "mppi.horizon=12", "mppi.u_per_command=12"]
# around ARENA_EP (the obstacle between robot and box): obs_*, wall, mu_rb and box_m varied
ARENAS_EP = [None,
             ARENA_EP,
             "point_scene={obs_x: 0.1, obs_y: 1.0, obs_hx: 0.25, obs_hy: 0.15, wall: 3.2, mu_rb: 0.15, box_m: 8.0, box_I: 0.2133}",
             "point_scene={obs_x: -0.1, obs_y: 0.8, obs_hx: 0.35, obs_hy: 0.1, wall: 2.6, mu_rb: 0.6, box_m: 24.0, box_I: 0.64}"]


def _tools():
    import tests.test_episodes_gpu  # noqa: F401  (puts tools/ on the path)
    import band_stats
    import closed_loop
    return band_stats, closed_loop


def _episodes(extra_of):
    bs, _ = _tools()
    return [("config_point", bs.overrides(SC, "default") + SMALL + list(extra_of(i)), bs.jitter_of(SC, 1 + i))
            for i in range(len(ARENAS_EP))]


def test_episodes_with_an_arena_each_equal_the_serial_loop():
    """n = 4 episodes, four different arenas (episode 0: the reference's): every planner plans in its own, every world row is
    stepped in its own (k_episodes_post_sv) -- report and every trace row equal closed_loop.run's, bit for bit"""
    from m3p2i_aip_amd.episodes import run_point_episodes
    from tests.test_episodes_gpu import _same
    _, closed_loop = _tools()
    eps = _episodes(lambda i: [ARENAS_EP[i]] if ARENAS_EP[i] else [])
    serial = [closed_loop.run(cn, ov, ticks=16, jitter=j, trace=True) for cn, ov, j in eps]
    for i in range(4):          # the arenas are live: four different traces
        for k in range(i):
            assert serial[i]["trace"] != serial[k]["trace"], (i, k)
    reps = run_point_episodes(eps, max_ticks=16, trace=True)
    for r, s in zip(reps, serial):
        _same(r, s)


def test_model_mismatch_world_arena_differs_from_the_planners():
    """two episodes, one `point_scene`, two `world_point_scene`s: the planners keep the nominal arena, the world's rows carry
    the mismatched ones, and the episodes equal the serial loop bit for bit"""
    from m3p2i_aip_amd.episodes import build_set
    from tests.test_episodes_gpu import _same
    bs, closed_loop = _tools()
    # (robot_m: the world's velocity drive feels it from the first step, long before the robot reaches the box)
    worlds = ["world_point_scene={robot_m: 6.0, box_m: 24.0, box_I: 0.64, mu_rb: 0.15}",
              "world_point_scene={robot_m: 14.0, box_m: 10.0, box_I: 0.2667, box_mu_g: 0.5, wall: 2.8}"]
    eps = [("config_point", bs.overrides(SC, "default") + SMALL + [ARENA_EP, worlds[i]], bs.jitter_of(SC, 1 + i)) for i in range(2)]
    nominal = dict(obs_x=0.0, obs_y=0.9, obs_hx=0.3, obs_hy=0.1, wall=2.95, mu_rb=0.4)
    mism = [dict(nominal, robot_m=6.0, box_m=24.0, box_I=0.64, mu_rb=0.15),
            dict(nominal, robot_m=14.0, box_m=10.0, box_I=0.2667, box_mu_g=0.5, wall=2.8)]
    es = build_set(eps, max_ticks=16, trace=True)
    try:
        es.run()
        reps = es.reports()
        assert es.real._engine.point_scene_rows_set()
        for e, side in enumerate(es.sides):
            assert side.motion_planner._engine.point_scene() == _f32(X.scene_dict(nominal)), e
            assert side.sim._engine.point_scene() == _f32(X.scene_dict(nominal)), e
            assert es.real._engine.point_scene_row(e) == _f32(X.scene_dict(mism[e])), e
    finally:
        es.close()
    serial = [closed_loop.run(cn, ov, ticks=16, jitter=j, trace=True) for cn, ov, j in eps]
    for r, s in zip(reps, serial):
        _same(r, s)
    for (cn, ov, j), s in zip(eps, serial):             # the mismatch is live: the nominal world gives another trace
        assert closed_loop.run(cn, ov[:-1], ticks=16, jitter=j, trace=True)["trace"] != s["trace"]


def test_rows_changed_between_ticks():
    """4 ticks, other rows, 4 more ticks: a freshly built set on the same schedule gives the same bytes, and rows 4 to 7 of
    the trace differ from a run whose rows never changed"""
    from m3p2i_aip_amd.episodes import build_set
    eps = _episodes(lambda i: [ARENAS_EP[i]] if ARENAS_EP[i] else [])
    # (robot_m: the velocity drive feels it in the very next step, far from any contact)
    other = [dict(X.scene_dict(), robot_m=4.0 + i, box_m=30.0, box_I=0.8, mu_rb=0.05 + 0.1 * i, box_mu_g=1.2, wall=2.7 + 0.1 * i)
             for i in range(4)]

    def trace_of(change):
        es = build_set(eps, max_ticks=8, trace=True)
        try:
            es.start()
            for t in range(1, 8):
                if t == 4 and change:
                    es.real._engine.set_point_scene_rows(other)
                es.tick()
            st, tr = es.eps.status(with_trace=True)
            assert all(s["done_tick"] == 7 and not s["success"] for s in st)
            return np.asarray(tr, F).copy()
        finally:
            es.close()

    a, b, never = trace_of(True), trace_of(True), trace_of(False)
    assert a.tobytes() == b.tobytes()
    assert a[:4].tobytes() == never[:4].tobytes()       # the row of tick t is written before tick t's step
    assert a[4].tobytes() == never[4].tobytes()         # (the first step in the new rows shows in the row of tick 5)
    for e in range(4):
        assert a[5:8, e].tobytes() != never[5:8, e].tobytes(), e


# ------------------------------------------------------------------ round trip and refusals
def test_round_trip_and_refusals():
    lib = L.load()
    w = HipEngine(make_config(K=5, K_local=5, T=1, nu=2, sim_only=True, filter_u=False))
    rows = [None, X.CUSTOM, X.CUSTOM_B, dict(wall=2.0), None]
    default = _f32(L.POINT_SCENE_DEFAULTS)
    sc = L.PointSceneFields()

    def state():
        return (w.point_scene_rows_set(), w.point_scene(),
                [w.point_scene_row(i) for i in range(5)] if w.point_scene_rows_set() else None)

    try:
        assert lib.m3_point_scene_rows_set(w._h) == 0 and not w.point_scene_rows_set()        # a fresh handle
        assert lib.m3_get_point_scene_row(w._h, 0, C.byref(sc)) == -4                          # M3_ERR_STATE: no rows
        w.set_point_scene_rows(rows)
        assert w.point_scene_rows_set()
        for i, r in enumerate(rows):
            assert w.point_scene_row(i) == _f32(X.scene_dict(r)), i
        assert w.point_scene() == default                       # the single scene is what it was
        assert lib.m3_get_point_scene_row(w._h, 5, C.byref(sc)) == -1 and lib.m3_get_point_scene_row(w._h, -1, C.byref(sc)) == -1
        w.set_point_scene_rows(None)                             # NULL clears
        assert not w.point_scene_rows_set()
        w.set_point_scene_rows(rows)
        w.set_point_scene(X.CUSTOM)                              # the last call wins: m3_set_point_scene clears the rows
        assert not w.point_scene_rows_set() and w.point_scene() == _f32(X.scene_dict(X.CUSTOM))
        w.set_point_scene_rows(rows[::-1])                       # (the blocks of the first call are reused)
        assert w.point_scene_row(1) == _f32(X.scene_dict(dict(wall=2.0))) and w.point_scene()["wall"] == 1.5
        # ---- refusals: the rows and the scene stay what they were
        before = state()
        arr = (L.PointSceneFields * 5)(*[L.PointSceneFields(**X.scene_dict(r)) for r in rows])
        assert lib.m3_set_point_scene_rows(w._h, arr, 4) == -3 and lib.m3_set_point_scene_rows(w._h, arr, 6) == -3   # M3_ERR_SHAPE
        assert state() == before
        arr[2].box_m = float("nan")
        assert lib.m3_set_point_scene_rows(w._h, arr, 5) == -1                                                        # M3_ERR_BAD_ARG
        msg = lib.m3_last_error(w._h).decode()
        assert "row 2" in msg and "box_m" in msg, msg
        assert state() == before
        with pytest.raises(L.M3Error, match="row 3.*wall"):
            w.set_point_scene_rows([None, None, None, dict(wall=0.1), None])
        with pytest.raises(ValueError, match="row 1"):
            w.set_point_scene_rows([None, dict(nope=1.0), None, None, None])
        assert state() == before
    finally:
        w.close()
    p = HipEngine(make_config(K=64, T=12, nu=2, **PK))          # a planner handle: its rollouts share one model
    try:
        p.set_point_scene(wall=2.0)
        arr = (L.PointSceneFields * 64)(*[L.PointSceneFields(**X.scene_dict()) for _ in range(64)])
        assert lib.m3_set_point_scene_rows(p._h, arr, 64) == -4 and lib.m3_set_point_scene_rows(p._h, None, 64) == -4   # M3_ERR_STATE
        assert lib.m3_point_scene_rows_set(p._h) == 0 and p.point_scene() == _f32(X.scene_dict(dict(wall=2.0)))
    finally:
        p.close()
    q = HipEngine(make_config(K=64, T=12, nu=9, env_type="panda_env", u_min=[-2] * 9, u_max=[2] * 9, noise_sigma_diag=[1] * 9))
    try:
        arr = (L.PointSceneFields * 64)()
        assert lib.m3_set_point_scene_rows(q._h, arr, 64) == -5 and lib.m3_get_point_scene_row(q._h, 0, C.byref(sc)) == -5   # M3_ERR_UNSUPPORTED
    finally:
        q.close()


def test_the_forced_off_switch_refuses_the_step_of_a_handle_with_rows(oracle):
    sim = _world(oracle, point_scenes=[None] * N)       # rows of the default arena are rows all the same
    try:
        before = _views(sim)
        sim._engine.set_point_scene_instance(0)
        with pytest.raises(L.M3Error, match="forced off"):
            _step(sim, R.row_actions()[0])
        assert _views(sim) == before
        sim._engine.set_point_scene_instance(-1)
        _step(sim, R.row_actions()[0])
        assert _views(sim) != before
    finally:
        sim.stop_sim()
