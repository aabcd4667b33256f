"""The run-time point_env arena against MECHANICS on the GPU: the closed forms of tests/arena_mechanics.py through the kernels that
take the arena at run time -- step mode with one arena per handle (k_sim_step_s) and one per row (k_sim_step_sv), the fused
rollout with one arena per handle (k_rollout_point<PointSceneRT>) and one per sample (k_rollout_point_sv).  Arenas, forms and
bounds are those of tests/test_arena_mechanics_cpu.py (tests/arena_mechanics_checks.py): the bounds were measured on the CPU oracle (never on a GPU result), and
the kernels equal the oracle bit for bit, so the GPU gets the same numbers.

Regression (spec v1.8): a box / dyn-obs without ground friction at rest against a wall -- NaN before -- in step mode and in a
fused push rollout whose costs and plan stay finite."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd import scenes  # noqa: E402
from m3p2i_aip_amd.engine import HipEngine, make_config  # noqa: E402
from tests import arena_mechanics as M  # noqa: E402
from tests import point_scene_fixture as X  # noqa: E402
from tests.arena_mechanics_checks import COUPLING, REPORTED, bounds_of, check, coupling_world, reported_world  # noqa: E402

F = np.float32
BOX_ACTOR, DYN_ACTOR = scenes.actor_index("point_env", "box"), scenes.actor_index("point_env", "dyn-obs")
BOX_BODY, ROBOT_BODY = scenes.body_index("point_env", "box", "box"), scenes.body_index("point_env", "point_robot", "link_y")
DEV = "cuda:0"


# ------------------------------------------------------------------ step mode
def step_mode(worlds, controls, steps, point_scene=None, point_scenes=None):
    """`steps` steps of the world rows (31 floats each) under their constant controls in a wrapper with one environment per
    row: trajectories [n, steps, 31] (float64; robot, box, dyn-obs and the robot's contact force filled in)"""
    from m3p2i_aip_amd import isaacgym_wrapper as wrapper
    w = np.asarray(worlds, F)
    n = len(w)
    cfg = wrapper.IsaacGymConfig(dt=M.DT, point_scene=dict(point_scene) if point_scene else None)
    sim = wrapper.IsaacGymWrapper(cfg, "point_env", num_envs=n, device=DEV, point_scenes=point_scenes)
    try:
        assert sim._engine.point_scene_rows_set() == (point_scenes is not None)
        dof = np.stack([w[:, 0], w[:, 4], w[:, 1], w[:, 5]], 1)
        sim._dof_state.copy_(torch.tensor(dof))
        root = sim._root_state.cpu().numpy()
        for actor, o in ((BOX_ACTOR, M.W_B), (DYN_ACTOR, M.W_D)):
            th = np.arctan2(w[:, o + 3].astype(np.float64), w[:, o + 2].astype(np.float64))
            root[:, actor, 0:2] = w[:, o:o + 2]
            root[:, actor, 3:7] = np.stack([0 * th, 0 * th, np.sin(th / 2), np.cos(th / 2)], 1)
            root[:, actor, 7:9] = w[:, o + 4:o + 6]
            root[:, actor, 9:12] = 0.0
            root[:, actor, 12] = w[:, o + 6]
        sim._root_state.copy_(torch.tensor(root))
        sim.set_dof_state_tensor(sim._dof_state)
        sim.set_actor_root_state_tensor(sim._root_state)
        if np.abs(w[:, M.W_FEXT_B:M.W_FEXT_B + 2]).sum() > 0:
            f = torch.zeros(n, sim.bodies_per_env, 3)
            f[:, BOX_BODY, 0:2] = torch.tensor(w[:, M.W_FEXT_B:M.W_FEXT_B + 2])
            sim.apply_rigid_body_force_tensors(f.to(DEV))
        u = torch.tensor(np.asarray(controls, F).reshape(n, 2), device=DEV)
        out = np.full((n, steps, M.ROW), np.nan)
        for t in range(steps):
            sim.set_dof_velocity_target_tensor(u)
            sim.step()
            torch.cuda.synchronize()
            dof, root = sim._dof_state.cpu().numpy(), sim._root_state.cpu().numpy()
            out[:, t, [0, 4, 1, 5]] = dof
            for actor, o in ((BOX_ACTOR, M.W_B), (DYN_ACTOR, M.W_D)):
                qz, qw = root[:, actor, 5].astype(np.float64), root[:, actor, 6].astype(np.float64)
                out[:, t, o:o + 2] = root[:, actor, 0:2]
                out[:, t, o + 2], out[:, t, o + 3] = 1.0 - 2.0 * qz * qz, 2.0 * qz * qw
                out[:, t, o + 4:o + 6] = root[:, actor, 7:9]
                out[:, t, o + 6] = root[:, actor, 12]
            out[:, t, M.W_FC_R:M.W_FC_R + 2] = sim._net_contact_force.cpu().numpy()[:, ROBOT_BODY, 0:2]
        return out
    finally:
        sim.stop_sim()


# the forms in wrappers of one to three environments, grouped by the fields they set on top of the arena
GROUPS = [["drive", "drive_limit", "push"], ["slide_box", "slide_dyn", "spin_box"], ["spin_dyn", "wall_x", "wall_y"], ["obs_x", "obs_y"],
          ["fext_box"], ["headon_x", "headon_y", "boxwall_x"], ["boxwall_y", "dynwall_x", "dynwall_y"]]


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "+".join(g))
@pytest.mark.parametrize("arena", list(M.ARENAS))
def test_step_mode_one_arena_per_handle(arena, group):
    forms = [M.FORMS[n] for n in group]
    assert len({tuple(sorted(f.overrides.items())) for f in forms}) == 1
    sd = X.scene_dict(forms[0].scene(M.ARENAS[arena]))
    trajs = step_mode([f.world(sd) for f in forms], [f.u for f in forms], max(f.steps for f in forms), point_scene=sd)
    for f, traj in zip(forms, trajs):
        check(f, sd, traj[:f.steps], f"step mode, arena {arena}")


@pytest.mark.parametrize("arena", list(M.ARENAS))
def test_step_mode_isolated_pair_conserves_momenta(arena):
    """as on the CPU: 12 oblique off-centre spinning hits and two head-on hits at 2 m/s, momenta formed with the arena's own
    masses and inertias conserved to 2e-4, energy never gained; three environments per wrapper"""
    sd = X.scene_dict({**M.ARENAS[arena], **M.NO_GROUND})
    worlds = list(M.pair_worlds(sd)) + [M.fast_headon_world(sd, 0), M.fast_headon_world(sd, 1)]
    hits = 0
    for i in range(0, len(worlds), 3):
        part = worlds[i:i + 3]
        for w0, traj in zip(part, step_mode(part, [(0.0, 0.0)] * len(part), 10, point_scene=sd)):
            p0, L0, E0 = M.momenta(sd, w0)
            E_prev = E0
            for row in traj:
                p, Lz, E = M.momenta(sd, row)
                np.testing.assert_allclose(p, p0, atol=2e-4)
                assert abs(Lz - L0) < 2e-4
                assert E <= E_prev * (1 + 1e-6)
                E_prev = E
            hits += E_prev < 0.98 * E0
    assert hits >= 12


@pytest.mark.parametrize("field", list(M.PAIR_ONLY))
def test_step_mode_robot_friction_acts_on_its_own_pair_only(field):
    """mu_rb / mu_rd (no steady closed form, see the CPU test): the robot pressed against the box and against the dyn-obs, in
    ARENA_A and with `field` varied: the other body's scene keeps its bits, the own body's scene changes"""
    sd = X.scene_dict(M.ARENA_A)
    varied = dict(sd)
    varied[field] = sd[field] * 1.5
    worlds = [M.press_world(sd, "box"), M.press_world(sd, "dyn")]
    t0 = step_mode(worlds, [M.U_PRESS] * 2, M.N_PRESS, point_scene=sd)
    t1 = step_mode(worlds, [M.U_PRESS] * 2, M.N_PRESS, point_scene=varied)
    own = ("box", "dyn").index(M.PAIR_ONLY[field])
    assert np.abs(t0[:, -1, M.W_FC_R:M.W_FC_R + 2]).sum(1).min() > 0
    assert abs(t0[own, -1, 5] - t1[own, -1, 5]) > 0.02
    np.testing.assert_array_equal(t0[1 - own], t1[1 - own])


N_ROWS = 65


@pytest.mark.parametrize("name", M.ROW_FORMS)
def test_step_mode_one_arena_per_row(name):
    """65 environments (a wavefront and one lane), row i in ROW_ARENAS[i % 5] -- its own robot_m, box_mu_g, box_m, wall, robot_r
    (the default arena among them, neighbours different) -- all rows running the same form at once, each held to the closed
    form of ITS arena.  A lane that read its neighbour's row fails: the smallest difference between neighbouring rows' expected
    values is 0.070 m/s for drive.v (bound 3e-6), 0.59 m/s for slide_box.v (2e-6), 0.026 m/s for push.v (1.9e-3) and 0.3 m for
    wall_x.rest (0.01): every bound is under a tenth of it (tests/test_arena_mechanics_cpu.py::
    test_tolerances_tell_neighbouring_rows_apart)."""
    form = M.FORMS[name]
    rows = [form.scene(M.ROW_ARENAS[i % len(M.ROW_ARENAS)]) for i in range(N_ROWS)]
    sds = [X.scene_dict(r) for r in rows]
    trajs = step_mode([form.world(sd) for sd in sds], [form.u] * N_ROWS, form.steps, point_scenes=rows)
    worst = {}
    for sd, traj in zip(sds, trajs):
        check(form, sd, traj, name, worst=worst)
    for q, (dev, lim) in sorted(worst.items()):
        print(f"{N_ROWS} rows, {name}.{q}: max |got - closed form| = {dev:.3g} (bound {lim:.3g})")


# ------------------------------------------------------------------ fused rollout
T_ROLL = 12


def rollout(K, world, controls, scene=None, rows=None, lanes=None):
    """robot trajectories [K, T, 31] (float64; only the robot's columns are filled) of a fused rollout from `world` in which
    sample k applies controls[k] at every step: the noise table is delta[k, t] = controls[k], the warm start zero, no filter,
    wide bounds.  (The last sample's noise is not used: it is the planner's noise-free sample, here the zero control.)"""
    delta = np.ascontiguousarray(np.repeat(np.asarray(controls, F)[:, None, :], T_ROLL, axis=1))
    delta[K - 1] = 0.0
    eng = HipEngine(make_config(K=K, T=T_ROLL, nu=2, filter_u=False, sample_null_action=False, u_min=[-100.0] * 2, u_max=[100.0] * 2,
                                noise_sigma_diag=[1.0, 1.0]))
    try:
        eng.set_objective("navigation", (1.0, 1.0))
        eng.set_noise(delta)
        if scene is not None:
            eng.set_point_scene(scene)
        if rows is not None:
            eng.set_point_rollout_scenes(rows)
            assert eng.point_rollout_scenes_set()
        if lanes is not None:
            eng.set_rollout_lanes(lanes)
        eng.set_world_point_raw(np.concatenate([np.asarray(world, F)[[0, 1, 4, 5]], np.asarray(world, F)[7:14], np.asarray(world, F)[14:21]]))
        eng.rollout()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(eng.actions.cpu().numpy(), delta)        # the controls are what was asked for
        states = eng.states.cpu().numpy().astype(np.float64)                  # [K, T, (x, vx, y, vy)]
    finally:
        eng.close()
    traj = np.full((K, T_ROLL, M.ROW), np.nan)
    traj[:, :, [0, 4, 1, 5]] = states
    return traj


def rollout_forms(k):
    """the robot-observable forms of sample k with its own control: drive response, steady-push speed, rest position and
    v_t = u_t - mu u_n at two walls and two obstacle faces"""
    forms = [M.drive_form("drive", M.sample_control("drive", k), 4), M.push_form("push", M.sample_control("push", k)[0], T_ROLL)]
    return forms + [M.rest_form(kind, *M.sample_control(kind, k)) for kind in M.REST_KINDS]


def check_rollout(K, arena_of, start_arena, only=None, **kw):
    """one rollout per form: sample k in arena_of(k) under its own control against its own closed form"""
    for j, proto in enumerate(rollout_forms(0)):
        if only is not None and proto.name not in only:
            continue
        forms = [rollout_forms(k)[j] for k in range(K)]
        world = proto.world(X.scene_dict(proto.scene(start_arena)))
        trajs = rollout(K, world, [f.u for f in forms], **kw)
        bad = []
        assert (trajs[K - 1][:, 4:6] == 0.0).all()          # (the noise-free sample stays where it is)
        for k, (f, traj) in enumerate(zip(forms[:K - 1], trajs)):
            sd = X.scene_dict(f.scene(arena_of(k)))
            want, got, tol = f.expected(sd), f.observed(traj, sd), bounds_of(f)
            for q in f.robot_only:
                w, g = np.asarray(want[q], np.float64), np.asarray(got[q], np.float64)
                if not (np.isfinite(g).all() and (np.abs(g - w) <= tol[q][1] + tol[q][0] * np.abs(w)).all()):
                    bad.append((k, f.name, q, g.tolist(), w.tolist()))
        assert not bad, bad[:5]


@pytest.mark.parametrize("K", [64, 100])
@pytest.mark.parametrize("arena", list(M.ARENAS))
def test_rollout_one_arena_per_handle(arena, K):
    check_rollout(K, lambda k: M.ARENAS[arena], M.ARENAS[arena], scene=M.ARENAS[arena])


# (the surfaces the robot meets are where they are in every sample's arena; along them the start leaves room in the arena
# with the smallest obstacle)
START_ARENA = M.sample_arena(7)


@pytest.mark.parametrize("K", [64, 100])
def test_rollout_one_arena_per_sample(K):
    """Sample k in sample_arena(k) under sample_control(., k), held to the closed forms of ITS arena.  What tells the samples
    apart: the drive response (robot_m), v_t = u_t - mu u_n (mu_rw, mu_ro) and the steady-push speed (box_m box_mu_g).  The
    REST POSITIONS do not: the samples share one start world, so sample_arena keeps wall - robot_r, obs - h - robot_r and
    robot_r + box_hx the same for every k (2.3 / -1.55 ...), and a lane that read another sample's wall or robot_r would still
    rest where it should -- the rest position per arena is what the one-arena-per-row step-mode test holds.  Sample K - 1 is the
    planner's noise-free sample: zero control, held to no arena-dependent form (it must stay where it is)."""
    check_rollout(K, M.sample_arena, START_ARENA, rows=[M.sample_arena(k) for k in range(K)])


@pytest.mark.parametrize("per_sample", [False, True], ids=["handle", "sample"])
def test_rollout_through_the_two_wave_build(per_sample):
    """K = 1025 with one sample per wavefront: the occ2 build; the drive form"""
    if per_sample:
        check_rollout(1025, M.sample_arena, START_ARENA, only=("drive",), rows=[M.sample_arena(k) for k in range(1025)], lanes=1)
    else:
        check_rollout(1025, lambda k: M.ARENA_A, M.ARENA_A, only=("drive",), scene=M.ARENA_A, lanes=1)


# ------------------------------------------------------------------ regression: ground friction 0 at rest against a wall
def _at_rest_and_finite(case, traj):
    b, ov, ax = REPORTED[case]
    sd = X.scene_dict(ov)
    cols = list(range(0, 2)) + list(range(4, 6)) + list(range(7, 21))
    assert np.isfinite(traj[:, cols]).all(), case
    o = M._body(b)
    assert abs(traj[-1, o + ax] - (sd["wall"] - sd[b + "_" + ("hx", "hy")[ax]])) < M.CONTACT_OFFSET
    assert np.abs(traj[-1, o + 4:o + 7]).max() < 1e-6


@pytest.mark.parametrize("case", list(REPORTED))
def test_step_mode_reported_scenes_stay_finite_and_at_rest(case):
    sd, w = reported_world(case)
    _at_rest_and_finite(case, step_mode([w], [(0.0, 0.0)], 200, point_scene=REPORTED[case][1])[0])


def test_step_mode_reported_scenes_as_rows():
    """the five reported scenes as the rows of one wrapper (k_sim_step_sv)"""
    cases = list(REPORTED)
    trajs = step_mode([reported_world(c)[1] for c in cases], [(0.0, 0.0)] * len(cases), 200, point_scenes=[REPORTED[c][1] for c in cases])
    for c, traj in zip(cases, trajs):
        _at_rest_and_finite(c, traj)


@pytest.mark.parametrize("per_sample", [False, True], ids=["handle", "sample"])
def test_push_rollout_with_a_frictionless_box_at_the_wall_stays_finite(per_sample):
    """K = 64, T = 30, task push, the arena of the report: the box, 5 cm from the +y wall at 0.3 m/s, meets it in the third step
    and is at rest -- through the subnormals -- long before the horizon ends; constant controls keep the robot away from it.
    Costs, weights and plan are finite."""
    K, T = 64, 30
    arena = REPORTED["box_+y"][1]
    sd = X.scene_dict(arena)
    w = M.parked(sd, robot=(-1.0, -1.0), box=(0.0, sd["wall"] - sd["box_hy"] - 0.05, 1, 0, 0, 0.3, 0), dyn=(-1.5, 1.5, 1, 0, 0, 0, 0))
    controls = np.array([M.sample_control("drive", k) for k in range(K)], F) * F(0.25)
    delta = np.ascontiguousarray(np.repeat(controls[:, None, :], T, axis=1))
    delta[K - 1] = 0.0                                   # (the planner's noise-free sample)
    eng = HipEngine(make_config(K=K, T=T, nu=2, filter_u=False, sample_null_action=False, u_min=[-3.0] * 2, u_max=[3.0] * 2,
                                noise_sigma_diag=[1.0, 1.0]))
    try:
        eng.set_objective("push", (1.0, 1.0))
        eng.set_noise(delta)
        if per_sample:
            eng.set_point_rollout_scenes([arena] * K)
        else:
            eng.set_point_scene(arena)
        wf = np.asarray(w, F)
        eng.set_world_point_raw(np.concatenate([wf[[0, 1, 4, 5]], wf[7:14], wf[14:21]]))
        plan = eng.command(sync_host=True)
        np.testing.assert_array_equal(eng.actions.cpu().numpy(), delta)
        for buf in (L.BUF_TRAJ_COST, L.BUF_COST_HORIZON, L.BUF_WEIGHTS, L.BUF_STATES, L.BUF_MEAN):
            assert torch.isfinite(eng.buffer(buf)).all(), buf
        assert np.isfinite(np.asarray(plan)).all()
    finally:
        eng.close()


# ------------------------------------------------------------------ regression: a coupling factor that underflows
@pytest.mark.parametrize("rows", [False, True], ids=["handle", "rows"])
@pytest.mark.parametrize("case", list(COUPLING))
def test_step_mode_coupling_factor_that_underflows_stays_finite(case, rows):
    """the scene of tests/test_arena_mechanics_cpu.py::test_a_coupling_factor_that_underflows_stays_finite (NaN after one step
    before spec v1.8; the floor at the coupling factor, not the derived constants', is what holds it) through k_sim_step_s
    and, as row 1 of three, k_sim_step_sv"""
    b, ov = COUPLING[case]
    sd, w = coupling_world(case)
    if rows:
        traj = step_mode([M.parked(X.scene_dict()), w, M.parked(X.scene_dict())], [(0.0, 0.0)] * 3, 4, point_scenes=[None, ov, None])[1]
    else:
        traj = step_mode([w], [(0.0, 0.0)], 4, point_scene=ov)[0]
    o = M._body(b)
    cols = [0, 1, 4, 5] + list(range(7, 21))
    assert np.isfinite(traj[:, cols]).all(), traj[0, o:o + 7]
    want = M.coulomb_spin(sd, b, 5.0, 4)
    np.testing.assert_allclose(traj[want > 0, o + 6], want[want > 0], rtol=1e-5)
    assert np.abs(traj[:, o:o + 2]).max() < 1e-12 and np.abs(traj[:, o + 4:o + 6]).max() < 1e-12


@pytest.mark.parametrize("per_sample", [False, True], ids=["handle", "sample"])
def test_push_rollout_coupling_factor_that_underflows_stays_finite(per_sample):
    """K = 64, T = 4, task push, the light spinning box with a slide of 2e-19 m/s left; the robot stays away: costs, weights and
    plan are finite (the box's words, and with them every push cost, were NaN from the first step before spec v1.8)"""
    K, T = 64, 4
    b, arena = COUPLING["box"]
    sd, w = coupling_world("box")
    controls = np.array([M.sample_control("drive", k) for k in range(K)], F) * F(0.25)
    delta = np.ascontiguousarray(np.repeat(controls[:, None, :], T, axis=1))
    delta[K - 1] = 0.0
    eng = HipEngine(make_config(K=K, T=T, nu=2, filter_u=False, sample_null_action=False, u_min=[-3.0] * 2, u_max=[3.0] * 2,
                                noise_sigma_diag=[1.0, 1.0]))
    try:
        eng.set_objective("push", (1.0, 1.0))
        eng.set_noise(delta)
        if per_sample:
            eng.set_point_rollout_scenes([arena] * K)
        else:
            eng.set_point_scene(arena)
        wf = np.asarray(w, F)
        eng.set_world_point_raw(np.concatenate([wf[[0, 1, 4, 5]], wf[7:14], wf[14:21]]))
        plan = eng.command(sync_host=True)
        np.testing.assert_array_equal(eng.actions.cpu().numpy(), delta)
        for buf in (L.BUF_TRAJ_COST, L.BUF_COST_HORIZON, L.BUF_WEIGHTS, L.BUF_STATES, L.BUF_MEAN):
            assert torch.isfinite(eng.buffer(buf)).all(), buf
        assert np.isfinite(np.asarray(plan)).all()
    finally:
        eng.close()
