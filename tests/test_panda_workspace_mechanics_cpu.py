"""The run-time panda_env workspace (m3_set_panda_scene) against MECHANICS, without a GPU: every closed form of
tests/panda_workspace_mechanics.py in the default room and in two workspaces that break all of its coincidences, on the CPU
oracle, on the host build of panda_dyn.hpp through PandaSceneRT (step mode and the pick rollout's stepping) and, in the default
room, through the compile-time PandaScene.  The twin tests (tests/test_panda_scene_cpu.py) say that oracle and device source
agree bit for bit; these say that a field of the workspace means what its name says -- a half extent read as a full one, mu
missing from a friction row, the shelf's centre where the table's belongs would pass every twin test and fail here.

Tolerances: the project's own for what it already holds in the default room (tests/test_dynamics_physics.py: forward kinematics
3e-6, free fall 5e-6 / 1e-5 relative, the descent's 2 mm and torque ratio 1.02); contact_offset and rest_gap where the spec
promises no more (slide_into_shelf, landings faster than 2 m/s); everything else four times the CPU oracle's largest deviation
(tests/panda_workspace_mechanics_checks.py: MEASURED, recomputed here by test_measured_table_is_the_oracles).  Every test
prints each deviation beside its bound.

Not anchored by a closed form (panda_workspace_mechanics.UNANCHORED): obs_m -- held to "acts on the plate only" and to "a
heavier plate leaves the first contact slower" -- and the cube's inertia.  In the default room the shelf stand is beyond the
reach of a gripper pointing straight down (its near edge is 0.85 m from the base at the shoulder's height): descent_shelf and
side_shelf run in WS_A and WS_B only, and test_which_forms_the_arm_reaches holds that as a fact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import panda_scene_fixture as X
from tests import panda_workspace_mechanics as M
from tests import panda_workspace_mechanics_checks as K
from tests.native_flags import host_flags
from tests.test_device_dynamics_on_host import HOST_FLAGS, fma_flag
from tests.test_dynamics_physics import _point_jacobian

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
F = np.float32


@pytest.fixture(scope="module")
def P():
    import oracle.panda as P
    P.lib()
    return P


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """the host build of panda_dyn.hpp (tests/native/panda_scene_host.cpp), as tests/test_panda_scene_cpu.py builds it"""
    out = str(tmp_path_factory.mktemp("panda_workspace") / "libpanda_scene_host.so")
    subprocess.check_call(["g++"] + host_flags(HOST_FLAGS) + fma_flag() + ["-Wno-unknown-pragmas", "-I" + os.path.join(NATIVE, "shim"),
                           os.path.join(NATIVE, "panda_scene_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    VP = C.c_void_p
    lib.pss_step.argtypes = [VP, C.c_float, C.c_int, VP, C.c_int, VP, VP, C.c_int, VP, VP]
    lib.pss_infer_held.argtypes = [VP, C.c_float, C.c_int, VP, C.c_int, VP]
    lib.pss_fk.argtypes = [VP, VP, VP]
    return lib


# backend: (run-time scene, panda_step instance: 0 step mode, 1 the pick rollout's <FORCES, LAZY>)
HOST = {"host_rt_step": (True, 0), "host_rt_rollout": (True, 1), "host_ct_step": (False, 0)}
BACKENDS = ["oracle"] + list(HOST)


def stepper(backend, P, lib, form, ws):
    """(load, step) of tests/panda_workspace_mechanics_checks.trajectory in the workspace `ws` (a full scene)"""
    if backend == "oracle":
        return K.oracle_stepper(P, X, form, ws)
    rt, mode = HOST[backend]
    arr = X.flat21(ws)
    ptr = arr.ctypes.data if rt else None
    hp, trav, obs = np.zeros((1, 3), F), np.zeros(1, F), np.zeros((1, 10), F)

    def load(row):
        w = np.ascontiguousarray(row[None])
        lib.pss_infer_held(ptr, form.dt, form.substeps, w.ctypes.data, 1, hp.ctypes.data)
        return w[0]

    def step(row, u):
        w, uu = np.ascontiguousarray(row[None]), np.ascontiguousarray(u[None])
        lib.pss_step(ptr, form.dt, form.substeps, w.ctypes.data, 1, uu.ctypes.data, obs.ctypes.data, mode, hp.ctypes.data, trav.ctypes.data)
        return w[0]

    load.keep = step.keep = arr
    return load, step


def cases():
    out = []
    for name, form in M.FORMS.items():
        for wn, ws in M.WORKSPACES.items():
            if not form.applies(form.scene(ws)):
                continue
            for backend in BACKENDS:
                if backend == "host_ct_step" and (wn != "default" or form.overrides):
                    continue            # the compile-time scene is the default room
                out.append(pytest.param(name, wn, backend, id=f"{name}-{wn}-{backend}"))
    return out


@pytest.mark.parametrize("name,wn,backend", cases())
def test_closed_form(P, host_lib, name, wn, backend):
    form = M.FORMS[name]
    ws = form.scene(M.WORKSPACES[wn])
    traj = K.trajectory(form, ws, *stepper(backend, P, host_lib, form, ws))
    K.check(form, ws, traj, f"{backend} workspace {wn}")


@pytest.mark.parametrize("wn", list(M.WORKSPACES))
def test_forward_kinematics_stand_on_the_workspaces_base(P, host_lib, wn):
    """the oracle's and the host build's link poses against the textbook chain from the URDF numbers with the workspace's base
    (anchors base[0..2])"""
    ws = M.ws_full(M.WORKSPACES[wn])
    sc, arr = X.oracle_scene(P, ws), X.flat21(ws)
    worst = 0.0
    for q in M.fk_poses():
        want = M.fk_expected(ws, q.astype(np.float64))
        Lk = P.fk(sc, q)
        got = np.array([Lk["pos"][7], Lk["pos"][8], Lk["pos"][9], Lk["pos"][10], Lk["ay"][8], Lk["az"][8]], np.float64)
        worst = max(worst, np.abs(got - want).max())
        np.testing.assert_allclose(got, want, atol=M.FK_ATOL)
        out = np.zeros(77, F)
        host_lib.pss_fk(arr.ctypes.data, q.ctypes.data, out.ctypes.data)
        np.testing.assert_allclose(out.reshape(11, 7)[[7, 8, 9, 10], :3], want[:4], atol=M.FK_ATOL)
    print(f"workspace {wn} fk: max |got - chain| = {worst:.3g} (bound {M.FK_ATOL:.3g})")


def test_which_forms_the_arm_reaches(P):
    """the gripper pointing straight down reaches the table top and the plate in every workspace, the shelf stand's top and side
    in WS_A and WS_B -- and NOT in the default room; where it reaches, the oracle's kinematics put the hand where the binary64
    inverse kinematics say"""
    arm = ("descent_table", "descent_shelf", "side_shelf", "plate_face_x", "plate_face_y", "plate_face_z")
    for wn, ws in M.WORKSPACES.items():
        sc = X.oracle_scene(P, ws)
        for name in arm:
            form = M.FORMS[name]
            assert form.applies(form.scene(ws)) == (not (wn == "default" and name in ("descent_shelf", "side_shelf"))), (wn, name)
            if form.applies(form.scene(ws)):
                q = form.world(form.scene(ws))[:9]
                Lk = P.fk(sc, q.astype(F))
                assert np.abs(Lk["pos"][8] - M.chain(ws, q)["hand"]).max() < 1e-5 and Lk["az"][8][2] < -0.99999
    assert all(f.applies(f.scene(ws)) for f in M.FORMS.values() if f.name not in arm for ws in M.WORKSPACES.values())


@pytest.mark.parametrize("backend", ["oracle", "host_rt_step"])
@pytest.mark.parametrize("wn", ["A", "B"])
def test_a_cube_tips_when_mu_exceeds_one(P, host_lib, wn, backend):
    """the stated limit of the slide forms: with mu = 2.5 (> half width over half height = 1) a cube given 0.5 m/s on the table
    tips over its leading edge instead of sliding: the tilt's |q_w| leaves 0.999"""
    proto = M.FORMS["slide_table_x"]
    ws = {**M.ws_full(M.WORKSPACES[wn]), "mu": 2.5}
    w0 = proto.world(ws)
    w0[M.W_CUBEA + 7] = 0.5
    form = M.Form("tip", lambda ws: w0, 60, None, None, {}, [])
    traj = K.trajectory(form, ws, *stepper(backend, P, host_lib, form, ws))
    tilt = np.abs(traj[:, M.W_CUBEA + 6]).min()
    print(f"{backend} workspace {wn} mu 2.5: smallest |q_w| = {tilt:.4f} (flat: above 0.999)")
    assert np.isfinite(traj[:, :M.W_OBS + 3]).all() and tilt < 0.999


# ------------------------------------------------------------------ the descent's force: Newton's law per joint
@pytest.mark.parametrize("which", ["table", "shelf"])
@pytest.mark.parametrize("wn", list(M.WORKSPACES))
def test_descent_reports_the_effort_limited_force(P, wn, which):
    """tests/test_dynamics_physics.py::test_panda_descent_into_the_table_stops_and_reports_the_effort_limited_force with the
    workspace's top and base (one substep per step: the reported force is the step's): the tip reaches the top and stays within
    2 mm of it, and every reported force is explained by bounded drive torques, I dq' / h - J^T f = tau with |tau| <= effort
    (ratio < 1.02) on every joint that is not on a stop, one of them at its limit.  (The gripper leans by 0.1 rad so that one
    tip carries the contact: the reported force is then that contact's.)"""
    h = 0.005
    form = M.descent_form("descent", which, [], dt=h, substeps=1, lean=0.1)      # (leaning: one finger tip arrives first)
    ws = M.ws_full(M.WORKSPACES[wn])
    if not form.applies(ws):
        assert (wn, which) == ("default", "shelf")       # (beyond reach: test_which_forms_the_arm_reaches)
        return
    top = M.support(ws, which)[2]
    sc = X.oracle_scene(P, ws)
    sc.dt, sc.substeps = h, 1
    w = np.ascontiguousarray(P.infer_state(sc, np.ascontiguousarray(form.world(ws), F))[None])
    inertia, eff = np.array(sc.inertia), np.array(sc.effort)
    ft = P.W_FT if which == "table" else P.W_FS
    gaps, ratios, forces = [], [], []
    for t in range(70):
        q0, qd0 = w[0, :9].copy(), w[0, 9:18].copy()
        L = P.fk(sc, q0)
        u = form.control(ws, w[0].astype(np.float64)).astype(F)[None]
        tl, tr = L["pos"][9] + sc.tip_z * L["az"][8], L["pos"][10] + sc.tip_z * L["az"][8]
        P.step_batch(sc, w, u)
        n_grip = P.last_rows()[0]
        f = -w[0, ft:ft + 3].astype(np.float64)          # on the gripper
        gaps.append(M._tip_bottom(ws, w[0, :9]) - top)
        if n_grip == 1 and np.linalg.norm(f) > 0:
            s = 0 if tl[2] < tr[2] else 1
            J, _ = _point_jacobian(P, sc, q0, (tl if s == 0 else tr) - np.array([0, 0, sc.tip_r]))
            J[:, 7 + s] = (1 - 2 * s) * L["ay"][8]
            tau = inertia * (w[0, 9:18] - qd0) / h - J.T @ f
            free = w[0, 9:16] != 0.0                               # (a joint on a stop is held by the stop)
            ratios.append(np.abs(tau[:7][free] / eff[:7][free]).max())
            forces.append(f[2])
    first = next(i for i, g in enumerate(gaps) if g < 1e-3)
    print(f"workspace {wn} descent onto the {which}: arrives at step {first}, deepest {min(gaps):.3g} (bound -2e-3), "
          f"highest after {max(gaps[first:]):.3g} (bound 1e-3), torque ratio {max(ratios):.4f} (bound 1.02), force {max(forces):.1f} N")
    assert 15 < first < 40
    assert min(gaps) > -2e-3 and max(gaps[first:]) < 1e-3
    assert len(ratios) > 15 and max(ratios) < 1.02
    assert max(ratios[5:]) > 0.98
    assert 50 < max(forces) < 600


# ------------------------------------------------------------------ obs_m: no closed form; what it is held to
@pytest.mark.parametrize("backend", ["oracle", "host_rt_step"])
@pytest.mark.parametrize("wn", ["A", "B"])
def test_plate_mass_acts_on_the_plate_only(P, host_lib, wn, backend):
    """obs_m x 4 under the same sweep: every cube word keeps its bits; the gripper meets the plate at the same step, and the
    plate leaves that first contact step slower (the same drives deliver at most the same impulse, and dv = impulse / m)"""
    form = M.FORMS["plate_face_x"]
    ws = form.scene(M.WORKSPACES[wn])
    heavy = {**ws, "obs_m": 4.0 * ws["obs_m"]}
    a = K.trajectory(form, ws, *stepper(backend, P, host_lib, form, ws))
    b = K.trajectory(form, heavy, *stepper(backend, P, host_lib, form, heavy))
    cubes = slice(M.W_CUBEA, M.W_OBS)
    np.testing.assert_array_equal(a[:, cubes], b[:, cubes])
    ta, tb = (int(np.nonzero(t[:, M.W_OBS + 7] != 0.0)[0][0]) for t in (a, b))
    print(f"{backend} workspace {wn}: first contact at step {ta} / {tb}, the plate leaves it at {a[ta, M.W_OBS + 7]:.4f} m/s with obs_m, "
          f"{b[tb, M.W_OBS + 7]:.4f} m/s with 4 obs_m")
    assert ta == tb and 0.0 < b[tb, M.W_OBS + 7] < a[ta, M.W_OBS + 7]
    np.testing.assert_array_equal(a[:ta], b[:ta])           # nothing differs before they meet


# ------------------------------------------------------------------ the bounds and the coverage
def test_measured_table_is_the_oracles(P):
    """every entry of MEASURED is the CPU oracle's largest deviation over the workspaces, rounded up to two digits"""
    got = K.measure(P, X)
    assert sorted(got) == sorted(K.MEASURED)
    for key in sorted(got):
        print(f"{key}: measured {got[key]:.4g}, table {K.MEASURED[key]:.4g}, bound {K.MARGIN * K.MEASURED[key]:.4g}")
        assert got[key] <= K.MEASURED[key] <= 1.06 * got[key] + 1e-12, key


def _separation(form_a, ws_a, form_b, ws_b, bounds):
    """the largest |expected_a - expected_b| / bound over the quantities both have"""
    a, b, best = form_a.anchor(ws_a), form_b.anchor(ws_b), 0.0
    for q in a:
        if q not in b:
            continue
        x, y = np.atleast_1d(np.asarray(a[q], np.float64)), np.atleast_1d(np.asarray(b[q], np.float64))
        n = min(len(x), len(y))
        rtol, atol = bounds[q]
        lim = atol + rtol * np.abs(x[:n])
        if n and lim.max() > 0:
            best = max(best, float((np.abs(x[:n] - y[:n]) / np.where(lim > 0, lim, np.inf)).max()))
    return best


@pytest.mark.parametrize("kind,wn", [("fall_table", "default"), ("fall_table", "A"), ("slide_table_x", "A")])
def test_tolerances_tell_neighbouring_rows_apart(kind, wn):
    """the many-row GPU runs (65 rows): the expected values of neighbouring rows differ by at least ten bounds: a lane that read
    its neighbour's state fails.  (The slide runs in WS_A: with the default room's mu = 1 its bounds are the `high` regime's, a
    fifth of the difference between neighbours.)"""
    ws = M.ws_full(M.WORKSPACES[wn])
    worst = np.inf
    for i in range(64):
        f, g = M.row_form(kind, i), M.row_form(kind, i + 1)
        worst = min(worst, _separation(f, ws, g, ws, K.bounds_of(f, ws)))
    print(f"{kind} workspace {wn}: neighbouring rows differ by at least {worst:.3g} bounds")
    assert worst >= 10.0


@pytest.mark.parametrize("name", [n for n, f in M.FORMS.items() if f.fields])
def test_workspace_a_shows_in_every_form(name):
    """the share-style guard: each form's expected values in WS_A differ from the default room's by more than ten bounds, so a
    scene that reached nothing cannot pass"""
    form = M.FORMS[name]
    a = form.scene(M.WS_A)
    d = form.scene(M.DEFAULT)
    sep = _separation(form, a, form, d, K.bounds_of(form, a))
    print(f"{name}: WS_A and the default room differ by {sep:.3g} bounds")
    assert sep > 10.0


def _fails(P, name, closed_ws, given_ws):
    """whether the oracle in `given_ws` misses the closed form of `closed_ws`"""
    if name == "fk":
        sc = X.oracle_scene(P, given_ws)
        q = M.fk_poses(1)[0]
        return np.abs(P.fk(sc, q)["pos"][8] - M.fk_expected(closed_ws, q.astype(np.float64))[1]).max() > M.FK_ATOL
    form = M.FORMS[name]
    load, step = K.oracle_stepper(P, X, form, given_ws)
    try:
        K.check(form, closed_ws, K.trajectory(form, closed_ws, load, step), f"[{name} in a perturbed scene]")
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("field", M.FIELD_NAMES)
def test_every_field_is_anchored(P, field):
    """each of the 21 fields: with that field alone off by 10 % (up, and down) in the scene handed to the oracle, but not in the
    closed form, a form that names the field fails -- or the field is listed as unanchored, with its reason"""
    if field in M.UNANCHORED:
        assert field not in M.FIELD_FORMS and len(M.UNANCHORED[field]) > 20
        return
    names = M.FIELD_FORMS[field]
    closed = {name: M.ws_full(M.WS_A) if name == "fk" else M.FORMS[name].scene(M.WS_A) for name in names}
    assert not _fails(P, names[0], closed[names[0]], closed[names[0]])          # (the scene as it is passes)
    for factor in (1.1, 0.9):
        caught = [name for name in names if _fails(P, name, closed[name], M.perturbed(closed[name], field, factor))]
        print(f"{field} x {factor}: caught by {caught} of {names}")
        assert caught, (field, factor, names)


def test_field_list_is_the_structs():
    assert len(M.FIELD_NAMES) == 21 and M.DEFAULT == X.DEFAULTS
    assert set(M.FIELD_FORMS) | {"obs_m"} == set(M.FIELD_NAMES)
    np.testing.assert_array_equal(X.flat21(M.perturbed(M.DEFAULT, "shelf[4]", 2.0))[13], F(0.2))
