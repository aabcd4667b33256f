"""The run-time point_env arena against MECHANICS, without a GPU: every closed form of tests/arena_mechanics.py in two arenas that
break all the default arena's symmetries, on the CPU oracle and on the host build of the device header (planar_dyn.hpp through
PointSceneRT, step mode and the rollout's instance dispatch).  The oracle-twin tests (tests/test_point_scene_cpu.py) say that the
two implementations of the spec agree; these say that a field of the arena means what its name says -- and, run on both, whether
a failure is the spec's or the kernels'.

Tolerances: the project's own for the forms it already holds at the default arena (tests/test_dynamics_physics.py: drive rtol
2e-6, slide atol 2e-6, spin rtol 1e-5, pending force rtol 1e-6, steady push rtol 1e-3 / force 2e-3, momenta 2e-4); rest positions
within the spec's contact_offset (0.01).  For the new steady-state forms the bound is four times the CPU oracle's largest
deviation from the binary64 closed form in the arenas used (tests/arena_mechanics_checks.py, STEADY_TOL: measured value and bound side by side), and under a tenth
of what the nearest confusable field would change (test_steady_bounds_separate_the_confusable_fields).

Regression: a box / dyn-obs without ground friction that came to rest against a wall turned into NaN a few steps later (the
friction row's spec_rsqrt of a subnormal |impulse|^2 is not finite, and a limit of 0 selected it: 0 * inf); spec v1.8."""
import numpy as np
import pytest

import ctypes as C
import os
import subprocess

from tests import arena_mechanics as M
from tests import point_scene_fixture as X
from tests.arena_mechanics_checks import COUPLING, REPORTED, bounds_of, check, coupling_world, reported_world
from tests.native_flags import host_flags

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """the host build of planar_dyn.hpp through the run-time scene type (tests/native/point_scene_host.cpp)"""
    out = str(tmp_path_factory.mktemp("arena_mechanics") / "libpoint_scene_host.so")
    try:
        fma = ["-mfma"] if " fma " in open("/proc/cpuinfo").read() else []
    except OSError:
        fma = []
    flags = ["-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]
    subprocess.check_call(["g++"] + host_flags(flags) + fma + ["-I" + os.path.join(HERE, "native", "shim"),
                           os.path.join(HERE, "native", "point_scene_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.psh_step_rt.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    return lib


BACKENDS = ["oracle", "host_step", "host_rollout"]


def stepper(backend, O, lib, sd):
    """step(worlds [n, 31] float32, u [n, 2]) in arena `sd` (a full scene dict)"""
    if backend == "oracle":
        sc = X.oracle_scene(O, sd)
        return lambda w, u: O.step_batch(sc, w, u)
    arr = np.array([sd[n] for n in X.FIELDS], F)
    mode = 0 if backend == "host_step" else 1
    return lambda w, u: lib.psh_step_rt(arr.ctypes.data, M.DT, M.SUBSTEPS, 6, w.ctypes.data, len(w), u.ctypes.data, mode)


def run(step, world, u, steps):
    """trajectory [steps, 31] (float64) of one world under the constant control u"""
    w = np.ascontiguousarray(np.asarray(world, F)[None])
    uu = np.ascontiguousarray(np.asarray(u, F)[None])
    out = []
    for _ in range(steps):
        step(w, uu)
        out.append(w[0].astype(np.float64))
    return np.array(out)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("arena", list(M.ARENAS))
@pytest.mark.parametrize("name", list(M.FORMS))
def test_closed_form(oracle, host_lib, name, arena, backend):
    form = M.FORMS[name]
    sd = X.scene_dict(form.scene(M.ARENAS[arena]))
    if backend == "host_rollout" and name == "push":
        only = ("v", "v_box", "distance")        # (the rollout's instances form the dyn-obs' contact force only)
    else:
        only = None
    traj = run(stepper(backend, oracle, host_lib, sd), form.world(sd), form.u, form.steps)
    check(form, sd, traj, f"{backend} arena {arena}", only)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("arena", list(M.ARENAS))
def test_isolated_pair_conserves_momenta_and_never_gains_energy(oracle, host_lib, arena, backend):
    """no ground friction: linear momentum and angular momentum about the origin, formed with the arena's OWN box_m, box_I,
    dyn_m, dyn_I, are conserved through oblique off-centre spinning hits (2e-4) and energy never increases; the same for a
    head-on hit at 2 m/s along x and along y"""
    sd = X.scene_dict({**M.ARENAS[arena], **M.NO_GROUND})
    step = stepper(backend, oracle, host_lib, sd)
    worlds = list(M.pair_worlds(sd)) + [M.fast_headon_world(sd, 0), M.fast_headon_world(sd, 1)]
    hits, worst_p, worst_L = 0, 0.0, 0.0
    for w0 in worlds:
        p0, L0, E0 = M.momenta(sd, w0)
        E_prev = E0
        for row in run(step, w0, (0.0, 0.0), 10):
            p, L, E = M.momenta(sd, row)
            worst_p, worst_L = max(worst_p, np.abs(p - p0).max()), max(worst_L, abs(L - L0))
            np.testing.assert_allclose(p, p0, atol=2e-4)
            assert abs(L - L0) < 2e-4
            assert E <= E_prev * (1 + 1e-6)
            E_prev = E
        hits += E_prev < 0.98 * E0
    print(f"{backend} arena {arena}: momentum drift {worst_p:.3g}, angular momentum drift {worst_L:.3g}, {hits} of {len(worlds)} collide")
    assert hits >= 12


# ------------------------------------------------------------------ the bounds and the coverage
CONFUSABLE = [("wall_x", "mu_rw", "mu_ro"), ("wall_x", "mu_rw", "mu_rb"), ("obs_x", "mu_ro", "mu_rw"), ("obs_y", "mu_ro", "mu_rd"),
              ("headon_x", "box_hx", "box_hy"), ("headon_y", "dyn_hy", "dyn_hx"), ("headon_x", "box_m", "dyn_m"),
              ("boxwall_x", "box_hx", "box_hy"), ("dynwall_y", "dyn_hy", "dyn_hx"), ("boxwall_y", "box_hy", "dyn_hy"),
              ("spin_dyn", "dyn_req", "box_req"), ("spin_box", "box_I", "dyn_I"), ("slide_dyn", "dyn_mu_g", "box_mu_g"),
              ("push", "box_m", "dyn_m"), ("push", "box_hx", "box_hy")]


@pytest.mark.parametrize("name,field,other", CONFUSABLE)
@pytest.mark.parametrize("arena", list(M.ARENAS))
def test_steady_bounds_separate_the_confusable_fields(name, field, other, arena):
    """reading `other` where `field` belongs moves an expected value of the form by more than ten times its bound"""
    form = M.FORMS[name]
    sd = X.scene_dict(form.scene(M.ARENAS[arena]))
    swapped = dict(sd)
    swapped[field] = sd[other]
    a, b, tol = form.expected(sd), form.expected(swapped), bounds_of(form)
    ratio = max(float(np.max(np.abs(np.asarray(b[q], np.float64) - np.asarray(a[q], np.float64)) /
                             (tol[q][1] + tol[q][0] * np.abs(np.asarray(a[q], np.float64))))) for q in a)
    assert ratio > 10.0, (name, field, other, ratio)


@pytest.mark.parametrize("field", X.FIELDS)
def test_every_field_is_anchored_by_a_closed_form(field):
    """every field of POINT_SCENE_DEFAULTS but the five listed in arena_mechanics.UNANCHORED enters the expected value of a form
    the tests above run: varying it alone changes that value"""
    if field in M.UNANCHORED or field in M.PAIR_ONLY:      # (mu_rb, mu_rd: test_robot_friction_acts_on_its_own_pair_only)
        assert field not in M.FIELD_FORMS
        return
    assert M.FIELD_FORMS.get(field), field
    for arena in M.ARENAS.values():
        sd = X.scene_dict(arena)
        varied = dict(sd)
        varied[field] = sd[field] * 1.25 + 0.05
        for name in M.FIELD_FORMS[field]:
            if name == "pair":
                row = M.pair_worlds(sd)[0]
                row[M.W_D + 6] = 1.0        # (after a hit both bodies spin)
                a, b = np.hstack(M.momenta(sd, row)), np.hstack(M.momenta(varied, row))
            else:
                a, b = M.flat(M.FORMS[name].expected(sd)), M.flat(M.FORMS[name].expected(varied))
            assert (a != b).any(), (field, name)


def test_the_arenas_break_every_default_symmetry():
    for a in M.ARENAS.values():
        for k in ("m", "I", "req", "mu_g"):
            assert a["box_" + k] != a["dyn_" + k]
        assert a["box_hx"] != a["box_hy"] and a["dyn_hx"] != a["dyn_hy"]
        assert a["box_hx"] + a["dyn_hx"] != a["box_hy"] + a["dyn_hy"]
        assert len({a["mu_rw"], a["mu_ro"], a["mu_rb"], a["mu_rd"]}) == 4
        for k in ("robot_m", "robot_r", "wall", "obs_x", "obs_y", "obs_hx", "obs_hy"):
            assert a[k] != X.scene_dict()[k], k


def test_tolerances_tell_neighbouring_rows_apart():
    """the one-arena-per-row GPU test: for every form it runs and every pair of (cyclically) neighbouring ROW_ARENAS, a quantity
    whose expected values differ by more than ten times its bound -- a lane that read its neighbour's row fails.  Smallest
    difference / bound over the pairs: drive.v 0.070 m/s against 3e-6, slide_box.v 0.59 m/s against 2e-6, push.v 0.026 m/s
    against 1.9e-3, wall_x.rest 0.3 m against 0.01."""
    n = len(M.ROW_ARENAS)
    for name in M.ROW_FORMS:
        form = M.FORMS[name]
        tol = bounds_of(form)
        worst = None
        for i in range(n):
            a, b = (form.expected(X.scene_dict(form.scene(M.ROW_ARENAS[j]))) for j in (i, (i + 1) % n))
            best = max((float(np.max(np.abs(np.asarray(b[q], np.float64) - np.asarray(a[q], np.float64)))),
                        float(np.max(tol[q][1] + tol[q][0] * np.abs(np.asarray(a[q], np.float64)))), q) for q in a
                       if q in ("v", "rest"))
            worst = best if worst is None or best[0] / best[1] < worst[0] / worst[1] else worst
        print(f"{name}.{worst[2]}: smallest difference between neighbouring rows {worst[0]:.3g}, bound {worst[1]:.3g}")
        assert worst[0] > 10.0 * worst[1], (name, worst)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("field", list(M.PAIR_ONLY))
@pytest.mark.parametrize("arena", list(M.ARENAS))
def test_robot_friction_acts_on_its_own_pair_only(oracle, host_lib, arena, field, backend):
    """mu_rb / mu_rd have no steady closed form: the box (dyn-obs) the robot presses against a wall never comes to rest on the
    oracle (it creeps and turns at ~1e-2 m/s until the robot slides off).  The weaker statement: varying mu_rb changes the
    scene in which the robot slides along the BOX and leaves the one with the DYN-OBS bit-identical, and vice versa."""
    sd = X.scene_dict(M.ARENAS[arena])
    varied = dict(sd)
    varied[field] = sd[field] * 1.5
    for b in ("box", "dyn"):
        t0 = run(stepper(backend, oracle, host_lib, sd), M.press_world(sd, b), M.U_PRESS, M.N_PRESS)
        t1 = run(stepper(backend, oracle, host_lib, varied), M.press_world(sd, b), M.U_PRESS, M.N_PRESS)
        assert np.abs(t0[-1, 25:27]).sum() > 0 or backend == "host_rollout"     # (the robot is in contact)
        if b == M.PAIR_ONLY[field]:
            assert abs(t0[-1, 5] - t1[-1, 5]) > 0.02, (b, t0[-1, 5], t1[-1, 5])     # the robot's sliding speed feels it
        else:
            np.testing.assert_array_equal(t0, t1)


@pytest.mark.parametrize("backend", BACKENDS)
def test_steady_push_falls_short_for_a_heavy_box_on_a_light_robot(oracle, host_lib, backend):
    """A stated limit of the spec: the drive row is solved first in each of the six passes, the contact
    row after it, so the speed a substep ends with is the one the drive row saw minus the last pass's contact impulse / robot_m.
    Pair and force are right -- robot and box move together, the contact force is mu m g to 2e-3 -- but the common speed falls
    short of u - mu m g / D: by < 1e-3 of it up to box_m / robot_m = 2 (every arena of these tests), by 1 % at 24 kg on 6 kg.
    The passes' contact increments decrease, so the last is at most their mean: 0 <= shortfall <= mu m g h / (6 robot_m)."""
    arena = dict(M.ARENA_A, robot_m=6.0, box_m=24.0, box_I=24.0 * (0.6 ** 2 + 0.3 ** 2) / 12.0, box_mu_g=0.7)
    form = M.push_form("push", 2.08, 30)
    sd = X.scene_dict(arena)
    traj = run(stepper(backend, oracle, host_lib, sd), form.world(sd), form.u, form.steps)
    want, got = form.expected(sd), form.observed(traj, sd)
    shortfall = want["v"] - got["v"]
    print(f"{backend}: steady push at 24 kg on 6 kg: speed {got['v']:.6f} against {want['v']:.6f}, shortfall {shortfall:.3g}")
    assert -1e-3 * want["v"] <= shortfall <= -want["force"] * M.substep() / (6 * sd["robot_m"])
    assert shortfall > 5e-3                                    # (the limit is real: five times the steady-push bound)
    assert abs(got["v_box"] - got["v"]) < 1e-5 and abs(got["distance"] - want["distance"]) < M.CONTACT_OFFSET
    if backend != "host_rollout":
        np.testing.assert_allclose(got["force"], want["force"], rtol=2e-3)


def test_sample_arenas_hold_their_closed_forms_on_the_oracle(oracle):
    """the hundred (arena, control) pairs of the fused-rollout GPU tests, sample by sample on the oracle: drive, steady-push
    speed, rest position and v_t at both walls and both obstacle faces"""
    for k in range(100):
        arena = M.sample_arena(k)
        forms = [M.drive_form("drive", M.sample_control("drive", k), 4), M.push_form("push", M.sample_control("push", k)[0], 12)]
        forms += [M.rest_form(kind, *M.sample_control(kind, k)) for kind in M.REST_KINDS]
        for form in forms:
            sd = X.scene_dict(form.scene(arena))
            traj = run(stepper("oracle", oracle, None, sd), form.world(sd), form.u, form.steps)
            want, got, tol = form.expected(sd), form.observed(traj, sd), bounds_of(form)
            for q in form.robot_only:
                np.testing.assert_allclose(got[q], want[q], rtol=tol[q][0], atol=tol[q][1], err_msg=f"sample {k} {form.name}.{q}")


# ------------------------------------------------------------------ regression: ground friction 0 at rest against a wall
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["boxwall_x", "boxwall_y", "dynwall_x", "dynwall_y"])
@pytest.mark.parametrize("arena", list(M.ARENAS))
def test_frictionless_body_against_a_wall_stays_finite(oracle, host_lib, name, arena, backend):
    """200 steps: every state word finite (half of these eight scenes decay through the subnormals: NaN before spec v1.8)"""
    form = M.FORMS[name]
    sd = X.scene_dict(form.scene(M.ARENAS[arena]))
    traj = run(stepper(backend, oracle, host_lib, sd), form.world(sd), form.u, 200)
    bad = np.argwhere(~np.isfinite(traj[:, :25]))
    assert bad.size == 0, f"first non-finite word: step {bad[0][0]} column {bad[0][1]}"
    check(form, sd, traj, f"{backend} arena {arena}")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", list(REPORTED))
def test_the_reported_scenes_stay_finite_and_at_rest(oracle, host_lib, case, backend):
    """NaN in every word of the body at step 48 (49) before spec v1.8; now: finite for 200 steps, at wall - hx / wall - hy within
    contact_offset, at rest"""
    b, ov, ax = REPORTED[case]
    sd, w = reported_world(case)
    traj = run(stepper(backend, oracle, host_lib, sd), w, (0.0, 0.0), 200)
    assert np.isfinite(traj[:, :25]).all()
    o = M._body(b)
    h = sd[b + "_" + ("hx", "hy")[ax]]
    assert abs(traj[-1, o + ax] - (sd["wall"] - h)) < M.CONTACT_OFFSET
    assert np.abs(traj[-1, o + 4:o + 7]).max() < 1e-6


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", list(COUPLING))
def test_a_coupling_factor_that_underflows_stays_finite(oracle, host_lib, case, backend):
    """The floor where a substep applies the sliding-spinning coupling factor (the derived constants' floor does not reach it):
    a light box (dyn-obs) in the otherwise default arena, spinning at 5 rad/s with a slide of 2e-19 m/s left, zero control.  Its
    factor v / (v + 0.85 u) is ~1e-19, the limit's square underflows, mag2 = (m v)^2 is subnormal: NaN in every word of the
    body after ONE step before spec v1.8 (for every slide from 1.2e-19 to 5e-19 m/s), on the oracle and the device source.
    Now: finite, the spin decays by its torsion friction, the body stays where it is."""
    b, ov = COUPLING[case]
    sd, w = coupling_world(case)
    traj = run(stepper(backend, oracle, host_lib, sd), w, (0.0, 0.0), 4)
    o = M._body(b)
    assert np.isfinite(traj[:, :25]).all(), traj[0, o:o + 7]
    want = M.coulomb_spin(sd, b, 5.0, 4)
    assert want[0] > 0.5                                    # (it is still spinning after the first step)
    np.testing.assert_allclose(traj[want > 0, o + 6], want[want > 0], rtol=1e-5)
    assert np.abs(traj[want == 0, o + 6]).max() < 5.0 * 2.0 ** -22     # (stopped: 1 / I is a rounded reciprocal, the stopping row
    # leaves the spin times two binary32 roundings, as tests/test_dynamics_physics.py notes for the default arena)
    assert np.abs(traj[:, o:o + 2]).max() < 1e-12 and np.abs(traj[:, o + 4:o + 6]).max() < 1e-12
