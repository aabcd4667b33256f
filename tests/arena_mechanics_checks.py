"""Shared by tests/test_arena_mechanics_cpu.py and tests/test_arena_mechanics_gpu.py (a helper, not a test): the bounds of the
steady-state forms, the comparison of a trajectory with a form's closed form, and the worlds of the regression scenes."""
import numpy as np

from tests import arena_mechanics as M
from tests import point_scene_fixture as X

# quantity: (largest |oracle - closed form| measured on the CPU oracle, m or m/s) -- measured over ARENA_A, ARENA_B, ROW_ARENAS and
# the hundred sample_arena / sample_control pairs of the GPU rollouts (each in its own arena, in ARENA_A and in ARENA_B).  The
# bound is four times the measured value.
STEADY_MEASURED = {
    "headon.v": 7.78e-5,          # common velocity m_b v0 / (m_b + m_d): bound 3.112e-4
    "headon.distance": 4.7e-5,    # centre distance hx + hx / hy + hy: bound 1.88e-4
    "rest.v_t": 5.33e-5,          # v_t = u_t - mu u_n: bound 2.132e-4
    "rest.v_n": 3.65e-6,          # the robot does not move into the surface: bound 1.46e-5
}
STEADY_TOL = {k: (v, 4.0 * v) for k, v in STEADY_MEASURED.items()}


def bounds_of(form):
    """{quantity: (rtol, atol)} of a form: its own, or the measured steady-state bounds"""
    if form.tol is not None:
        return form.tol
    if form.name.startswith("headon"):
        return dict(v_box=(0.0, STEADY_TOL["headon.v"][1]), v_dyn=(0.0, STEADY_TOL["headon.v"][1]),
                    distance=(0.0, STEADY_TOL["headon.distance"][1]))
    return dict(rest=(0.0, M.CONTACT_OFFSET), v_t=(0.0, STEADY_TOL["rest.v_t"][1]), v_n=(0.0, STEADY_TOL["rest.v_n"][1]))


def check(form, sd, traj, label, only=None, worst=None):
    """every quantity of the form (or `only` those) within its bound; prints each deviation before asserting -- or, with
    `worst` (a dict the caller prints once), keeps the largest deviation and its bound per quantity"""
    want, got, tol = form.expected(sd), form.observed(traj, sd), bounds_of(form)
    bad = []
    for q in sorted(want):
        if only is not None and q not in only:
            continue
        w, g = np.asarray(want[q], np.float64), np.asarray(got[q], np.float64)
        rtol, atol = tol[q]
        dev, lim = np.abs(g - w), atol + rtol * np.abs(w)
        if worst is None:
            print(f"{label} {form.name}.{q}: max |got - closed form| = {dev.max():.3g} (bound {np.max(lim):.3g})")
        elif dev.max() >= worst.get(q, (-1.0, 0.0))[0]:
            worst[q] = (float(dev.max()), float(np.max(lim)))
        if not (np.isfinite(g).all() and (dev <= lim).all()):
            bad.append((q, g.tolist(), w.tolist()))
    assert not bad, (label, form.name, bad)


# the scenes of the report: the default arena with an oblong box (dyn-obs) without ground friction, 0.3 m/s into the +y / +x wall
REPORTED = {"box_+y": ("box", dict(box_hx=0.3, box_hy=0.15, box_mu_g=0.0), 1), "dyn_+y": ("dyn", dict(dyn_hx=0.3, dyn_hy=0.15, dyn_mu_g=0.0), 1),
            "box_+x": ("box", dict(box_hx=0.15, box_hy=0.3, box_mu_g=0.0), 0), "dyn_+x": ("dyn", dict(dyn_hx=0.15, dyn_hy=0.3, dyn_mu_g=0.0), 0),
            "box_+y_0.2x0.1": ("box", dict(box_hx=0.2, box_hy=0.1, box_mu_g=0.0), 1)}


def reported_world(case):
    b, ov, ax = REPORTED[case]
    sd = X.scene_dict(ov)
    pose = [0.0, 0.0, 1, 0, 0, 0, 0]
    pose[ax], pose[4 + ax] = 3.15, 0.3
    other = "dyn" if b == "box" else "box"
    return sd, M.parked(sd, robot=(-1.0, -1.0), **M._place(b, pose), **M._place(other, (-1.5, 1.5, 1, 0, 0, 0, 0)))


# a coupling factor that underflows: a light body in the otherwise default arena, spinning, with a slide of 2e-19 m/s left
COUPLING = {"box": ("box", dict(box_m=0.1, box_I=0.1 * 0.32 / 12.0)), "dyn": ("dyn", dict(dyn_m=0.1, dyn_I=0.1 * 0.32 / 12.0))}


def coupling_world(case):
    b, ov = COUPLING[case]
    sd = X.scene_dict(ov)
    return sd, M.parked(sd, **M._place(b, (0.0, 0.0, 1, 0, 2e-19, 0, 5.0)))
