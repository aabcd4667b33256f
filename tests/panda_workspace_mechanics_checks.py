"""Shared by tests/test_panda_workspace_mechanics_cpu.py and tests/test_panda_workspace_mechanics_gpu.py (a helper, not a test): the
measured bounds of the forms of tests/panda_workspace_mechanics.py, the comparison of a trajectory with a form's closed form,
and the loop that steps a form's world (whoever steps it)."""
import numpy as np

from tests import panda_workspace_mechanics as M

F = np.float32

# quantity: the largest |oracle - closed form| measured ON THE CPU ORACLE (never on the host build or a GPU result) over the
# default workspace, WS_A, WS_B, ROW_WS and the per-row parameters of row_form in the default workspace and WS_A (m, m/s; the
# slide's forces relative to the closed form's).  The bound is four times the measured value.  The slide's quantities are kept
# per regime -- `low` for mu <= 0.5, `high` above: the friction of the four corner rows pitches the cube forward, the more the
# closer mu comes to the tipping limit 1, and seven Gauss-Seidel sweeps leave the more of it.
# test_measured_table_is_the_oracles recomputes every entry.
MEASURED = {
    "rest_z": 2.2e-6,                  # top + cube_half after a drop of <= 0.2 m: bound 8.8e-6
    "rest_xy": 8.7e-6,                 # ... where it was released: bound 3.48e-5
    "impact_xy": 3.4e-5,               # ... after a landing faster than 2 m/s: bound 1.36e-4
    "edge_z": 8.2e-5,                  # ... of a cube with two corners over the shelf stand's edge: bound 3.28e-4
    "edge_xy": 4.8e-4,                 # bound 1.92e-3
    "slide_v.low": 1.7e-3,             # speed during the slide, after each step: bound 6.8e-3
    "slide_v.high": 3.6e-2,            # bound 1.44e-1
    "slide_x.low": 2.6e-4,             # position during the slide and at rest: bound 1.04e-3
    "slide_x.high": 2.9e-3,            # bound 1.16e-2
    "slide_force_t.low": 2.5e-3,       # (relative) mu cube_m g on the surface: bound 1e-2
    "slide_force_t.high": 3.0e-2,      # bound 1.2e-1
    "slide_force_n.low": 2.6e-4,       # (relative) -cube_m g: bound 1.04e-3
    "slide_force_n.high": 1.7e-2,      # bound 6.8e-2
    "slide_rest_z.low": 1.7e-5,        # top + cube_half at the end of the slide: bound 6.8e-5
    "slide_rest_z.high": 2.0e-4,       # bound 8e-4
    "slide_across.low": 6.1e-6,        # the coordinate across the slide at its end: bound 2.44e-5
    "slide_across.high": 4.1e-4,       # bound 1.64e-3
    "plate_onset.side": 3.1e-3,        # closest approach of the tip sphere to the plate's -x / -y face: bound 1.24e-2
    "plate_onset.top": 8.0e-5,         # ... to its top: bound 3.2e-4
}
RELATIVE = ("slide_force_t", "slide_force_n")
MARGIN = 4.0


def key_of(form, q, ws):
    """the measured table's entry of a form's quantity in a workspace"""
    key = form.measured[q]
    if key.startswith("slide_"):
        key += ".low" if ws["mu"] <= 0.5 else ".high"
    return key


def bounds_of(form, ws):
    """{quantity: (rtol, atol)}: the form's own, or four times the measured value"""
    out = dict(form.tol)
    for q in form.measured:
        if q in out:
            continue
        key = key_of(form, q, ws)
        out[q] = (MARGIN * MEASURED[key], 0.0) if key.split(".")[0] in RELATIVE else (0.0, MARGIN * MEASURED[key])
    return out


def deviations(form, ws, traj):
    """{quantity: (|got - closed form| per element, the bound per element, got, closed form)}"""
    want, got, tol = form.expected(ws), form.observed(traj, ws), bounds_of(form, ws)
    assert sorted(want) == sorted(got) and set(want) <= set(tol), (form.name, sorted(want), sorted(got), sorted(tol))
    out = {}
    for q in sorted(want):
        w, g = np.atleast_1d(np.asarray(want[q], np.float64)), np.atleast_1d(np.asarray(got[q], np.float64))
        rtol, atol = tol[q]
        out[q] = (np.abs(g - w), atol + rtol * np.abs(w), g, w)
    return out


def check(form, ws, traj, label, only=None, worst=None):
    """every quantity of the form (or `only` those) within its bound; prints each deviation beside its bound before asserting --
    or, with `worst` (a dict the caller prints once), keeps the largest deviation and its bound per quantity"""
    bad = []
    for q, (dev, lim, g, w) in deviations(form, ws, traj).items():
        if only is not None and q not in only:
            continue
        if worst is None:
            print(f"{label} {form.name}.{q}: max |got - closed form| = {dev.max():.3g} (bound {lim.max():.3g})")
        elif dev.max() >= worst.get(q, (-1.0, 0.0))[0]:
            worst[q] = (float(dev.max()), float(lim.max()))
        if not (np.isfinite(g).all() and (dev <= lim).all()):
            bad.append((q, g.tolist(), w.tolist()))
    assert not bad, (label, form.name, bad)


def trajectory(form, ws, load, step):
    """the world rows [steps, 84] (float64) of a form in the workspace `ws` (a full scene: form.scene(...)): load(row) -> the
    float32 row as a world load leaves it (grasp and sleep state inferred), step(row, u) -> the row one step later"""
    row = load(np.ascontiguousarray(form.world(ws), F))
    out = []
    for _ in range(form.steps):
        u = np.zeros(9, F) if form.control is None else np.asarray(form.control(ws, row.astype(np.float64)), F)
        row = step(row, u)
        out.append(row.astype(np.float64))
    return np.array(out)


def oracle_stepper(P, X, form, ws):
    """(load, step) of the CPU oracle in the workspace"""
    sc = X.oracle_scene(P, ws)
    sc.dt, sc.substeps = form.dt, form.substeps

    def load(row):
        return P.infer_state(sc, row)

    def step(row, u):
        w = np.ascontiguousarray(row[None])
        P.step_batch(sc, w, u[None])
        return w[0]

    return load, step


def measurement_cases():
    """(form, workspace) over which MEASURED holds"""
    cases = []
    spaces = list(M.WORKSPACES.values()) + [M.ROW_WS[1], M.ROW_WS[3]]
    for form in M.FORMS.values():
        if form.measured:
            cases += [(form, ws) for ws in spaces if form.applies(form.scene(ws))]
    for kind in M.ROW_FORMS:
        for i in range(8):
            cases += [(M.row_form(kind, i), ws) for ws in (M.DEFAULT, M.WS_A)]
    return cases


def measure(P, X):
    """{entry of MEASURED: the largest deviation on the CPU oracle}"""
    out = {}
    for form, ws in measurement_cases():
        sd = form.scene(ws)
        traj = trajectory(form, sd, *oracle_stepper(P, X, form, sd))
        for q, (dev, lim, g, w) in deviations(form, sd, traj).items():
            if q not in form.measured or q in form.tol:
                continue
            key = key_of(form, q, sd)
            d = float((dev / np.abs(w)).max()) if key.split(".")[0] in RELATIVE else float(dev.max())
            out[key] = max(out.get(key, 0.0), d)
    return out
