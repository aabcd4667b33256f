"""Closed forms of rigid-body mechanics as functions of the panda_env WORKSPACE (a helper, not a test).

Written from mechanics, the names of the 21 fields of m3_panda_scene (include/m3p2i_hip.h) and the Panda world spec's fixed
constants (g, dt, substeps, cube_half, contact_offset, rest_gap, sleep_v, the URDF numbers) alone: binary64, no call into the
oracle or the library.  A FORM is a small scene -- a start world, a control law, a number of steps, in a workspace given as a
dict of _lib.PANDA_SCENE_DEFAULTS' keys -- with the numbers a rigid-body simulator must show in it: `expected(ws)` computes them
from the workspace, `observed(traj, ws)` reads the same quantities off a trajectory (the oracle's 84-float world rows after each
step, whoever stepped them; words a stepper does not carry are NaN).  tests/test_panda_workspace_mechanics_cpu.py runs them on the
CPU oracle and on the host builds of panda_dyn.hpp, tests/test_panda_workspace_mechanics_gpu.py on the kernels.  The default room
hides a mix-up of fields behind its coincidences (table centre 0, 0; hx == hy everywhere; mu == 1; the masses the cost was tuned
for); WS_A and WS_B break every one of them.

Which form anchors which field: FIELD_FORMS.  UNANCHORED names the quantities no form holds, with the reason.

Stated limits of the forms (asserted as facts by the CPU tests, not hidden):
  * the slide forms need mu < 1: a cube pushed sideways on a surface TIPS instead of sliding once mu exceeds half width over half
    height (1 for a cube); the default room's mu == 1 still slides.  test_a_cube_tips_when_mu_exceeds_one holds mu = 2.5.
  * slide_into_shelf: a cube makes contact with ONE static box, the nearer to its centre.  A frictionless cube that slides on
    the table into the shelf stand's side face therefore trades the table's support for the face's while it is nearer to the
    face: it ends at rest, asleep, about 1 mm inside the face and 1.5 mm into the table top (measured on the CPU oracle), which is
    why the form's bounds are contact_offset horizontally and rest_gap vertically and not the rest height's.

World row (oracle/panda.py): q9 qd9 | cubeA13 cubeB13 plate13 (pos3 quat4 xyzw, vel3, angvel3) | held | rel_p3 rel_q4 | awake2 |
f_table3 f_shelf3 f_cubeB3 | warm8."""
import functools

import numpy as np

from tests.test_dynamics_physics import PANDA_FINGER_Z, generic_chain

G, DT, SUBSTEPS = 9.8, 0.01, 2
CUBE_HALF, CONTACT_OFFSET, REST_GAP, SLEEP_V = 0.025, 0.01, 0.002, 0.02
TIP_Z, TIP_R = 0.045, 0.012                     # the finger tip's collision sphere: along the hand's z from the finger, radius
HAND_TO_TIP = PANDA_FINGER_Z + TIP_Z            # hand origin -> tip sphere centre (gripper pointing down: straight below it)
Q_PARK = (0.0, 0.0, 0.0, -2.0, 0.0, 1.8675, 0.0, 0.02, 0.02)      # panda.yaml's initial pose: the arm folded above its base
W_Q, W_QD, W_CUBEA, W_CUBEB, W_OBS, W_HELD, W_RELQ, W_AWAKE, W_FT, W_FS, ROW = 0, 9, 18, 31, 44, 57, 61, 65, 67, 70, 84

DEFAULT = dict(base=(-0.45, 0.0, 1.125), table=(0.0, 0.0, 1.0, 0.6, 0.6, 0.025), shelf=(0.5, 0.0, 1.175, 0.1, 0.1, 0.15),
               obs_half=(0.1, 0.1, 0.01), obs_m=0.8, cube_m=0.125, mu=1.0)
# Two workspaces that break every coincidence of the default room: table centre x != y != 0 and hx != hy; shelf hx != hy and
# its top (1.26 / 1.36) != 1.325; three distinct obs_half; obs_m != 0.8, cube_m != 0.125; mu in (0.2, 0.9); the base moved in all
# three coordinates.  The shelf stand still stands on the table top and the arm still reaches both tops (the CPU tests check
# that the inverse kinematics converge there).  A cube released 4 cm beyond a side of the shelf stand either has 5 cm of table
# under it or none within 4 cm.
WS_A = dict(base=(-0.40, 0.05, 1.10), table=(0.08, -0.07, 0.97, 0.5, 0.55, 0.03), shelf=(0.40, 0.09, 1.13, 0.09, 0.12, 0.13),
            obs_half=(0.23, 0.26, 0.04), obs_m=0.5, cube_m=0.2, mu=0.4)
WS_B = dict(base=(-0.48, -0.06, 1.15), table=(-0.06, 0.07, 1.02, 0.66, 0.5, 0.02), shelf=(0.38, -0.08, 1.2, 0.12, 0.08, 0.16),
            obs_half=(0.07, 0.13, 0.03), obs_m=1.6, cube_m=0.06, mu=0.7)
WORKSPACES = {"default": DEFAULT, "A": WS_A, "B": WS_B}
# five workspaces, the default among them, neighbours (cyclically) different in the table's top, mu and cube_m: what the measured
# bounds are taken over.  (A panda_env handle has ONE workspace -- there is no workspace per environment as the point arena has
# -- so the many-environment runs give every row its own parameter of the form instead: row_form below.)
ROW_WS = [DEFAULT,
          dict(DEFAULT, table=(0.0, 0.0, 0.9, 0.6, 0.6, 0.06), shelf=(0.5, 0.0, 1.11, 0.1, 0.1, 0.15), cube_m=0.4, mu=0.3),
          WS_A,
          dict(DEFAULT, table=(0.03, -0.02, 1.01, 0.55, 0.6, 0.045), shelf=(0.5, 0.0, 1.205, 0.1, 0.1, 0.15), cube_m=0.05, mu=0.85),
          WS_B]
# what no closed form holds, and why
UNANCHORED = {
    "obs_m": "no closed form holds within a bound one can justify: with one substep per step and the force on the plate formed as "
             "obs_m dv / h, the per-joint balance I dq' / h + J^T f = D (u - q') leaves residuals as large as J^T f itself on the "
             "CPU oracle (up to 38 N m against 10 N m: the drive rows and the contact rows of seven Gauss-Seidel sweeps do not "
             "converge on each other), and |tau| <= effort alone does not see the mass (20 N m of 87); held to 'acts on the plate "
             "only' and to 'a heavier plate leaves the first contact slower' (impulse = m dv)",
    "invI_cube": "derived from cube_m in make_panda_scene; the resting and sliding forms do not turn the cube (cube_inertia is not built)",
}


def ws_full(ws=None):
    return {**DEFAULT, **(ws or {})}


def substep(dt=DT, substeps=SUBSTEPS):
    return dt / substeps


def support(ws, which):
    """(cx, cy, top, hx, hy) of the table / the shelf stand"""
    b = ws[which]
    return b[0], b[1], b[2] + b[5], b[3], b[4]


# ------------------------------------------------------------------ the closed forms
def free_fall(z0, n_steps, v0=0.0, dt=DT, substeps=SUBSTEPS):
    """semi-implicit Euler, exactly: v -= g h; z += h v per substep.  (z, v) after each step, and the smallest z any substep
    STARTED from within each step"""
    h, z, v, out = substep(dt, substeps), float(z0), float(v0), []
    for _ in range(n_steps):
        lowest = z
        for _ in range(substeps):
            lowest = min(lowest, z)
            v -= G * h
            z += h * v
        out.append((z, v, lowest))
    return np.array(out)


def free_steps(z0, top, n_steps, **kw):
    """the number of leading steps in which no substep starts with the cube's bottom face within contact_offset (+ 0.5 mm) of
    `top`: until then nothing but gravity acts on it"""
    lowest = free_fall(z0, n_steps, **kw)[:, 2]
    near = np.nonzero(lowest - CUBE_HALF - top < CONTACT_OFFSET + 5e-4)[0]
    return int(near[0]) if len(near) else n_steps


def coulomb_slide(mu, v0, n_steps, dt=DT, substeps=SUBSTEPS):
    """a sliding body: v <- max(0, v - mu g h) per substep, put to rest below sleep_v (the spec's sleep rule acts before the
    substep's integration); x += h v.  (speed, distance) after each step"""
    h, v, x, out = substep(dt, substeps), float(v0), 0.0, []
    for _ in range(n_steps):
        for _ in range(substeps):
            v = max(0.0, v - mu * G * h)
            if v < SLEEP_V:
                v = 0.0
            x += h * v
        out.append((v, x))
    return np.array(out)


def chain(ws, q):
    return generic_chain(np.asarray(q, np.float64), base=ws["base"])


def tips(ws, q):
    """centres of the two finger tips' collision spheres, and the hand's z axis"""
    c = chain(ws, q)
    az = c["R"][:, 2]
    return c["left"] + TIP_Z * az, c["right"] + TIP_Z * az, az


def hand_jacobian(ws, q, eps=1e-6):
    """d hand origin / d q[:7], central differences of the binary64 chain"""
    q = np.asarray(q, np.float64)
    J = np.zeros((3, 7))
    for j in range(7):
        a, b = q.copy(), q.copy()
        a[j] += eps; b[j] -= eps
        J[:, j] = (chain(ws, a)["hand"] - chain(ws, b)["hand"]) / (2 * eps)
    return J


@functools.lru_cache(maxsize=None)
def _ik_down_cached(base, target, lean):
    ws = dict(base=base)
    q = np.array([0, 0.3, 0, -2.2, 0, 2.5, 0.785, 0.04, 0.04], np.float64)
    lo = np.array([-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973]) + 0.02
    hi = np.array([2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973]) - 0.02

    def feat(q):
        c = chain(ws, q)
        return np.concatenate([c["hand"], 0.3 * c["R"][2, :]])       # the vertical components of the hand's axes

    want = np.concatenate([target, [0.0, -0.3 * np.sin(lean), -0.3 * np.cos(lean)]])
    for _ in range(400):
        f0 = feat(q)
        e = want - f0
        if np.linalg.norm(e) < 1e-7:
            return tuple(q)
        Jm = np.zeros((6, 7))
        for j in range(7):
            dq = q.copy(); dq[j] += 1e-6
            Jm[:, j] = (feat(dq) - f0) / 1e-6
        step = Jm.T @ np.linalg.solve(Jm @ Jm.T + 1e-6 * np.eye(6), e)
        q[:7] = np.clip(q[:7] + np.clip(step, -0.2, 0.2), lo, hi)
    raise AssertionError(f"the arm at {base} does not reach {target} pointing down")


def ik_down(ws, target, lean=0.0):
    """joint values that put the hand's origin at `target`, the gripper pointing straight down -- or leaning by `lean` radians
    about the hand's x, which brings the +y finger's tip lower than the other's (damped least squares on the
    binary64 chain, the yaw about the vertical left free: the wrist's limit does not allow every one; raises if the arm does not
    reach)"""
    return np.array(_ik_down_cached(tuple(float(x) for x in ws["base"]), tuple(float(x) for x in target), float(lean)))


# ------------------------------------------------------------------ worlds
def parked(ws, cubeA=None, vA=(0.0, 0.0, 0.0), q=None, plate=None):
    """a world row with everything a form does not use out of the way: the arm folded above its base, cubeB at rest in the
    table's (-x, +y) corner, cubeA at rest in its (+x, -y) corner (or at `cubeA`, moving at `vA`), the plate floating 0.9 m
    above the table's (+x, +y) quarter (or at `plate`)"""
    tx, ty, top, hx, hy = support(ws, "table")
    w = np.zeros(ROW)
    w[W_Q:W_Q + 9] = Q_PARK if q is None else q
    w[W_CUBEA:W_CUBEA + 3] = (tx + hx - 0.08, ty - hy + 0.08, top + CUBE_HALF) if cubeA is None else cubeA
    w[W_CUBEA + 7:W_CUBEA + 10] = vA
    w[W_CUBEB:W_CUBEB + 3] = (tx - hx + 0.08, ty + hy - 0.08, top + CUBE_HALF)
    w[W_OBS:W_OBS + 3] = (tx + 0.5 * hx, ty + 0.5 * hy, top + 0.9) if plate is None else plate
    for b in (W_CUBEA, W_CUBEB, W_OBS):
        w[b + 6] = 1.0
    w[W_RELQ + 3] = 1.0
    w[W_AWAKE:W_AWAKE + 2] = 1.0
    return w


class Form:
    """name; world(ws) -> row; control(ws, row) -> u[9] (None: zero); steps; expected(ws) / observed(traj, ws) -> {quantity:
    value}; tol {quantity: (rtol, atol)}, quantities missing from it take their bound from the measured table
    (tests/panda_workspace_mechanics_checks.py) under the name measured[quantity]; fields: the workspace's fields (by name and
    index) the expected values depend on; anchor(ws): where the expected values themselves are the same in every workspace (the
    gripper stops AT a surface: gap 0), the surface's place by the name of the quantity whose bound holds it; applies(ws): whether the form can be set up in the workspace (the arm reaches); overrides: fields the form sets on top of the workspace (a dict, or a function of the
    workspace); dt, substeps"""

    def __init__(self, name, world, steps, expected, observed, tol, fields, control=None, overrides=None, measured=None,
                 dt=DT, substeps=SUBSTEPS, applies=None, anchor=None):
        self.name, self.world, self.steps, self.expected, self.observed = name, world, steps, expected, observed
        self.tol, self.fields, self.control, self.overrides = dict(tol), tuple(fields), control, overrides or {}
        self.measured, self.dt, self.substeps = dict(measured or {}), dt, substeps
        self.applies = applies or (lambda ws: True)
        self.anchor = anchor or expected

    def scene(self, ws):
        full = ws_full(ws)
        return {**full, **(self.overrides(full) if callable(self.overrides) else self.overrides)}


FORMS = {}


def _add(form):
    assert form.name not in FORMS
    FORMS[form.name] = form
    return form


def _asleep(traj, t=-1):
    return float(traj[t, W_AWAKE] == 0.0 and np.all(traj[t, W_CUBEA + 7:W_CUBEA + 13] == 0.0))


def _flat(traj, t=-1, level=0.9999):
    return float(abs(traj[t, W_CUBEA + 6]) > level)          # |q_w|: turned about z at the most


# ---- a cube released above the table / the shelf stand
RELEASE, N_DROP, INSIDE, OUTSIDE, EDGE = 0.2, 60, CUBE_HALF + 0.015, 0.04, 0.008
EXACT = dict(z_free=(0.0, 5e-6), v_free=(1e-5, 0.0))       # tests/test_dynamics_physics.py: free fall
BOOL = (0.0, 0.0)


def _landing(ws, x, y):
    """what a cube falling at (x, y) beside the shelf stand meets: the table's top, or None when it has none within OUTSIDE"""
    tx, ty, top, hx, hy = support(ws, "table")
    inside = min(hx - abs(x - tx), hy - abs(y - ty))
    assert inside >= OUTSIDE or inside <= -OUTSIDE + 1e-6, ("a landing point on the table's edge", x, y, inside)
    return top if inside >= OUTSIDE else None


def drop_form(name, which, side=None, inside=True, release=RELEASE, steps=N_DROP, fields=(), overrides=None, at=(0.0, 0.0)):
    """cubeA released `release` above the top of `which`: over its centre + `at` (in half extents), or at `side` ('-x', '+x', '-y', '+y') with
    its centre INSIDE within the edge / OUTSIDE beyond it / (inside == "edge") EDGE within it: two of its corners hang over the
    edge, its centre of mass does not, and it stays"""
    def place(ws):
        cx, cy, top, hx, hy = support(ws, which)
        x, y = cx + at[0] * hx, cy + at[1] * hy
        if side is not None and which == "table":      # along the table's edge: clear of the shelf stand
            x, y = (cx, cy - 0.7 * hy) if side[1] == "x" else (cx - 0.3 * hx, cy)
        if side is not None:
            d = -(EDGE if inside == "edge" else INSIDE) if inside else OUTSIDE
            s = -1.0 if side[0] == "-" else 1.0
            if side[1] == "x":
                x = cx + s * (hx + d)
            else:
                y = cy + s * (hy + d)
        return x, y, top + CUBE_HALF + release, top

    def lands_on(ws):
        x, y, z0, top = place(ws)
        if side is None or inside:
            return top
        return None if which == "table" else _landing(ws, x, y)

    def world(ws):
        x, y, z0, _ = place(ws)
        return parked(ws, cubeA=(x, y, z0))

    def expected(ws):
        x, y, z0, _ = place(ws)
        top = lands_on(ws)
        n = steps if top is None else free_steps(z0, top, steps)
        f = free_fall(z0, n)
        out = dict(z_free=f[:, 0], v_free=f[:, 1], xy=np.array([x, y]))
        if top is not None:
            out.update(rest_z=top + CUBE_HALF, asleep=1.0, flat=1.0)
        return out

    def observed(traj, ws):
        x, y, z0, _ = place(ws)
        top = lands_on(ws)
        n = steps if top is None else free_steps(z0, top, steps)
        out = dict(z_free=traj[:n, W_CUBEA + 2], v_free=traj[:n, W_CUBEA + 9], xy=traj[-1, W_CUBEA:W_CUBEA + 2])
        if top is not None:
            out.update(rest_z=traj[-1, W_CUBEA + 2], asleep=_asleep(traj), flat=_flat(traj))
        return out

    # a cube that meets a surface faster than contact_offset / h = 2 m/s (a drop of more than 0.2 m) enters it before a contact
    # is made; the contacts then push it out at baumgarte (depth - slop) / h and it falls asleep once that is below sleep_v:
    # up to slop + sleep_v h / baumgarte = 1.5 mm deep.  Such a landing is held to rest_gap, not to the rest height's bound.
    hard = release > RELEASE or (side is not None and not inside)
    tol = dict(EXACT, asleep=BOOL, flat=BOOL, **(dict(rest_z=(0.0, REST_GAP)) if hard else {}))
    return Form(name, world, steps, expected, observed, tol, fields, overrides=overrides,
                measured=dict(rest_z="edge_z", xy="edge_xy") if inside == "edge" else
                dict(rest_z="rest_z", xy="impact_xy" if hard else "rest_xy"))


_add(drop_form("fall_table", "table", fields=["table[2]", "table[5]"], at=(0.4, -0.4)))
_add(drop_form("fall_shelf", "shelf", fields=["shelf[2]", "shelf[5]"]))
THIN = 1e-3


def _thin_overrides(ws):
    t = ws["table"]
    return dict(table=(t[0], t[1], t[2] + t[5] - THIN, t[3], t[4], THIN))      # (the same top, 2 mm of table under it)


_add(drop_form("thin_table", "table", release=0.8, steps=80, fields=["table[5]"], at=(0.4, -0.4), overrides=_thin_overrides))
for _which in ("table", "shelf"):
    for _side in ("-x", "+x", "-y", "+y"):
        _ax = 0 if _side[1] == "x" else 1
        _flds = [f"{_which}[{_ax}]", f"{_which}[{3 + _ax}]"]
        _add(drop_form(f"footprint_{_which}_{_side}_in", _which, _side, True, fields=_flds))
        _add(drop_form(f"footprint_{_which}_{_side}_out", _which, _side, False, fields=_flds))
        if _which == "shelf":       # (a tenth of the shelf stand's half extents is a centimetre: less than INSIDE)
            _add(drop_form(f"footprint_{_which}_{_side}_edge", _which, _side, "edge", fields=_flds))

# ---- a resting cube given v0 along x / y: Coulomb friction.  NEEDS mu < 1 (see the module docstring; the default's mu == 1
# still slides).  v0 = mu g * 0.15 s: a slide of 15 steps and 0.11 mu metres, which fits on the smallest shelf stand.
N_SLIDE, N_SLIDE_REST = 15, 8


def slide_form(name, which, ax, n_slide=N_SLIDE, fields=("mu", "cube_m")):
    n = n_slide + N_SLIDE_REST

    def v0(ws):
        return ws["mu"] * G * n_slide * DT

    def start(ws):
        cx, cy, top, hx, hy = support(ws, which)
        p = [cx, cy, top + CUBE_HALF]
        if which == "table":            # a quarter of the table away from the shelf stand, the parked cubes and the arm's hand
            p[0], p[1] = cx - 0.1 * hx, cy - 0.45 * hy
        else:
            p[ax] = (cx, cy)[ax] - (hx, hy)[ax] + CUBE_HALF + 0.005
        return p

    def world(ws):
        v = [0.0, 0.0, 0.0]
        v[ax] = v0(ws)
        return parked(ws, cubeA=start(ws), vA=v)

    def sliding(ws):
        s = coulomb_slide(ws["mu"], v0(ws), n)
        return s, np.nonzero(s[:, 0] > 0.0)[0]           # the steps whose last substep still slides: the force it reports

    def expected(ws):
        s, on = sliding(ws)
        assert len(on) >= n_slide - 2
        f_t, f_n = ws["mu"] * ws["cube_m"] * G, -ws["cube_m"] * G
        return dict(v=s[:, 0], x=start(ws)[ax] + s[:, 1], force_t=np.full(len(on), f_t), force_n=np.full(len(on), f_n),
                    rest_z=start(ws)[2], asleep=1.0, flat=1.0, across=start(ws)[1 - ax])

    def observed(traj, ws):
        _, on = sliding(ws)
        ft = W_FT if which == "table" else W_FS
        return dict(v=traj[:, W_CUBEA + 7 + ax], x=traj[:, W_CUBEA + ax], force_t=traj[on, ft + ax], force_n=traj[on, ft + 2],
                    rest_z=traj[-1, W_CUBEA + 2], asleep=_asleep(traj), flat=_flat(traj, level=0.999), across=traj[-1, W_CUBEA + 1 - ax])

    return Form(name, world, n, expected, observed, dict(asleep=BOOL, flat=BOOL), list(fields),
                measured=dict(v="slide_v", x="slide_x", force_t="slide_force_t", force_n="slide_force_n", rest_z="slide_rest_z",
                              across="slide_across"))


for _which in ("table", "shelf"):
    for _ax in (0, 1):
        _add(slide_form(f"slide_{_which}_{'xy'[_ax]}", _which, _ax))

# ---- mu = 0: a cube at 0.2 m/s on the table with nothing in its way keeps its speed
V_FRICTIONLESS, N_FRICTIONLESS = 0.2, 100


def _frictionless_start(ws):
    tx, ty, top, hx, hy = support(ws, "table")
    return (tx - 0.25, ty - 0.25, top + CUBE_HALF)


_add(Form("frictionless", lambda ws: parked(ws, cubeA=_frictionless_start(ws), vA=(V_FRICTIONLESS, 0.0, 0.0)), N_FRICTIONLESS,
          expected=lambda ws: dict(v=np.full(N_FRICTIONLESS, V_FRICTIONLESS), z=np.full(N_FRICTIONLESS, _frictionless_start(ws)[2]),
                                   x=_frictionless_start(ws)[0] + V_FRICTIONLESS * DT * np.arange(1, N_FRICTIONLESS + 1), finite=1.0),
          observed=lambda traj, ws: dict(v=traj[:, W_CUBEA + 7], z=traj[:, W_CUBEA + 2], x=traj[:, W_CUBEA],
                                         finite=float(np.isfinite(traj[:, :W_OBS + 3]).all() and np.isfinite(traj[:, W_HELD:]).all())),
          tol=dict(v=(0.0, 1e-6), z=(0.0, 1e-4), x=(0.0, 1e-4), finite=BOOL), fields=[], overrides=dict(mu=0.0)))

# ---- mu = 0: a cube sliding on the table into the shelf stand's -x face stops there (a stated limit: see the module docstring)
N_INTO = 80


def _into_start(ws):
    sx, sy, _, shx, _ = support(ws, "shelf")
    return (sx - shx - CUBE_HALF - 0.06, sy, support(ws, "table")[2] + CUBE_HALF)


_add(Form("slide_into_shelf", lambda ws: parked(ws, cubeA=_into_start(ws), vA=(V_FRICTIONLESS, 0.0, 0.0)), N_INTO,
          expected=lambda ws: dict(face=ws["shelf"][0] - ws["shelf"][3], z=_into_start(ws)[2], asleep=1.0),
          observed=lambda traj, ws: dict(face=traj[-1, W_CUBEA] + CUBE_HALF, z=traj[-1, W_CUBEA + 2], asleep=_asleep(traj)),
          tol=dict(face=(0.0, CONTACT_OFFSET), z=(0.0, REST_GAP), asleep=BOOL), fields=["shelf[0]", "shelf[3]"],
          overrides=dict(mu=0.0)))

# ---- forward kinematics in the workspace's base: not a trajectory, see fk_expected
FK_ATOL = 3e-6      # tests/test_dynamics_physics.py::test_panda_fk_is_the_urdf_chain


def fk_expected(ws, q):
    """positions of link7, hand, left and right finger and the hand's y and z axes, [6, 3]"""
    c = chain(ws, q)
    return np.array([c["link7"], c["hand"], c["left"], c["right"], c["R"][:, 1], c["R"][:, 2]])


def fk_poses(n=24, seed=11):
    lo = np.array([-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973, 0.0, 0.0])
    hi = np.array([2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973, 0.04, 0.04])
    return np.random.default_rng(seed).uniform(lo, hi, (n, 9)).astype(np.float32)


# ---- the gripper driven onto a surface: it stops there and stalls (the gripper path: pt_box on the static boxes, through base)
V_DESCENT, N_DESCENT = 0.2, 70


def _servo(ws, row, v, grip):
    """joint velocity targets that move the hand's origin at v (the planner's bounds), the fingers commanded `grip`"""
    u = np.zeros(9)
    u[:7] = np.clip(np.linalg.pinv(hand_jacobian(ws, row[:9])) @ np.asarray(v, np.float64), -2.0, 2.0)
    u[7:] = grip
    return u


def _descent_point(ws, which):
    bx, by, _ = ws["base"]
    if which == "table":
        return bx + 0.6, by - 0.2, support(ws, "table")[2]
    sx, sy, top, shx, _ = support(ws, "shelf")
    return sx - shx + 0.03, sy, top


def _tip_bottom(ws, q):
    a, b, _ = tips(ws, q)
    return min(a[2], b[2]) - TIP_R


def _stalled(gaps, first, dt):
    """the largest speed of the tip towards or off the surface from five steps after its arrival on (pressed against a surface
    the hand still pivots about the tip; the tip stays)"""
    return float(np.abs(np.diff(gaps[min(first + 4, len(gaps) - 2):])).max() / dt)


def reaches(ws, world):
    try:
        world(ws)
        return True
    except AssertionError:
        return False


def descent_form(name, which, fields, dt=DT, substeps=SUBSTEPS, lean=0.0):
    def world(ws):
        x, y, top = _descent_point(ws, which)
        q = ik_down(ws, (x, y, top + HAND_TO_TIP + TIP_R + 0.02), lean)
        q[7], q[8] = 0.04, 0.0
        return parked(ws, q=q)

    def observed(traj, ws):
        top = _descent_point(ws, which)[2]
        gaps = np.array([_tip_bottom(ws, r[:9]) - top for r in traj])
        first = min(int(np.nonzero(gaps < 1e-3)[0][0]) if (gaps < 1e-3).any() else len(gaps), len(gaps) - 6)
        ft = W_FT if which == "table" else W_FS
        return dict(arrives=float(first), deepest=min(0.0, gaps.min()), lifts=max(0.0, gaps[first:].max()),
                    stalled=_stalled(gaps, first, dt), presses=float(traj[first + 5:, ft + 2].min() < -1.0))

    # 2 cm at 0.2 m/s: 0.1 s, after the servo's few substeps
    return Form(name, world, N_DESCENT, lambda ws: dict(arrives=0.1 / dt + 2, deepest=0.0, lifts=0.0, stalled=0.0, presses=1.0), observed,
                dict(arrives=(0.0, 5.0), deepest=(0.0, 2e-3), lifts=(0.0, 1e-3), stalled=(0.0, 0.05), presses=BOOL), fields,
                control=lambda ws, row: _servo(ws, row, (0.0, 0.0, -V_DESCENT), (0.0, 0.0)), dt=dt, substeps=substeps,
                applies=lambda ws: reaches(ws, world), anchor=lambda ws: dict(deepest=_descent_point(ws, which)[2]))


_add(descent_form("descent_table", "table", ["base[0]", "base[1]", "base[2]", "table[2]", "table[5]"]))
_add(descent_form("descent_shelf", "shelf", ["base[0]", "base[1]", "base[2]", "shelf[2]", "shelf[5]"]))

# ---- the gripper driven sideways into the shelf stand's -x face, its tips 1.5 cm under the stand's top (the hand's own sphere
# passes above it)
TIP_UNDER_TOP = 0.015


def _side_world(ws):
    sx, sy, top, shx, _ = support(ws, "shelf")
    q = ik_down(ws, (sx - shx - TIP_R - 0.02, sy, top - TIP_UNDER_TOP + HAND_TO_TIP))
    q[7], q[8] = 0.0, 0.0
    return parked(ws, q=q)


def _side_observed(traj, ws):
    face = ws["shelf"][0] - ws["shelf"][3]
    gaps = np.array([face - (max(tips(ws, r[:9])[0][0], tips(ws, r[:9])[1][0]) + TIP_R) for r in traj])
    first = min(int(np.nonzero(gaps < 1e-3)[0][0]) if (gaps < 1e-3).any() else len(gaps), len(gaps) - 6)
    return dict(arrives=float(first), deepest=min(0.0, gaps.min()), lifts=max(0.0, gaps[first:].max()),
                stalled=_stalled(gaps, first, DT), presses=float(traj[first + 5:, W_FS].max() > 1.0))


_add(Form("side_shelf", _side_world, N_DESCENT, lambda ws: dict(arrives=12.0, deepest=0.0, lifts=0.0, stalled=0.0, presses=1.0),
          _side_observed, dict(arrives=(0.0, 5.0), deepest=(0.0, 2e-3), lifts=(0.0, 1e-3), stalled=(0.0, 0.05), presses=BOOL),
          ["base[0]", "base[1]", "base[2]", "shelf[0]", "shelf[3]"],
          control=lambda ws, row: _servo(ws, row, (V_DESCENT, 0.0, 0.0), (-1.5, -1.5)), applies=lambda ws: reaches(ws, _side_world),
          anchor=lambda ws: dict(deepest=ws["shelf"][0] - ws["shelf"][3])))

# ---- the closed gripper swept at 0.25 m/s towards a face of the floating plate: -x, -y, and the top from above
V_SWEEP, N_SWEEP, GAP0 = 0.25, 40, 0.03


def _sweep_hand(ws):
    bx, by, _ = ws["base"]
    return np.array([bx + 0.55, by - 0.2, support(ws, "table")[2] + 0.35])


def _plate_start(ws, ax):
    tip = _sweep_hand(ws) - np.array([0, 0, HAND_TO_TIP])
    p = tip.copy()
    if ax < 2:
        p[ax] += TIP_R + GAP0 + ws["obs_half"][ax]
        p[2] -= 0.5 * ws["obs_half"][2]                 # the tips meet the face's upper half: the hand's own sphere stays above the plate
    else:
        p[2] -= TIP_R + GAP0 + ws["obs_half"][2]
    return p


def plate_form(name, ax):
    sign = 1.0 if ax < 2 else -1.0
    vdir = np.zeros(3)
    vdir[ax] = sign * V_SWEEP

    def world(ws):
        q = ik_down(ws, _sweep_hand(ws))
        q[7], q[8] = 0.0, 0.0
        return parked(ws, q=q, plate=_plate_start(ws, ax))

    def observed(traj, ws):
        p0 = _plate_start(ws, ax).astype(np.float32).astype(np.float64)      # (as the world row carries it)
        lead = np.array([sign * max(sign * tips(ws, r[:9])[0][ax], sign * tips(ws, r[:9])[1][ax]) for r in traj])   # the leading tip centre
        # the gap a plate that stays where it is would have to the leading tip sphere, after each step
        virtual = sign * (p0[ax] - sign * ws["obs_half"][ax] - lead) - TIP_R
        before = np.concatenate([[GAP0], virtual[:-1]])
        moved = np.abs(traj[:, W_OBS:W_OBS + 3] - p0).max(axis=1)
        early = before > CONTACT_OFFSET + DT * V_SWEEP * 1.5      # (the whole step's travel, the servo's overshoot included)
        late = virtual < 0.0
        assert early.sum() >= 3 and late[:-1].any(), (name, virtual.tolist())
        t_late = int(np.nonzero(late)[0][0])
        # ... and the smallest distance between the plate's centre and the leading tip sphere's centre along the sweep
        return dict(moved_early=moved[early].max(), moved_late=float(moved[t_late] > 0.0),
                    closest=(sign * (traj[:, W_OBS + ax] - lead)).min())

    return Form(name, world, N_SWEEP, lambda ws: dict(moved_early=0.0, moved_late=1.0, closest=ws["obs_half"][ax] + TIP_R), observed,
                dict(moved_early=BOOL, moved_late=BOOL), [f"obs_half[{ax}]"],
                control=lambda ws, row: _servo(ws, row, vdir, (-1.5, -1.5)),
                measured=dict(closest="plate_onset.side" if ax < 2 else "plate_onset.top"))


for _ax in range(3):
    _add(plate_form("plate_face_" + "xyz"[_ax], _ax))

# many environments of one wrapper side by side, each with its own parameter: row i slides for 11 .. 18 steps (its own v0) /
# is released from 0.08 .. 0.20 m; neighbouring rows differ by at least three steps of mu g dt / by at least 2 cm
def row_form(kind, i):
    if kind == "slide_table_x":
        return slide_form(kind, "table", 0, n_slide=11 + (3 * i) % 8)
    assert kind == "fall_table"
    return drop_form(kind, "table", release=0.08 + 0.02 * ((3 * i) % 7), fields=["table[2]", "table[5]"], at=(0.4, -0.4))


ROW_FORMS = ("fall_table", "slide_table_x")

# which forms' expected values depend on a field (every one of the 21 but obs_m appears)
FIELD_FORMS = {}
for _f in FORMS.values():
    for _k in _f.fields:
        FIELD_FORMS.setdefault(_k, []).append(_f.name)
for _i in range(3):
    FIELD_FORMS.setdefault(f"base[{_i}]", []).insert(0, "fk")
FIELD_NAMES = ([f"base[{i}]" for i in range(3)] + [f"table[{i}]" for i in range(6)] + [f"shelf[{i}]" for i in range(6)] +
               [f"obs_half[{i}]" for i in range(3)] + ["obs_m", "cube_m", "mu"])


def perturbed(ws, field, factor=1.1):
    """the workspace with one of its 21 fields scaled"""
    ws = {k: (tuple(v) if isinstance(v, (tuple, list)) else v) for k, v in ws_full(ws).items()}
    if "[" in field:
        name, i = field[:-1].split("[")
        v = list(ws[name])
        v[int(i)] *= factor
        ws[name] = tuple(v)
    else:
        ws[field] *= factor
    return ws


def flat(values):
    """{quantity: array} -> one float64 vector, quantities in sorted order"""
    return np.concatenate([np.ravel(np.asarray(values[k], np.float64)) for k in sorted(values)])


# ------------------------------------------------------------------ the fused rollout: what a sample's states and costs must show
# A rollout returns each sample's (q0, q0', q1, q1') and its cost after every step.  The samples share one start world -- cubeA
# released above / sliding on the table, the arm folded above its base -- and each applies its own constant velocity targets
# to joints 0 and 1, which stay far from everything: the states are the joint servo's recursion under the sample's own
# controls, and the cube's pose, the same in every sample, is the closed form's.
T_ROLL = 20
DRIVE_D = 600.0
INERTIA01, EFFORT01, VLIM01 = (1.32, 2.12), (87.0, 87.0), (2.175, 2.175)      # joints 0 and 1: mesh-derived inertia, URDF limits
ROLL_FORMS = {
    "fall_table": drop_form("fall_table", "table", release=0.06, steps=T_ROLL, at=(0.4, -0.4)),
    "footprint_table_-x_in": drop_form("footprint_table_-x_in", "table", "-x", True, release=0.06, steps=T_ROLL),
    "footprint_table_-x_out": drop_form("footprint_table_-x_out", "table", "-x", False, release=0.06, steps=T_ROLL),
    "slide_table_x": slide_form("slide_table_x", "table", 0, n_slide=10),
}


def rollout_controls(K):
    """[K, 9]: sample k's velocity targets of joints 0 and 1, spread over +-1.5 / +-1 rad/s; everything else zero"""
    k = np.arange(K)
    u = np.zeros((K, 9))
    u[:, 0] = -1.5 + 3.0 * ((k * 37) % 101) / 100.0
    u[:, 1] = -1.0 + 2.0 * ((k * 61) % 103) / 102.0
    return u


def servo_states(u, n_steps=T_ROLL, dt=DT, substeps=SUBSTEPS):
    """the implicit damper with the URDF's effort and velocity limits (tests/test_dynamics_physics.py::
    test_panda_servo_is_the_implicit_damper...) for joints 0 and 1 from rest at Q_PARK: [K, n_steps, 4] = (q0, q0', q1, q1')"""
    u = np.asarray(u, np.float64)[:, :2]
    h = substep(dt, substeps)
    inertia, effort, vlim = np.array(INERTIA01), np.array(EFFORT01), np.array(VLIM01)
    a = h * DRIVE_D / inertia
    q, v = np.tile(np.array(Q_PARK[:2]), (len(u), 1)), np.zeros((len(u), 2))
    out = np.zeros((len(u), n_steps, 4))
    for t in range(n_steps):
        for _ in range(substeps):
            dv = (v + a * u) / (1 + a) - v
            v = np.clip(v + np.clip(dv, -effort * h / inertia, effort * h / inertia), -vlim, vlim)
            q = q + h * v
        out[:, t, 0], out[:, t, 1], out[:, t, 2], out[:, t, 3] = q[:, 0], v[:, 0], q[:, 1], v[:, 1]
    return out


def cube_track(form, ws, bounds):
    """what the closed form says about cubeA after each of the form's steps: (position [steps, 3], NaN where it makes no claim;
    the bound on |position error| [steps]; sliding [steps]: 1 where the surface reports the slide's friction, 0 where the cube
    is in the air or asleep, NaN where the form does not say).  bounds: tests/panda_workspace_mechanics_checks.bounds_of(form, ws)"""
    want = form.expected(ws)
    start = form.world(ws)[W_CUBEA:W_CUBEA + 3]
    pos, tol, sliding = np.full((form.steps, 3), np.nan), np.zeros(form.steps), np.full(form.steps, np.nan)
    if "z_free" in want:
        n = len(want["z_free"])
        pos[:n, 0], pos[:n, 1], pos[:n, 2] = start[0], start[1], want["z_free"]
        tol[:n] = bounds["z_free"][1]
        sliding[:n] = 0.0
        if "rest_z" in want:
            pos[-1] = (start[0], start[1], want["rest_z"])
            tol[-1] = bounds["rest_z"][1] + 2.0 * bounds["xy"][1]
            sliding[-1] = 0.0
    else:
        ax = int(np.argmax(np.abs(form.world(ws)[W_CUBEA + 7:W_CUBEA + 9])))
        pos[:, ax], pos[:, 1 - ax], pos[:, 2] = want["x"], want["across"], want["rest_z"]
        tol[:] = bounds["x"][1] + bounds["across"][1] + bounds["rest_z"][1]
        moving = want["v"] > 0.0
        last = int(np.nonzero(moving)[0][-1])
        sliding[:last] = 1.0            # (the step in which it comes to rest reports what its last substep saw)
        sliding[last + 2:] = 0.0
    return pos, tol, sliding
