"""Closed forms of rigid-body mechanics as functions of the point_env ARENA (a helper, not a test).

Written from mechanics and the names of the arena's fields alone: binary64, no call into the oracle or the library.  A FORM is a
small scene -- a start world, a constant control, a number of steps, in an arena given as a dict of _lib.POINT_SCENE_DEFAULTS'
keys -- with the numbers a rigid-body simulator must show in it: `expected(sd)` computes them from the arena, `observed(traj)`
reads the same quantities off a trajectory (the 31-float world rows after each step, whoever stepped them).  The tests
(tests/test_arena_mechanics_cpu.py on the CPU oracle and the host build of the device header, tests/test_arena_mechanics_gpu.py
on the kernels) compare the two.  Every field of the arena enters the expected value of at least one form (FIELD_FORMS), so a
box / dyn-obs mix-up, an x / y mix-up or a wrong friction pair in a derived constant -- invisible at the default arena, where
box == dyn-obs, hx == hy and mu_rd == mu_ro == mu_rw -- shows as a number off its closed form.

World row: robot, box, dyn-obs as (x, y, cos, sin, vx, vy, w) at columns 0, 7, 14 | pending force on robot, box at 21, 23 |
net contact force on robot, box, dyn-obs at 25, 27, 29."""
import numpy as np

G, DRIVE_D, DRIVE_FMAX, CONTACT_OFFSET = 9.8, 600.0, 1000.0, 0.01
DT, SUBSTEPS = 0.05, 2
W_R, W_B, W_D, W_FEXT_B, W_FC_R, ROW = 0, 7, 14, 23, 25, 31

# Two arenas that break every symmetry of the default one at once: box != dyn-obs in mass, inertia, r_eq and ground friction;
# hx != hy for both, the x sums (0.42 / 0.36) != the y sums (0.45 / 0.39); four distinct robot friction pairs; robot, walls and
# obstacle away from the defaults.  (The obstacles stand in the upper half plane: the forms play in the lower one.)
ARENA_A = dict(robot_r=0.25, robot_m=8.0,
               box_hx=0.3, box_hy=0.15, box_m=9.0, box_I=9.0 * (0.6 ** 2 + 0.3 ** 2) / 12.0, box_mu_g=0.6, box_req=0.1,
               dyn_hx=0.12, dyn_hy=0.3, dyn_m=25.0, dyn_I=25.0 * (0.24 ** 2 + 0.6 ** 2) / 12.0, dyn_mu_g=0.9, dyn_req=0.2,
               obs_x=-1.0, obs_y=0.5, obs_hx=0.25, obs_hy=0.22, wall=2.4, mu_rb=0.2, mu_rd=0.35, mu_ro=0.3, mu_rw=0.45)
ARENA_B = dict(robot_r=0.15, robot_m=12.5,
               box_hx=0.1, box_hy=0.25, box_m=20.0, box_I=20.0 * (0.2 ** 2 + 0.5 ** 2) / 12.0, box_mu_g=0.35, box_req=0.12,
               dyn_hx=0.26, dyn_hy=0.14, dyn_m=6.0, dyn_I=6.0 * (0.52 ** 2 + 0.28 ** 2) / 12.0, dyn_mu_g=0.5, dyn_req=0.09,
               obs_x=0.9, obs_y=1.0, obs_hx=0.2, obs_hy=0.3, wall=2.8, mu_rb=0.5, mu_rd=0.15, mu_ro=0.6, mu_rw=0.25)
ARENAS = {"A": ARENA_A, "B": ARENA_B}
# the fields no steady closed form anchors (friction between the boxes, the walls and the obstacle: it acts while a box turns)
UNANCHORED = ("mu_bw", "mu_dw", "mu_bd", "mu_bo", "mu_do")


def substep(dt=DT, substeps=SUBSTEPS):
    return dt / substeps


# ------------------------------------------------------------------ the closed forms
def drive(sd, u, n_steps, dt=DT, substeps=SUBSTEPS):
    """m dv/dt = D (u - v), implicit Euler per substep, the force limited to F_max: dv = clip(a (u - v) / (1 + a), +-F_max h / m),
    a = D h / m.  Velocity and travelled distance after each step, [n_steps, 2] each."""
    h = substep(dt, substeps)
    a, cap = DRIVE_D * h / sd["robot_m"], DRIVE_FMAX * h / sd["robot_m"]
    u, v, x, vs, xs = np.asarray(u, np.float64), np.zeros(2), np.zeros(2), [], []
    for _ in range(n_steps):
        for _ in range(substeps):
            v = v + np.clip(a * (u - v) / (1.0 + a), -cap, cap)
            x = x + h * v
        vs.append(v.copy()); xs.append(x.copy())
    return np.array(vs), np.array(xs)


def coulomb_slide(sd, body, v0, n_steps, dt=DT, substeps=SUBSTEPS):
    """a sliding body (`box` / `dyn`): v -= mu_g g h per substep, clamped at rest; x += h v.  (speed, distance) after each step"""
    h, mu = substep(dt, substeps), sd[body + "_mu_g"]
    v, x, out = float(v0), 0.0, []
    for _ in range(n_steps):
        for _ in range(substeps):
            v = max(0.0, v - mu * G * h)
            x += h * v
        out.append((v, x))
    return np.array(out)


def coulomb_spin(sd, body, w0, n_steps, dt=DT, substeps=SUBSTEPS):
    """a body spinning in place: the friction torque mu_g m g r_eq decelerates it at a constant rate: w -= mu_g m g r_eq h / I"""
    h = substep(dt, substeps)
    dw = sd[body + "_mu_g"] * sd[body + "_m"] * G * sd[body + "_req"] * h / sd[body + "_I"]
    w, out = abs(float(w0)), []
    for _ in range(n_steps):
        for _ in range(substeps):
            w = max(0.0, w - dw)
        out.append(np.sign(w0) * w)
    return np.array(out)


def momenta(sd, row):
    """linear momentum, angular momentum about the origin and kinetic energy of the box / dyn-obs pair of one world row"""
    p, L, E = np.zeros(2), 0.0, 0.0
    for b, name in ((W_B, "box"), (W_D, "dyn")):
        m, inertia = sd[name + "_m"], sd[name + "_I"]
        x, y, _, _, vx, vy, om = np.asarray(row, np.float64)[b:b + 7]
        p += m * np.array([vx, vy])
        L += m * (x * vy - y * vx) + inertia * om
        E += 0.5 * m * (vx * vx + vy * vy) + 0.5 * inertia * om * om
    return p, L, E


# ------------------------------------------------------------------ worlds
def parked(sd, robot=None, box=None, dyn=None, robot_right=False):
    """a world row with everything the form does not use at rest in a corner of the arena: robot lower left (lower right with
    `robot_right`), box upper right, dyn-obs upper left; robot (x, y), box / dyn-obs (x, y, cos, sin, vx, vy, w)"""
    c = sd["wall"] - 0.6
    w = np.zeros(ROW)
    w[0:2] = (c if robot_right else -c, -c) if robot is None else robot
    w[W_B:W_B + 7] = (c, c, 1, 0, 0, 0, 0) if box is None else box
    w[W_D:W_D + 7] = (-c, c, 1, 0, 0, 0, 0) if dyn is None else dyn
    w[2] = 1.0
    return w


class Form:
    """name; overrides (fields the form sets on top of the arena, e.g. no ground friction); world(sd) -> row; u; steps;
    expected(sd) -> {quantity: value}; observed(traj, sd) -> {quantity: value}; tol {quantity: (rtol, atol)};
    robot_only: the quantities a fused rollout shows (it returns the robot's states only); fields: what the expected values
    depend on"""

    def __init__(self, name, world, u, steps, expected, observed, tol, fields, overrides=None, robot_only=()):
        self.name, self.world, self.u, self.steps, self.expected, self.observed = name, world, tuple(u), steps, expected, observed
        self.tol, self.fields, self.overrides, self.robot_only = tol, tuple(fields), dict(overrides or {}), tuple(robot_only)

    def scene(self, arena):
        """the arena the form runs in: the given field overrides and the form's own"""
        return {**(arena or {}), **self.overrides}


Y0 = -1.0          # the line the forms play on
NO_GROUND = dict(box_mu_g=0.0, dyn_mu_g=0.0)
FORMS = {}


def _add(form):
    FORMS[form.name] = form


def _body(b):
    return W_B if b == "box" else W_D


def _place(b, pose):
    return dict(box=pose) if b == "box" else dict(dyn=pose)


# ---- velocity drive: below the effort limit, and a first substep at it
DRIVE_START = (0.0, -0.3)


def drive_form(name, u, n):
    return Form(name, lambda sd: parked(sd, robot=DRIVE_START), u, n,
                expected=lambda sd: dict(v=drive(sd, u, n)[0], x=drive(sd, u, n)[1] + np.array(DRIVE_START)),
                observed=lambda traj, sd: dict(v=traj[:n, 4:6], x=traj[:n, 0:2]),
                tol=dict(v=(2e-6, 0.0), x=(2e-6, 0.0)), fields=["robot_m"], robot_only=("v", "x"))


_add(drive_form("drive", (1.5, -0.75), 4))
_add(drive_form("drive_limit", (6.0, -0.5), 2))

# ---- Coulomb slide and spin, box and dyn-obs each from their own fields
for _b in ("box", "dyn"):
    _v0, _w0 = (2.0, 3.0) if _b == "box" else (1.6, -8.0)
    _add(Form("slide_" + _b, lambda sd, b=_b, v0=_v0: parked(sd, **_place(b, (-0.6, Y0, 1, 0, v0, 0, 0))), (0.0, 0.0), 8,
              expected=lambda sd, b=_b, v0=_v0: dict(v=coulomb_slide(sd, b, v0, 8)[:, 0], x=-0.6 + coulomb_slide(sd, b, v0, 8)[:, 1]),
              observed=lambda traj, sd, b=_b: dict(v=traj[:, _body(b) + 4], x=traj[:, _body(b)]),
              tol=dict(v=(0.0, 2e-6), x=(0.0, 2e-6)), fields=[_b + "_mu_g"]))
    _add(Form("spin_" + _b, lambda sd, b=_b, w0=_w0: parked(sd, **_place(b, (-0.6, Y0, 1, 0, 0, 0, w0))), (0.0, 0.0), 2,
              expected=lambda sd, b=_b, w0=_w0: dict(w=coulomb_spin(sd, b, w0, 2)),
              observed=lambda traj, sd, b=_b: dict(w=traj[:, _body(b) + 6]),
              tol=dict(w=(1e-5, 0.0)), fields=[_b + "_mu_g", _b + "_m", _b + "_req", _b + "_I"]))

# ---- a pending external force on the box: consumed by the next step's first substep, dv = F h / m (no ground friction)
FEXT = (80.0, -40.0)


def _fext_world(sd):
    w = parked(sd, box=(-0.6, Y0, 1, 0, 0, 0, 0))
    w[W_FEXT_B:W_FEXT_B + 2] = FEXT
    return w


_add(Form("fext_box", _fext_world, (0.0, 0.0), 2,
          expected=lambda sd: dict(v=np.tile(np.array(FEXT) * substep() / sd["box_m"], (2, 1))),      # (then it coasts)
          observed=lambda traj, sd: dict(v=traj[:, W_B + 4:W_B + 6]),
          tol=dict(v=(1e-6, 0.0)), fields=["box_m"], overrides=dict(box_mu_g=0.0)))

# ---- slow head-on approach of the isolated pair along x and along y (0.3 m/s, below contact_offset / h: the speculative
# contact stops the approach at the surface): perfectly inelastic, common velocity m_b v0 / (m_b + m_d), centres hx + hx
# (hy + hy) apart
V_SLOW = 0.3
for _ax in (0, 1):
    _hk = ("hx", "hy")[_ax]

    def _headon_world(sd, ax=_ax, hk=_hk):
        gap = sd["box_" + hk] + sd["dyn_" + hk] + 0.045
        b = [-0.6, -0.8 if ax == 0 else -1.4, 1, 0, 0, 0, 0]
        d = list(b)
        d[ax] += gap
        b[4 + ax] = V_SLOW
        return parked(sd, box=b, dyn=d, robot_right=True)

    _add(Form("headon_" + "xy"[_ax], _headon_world, (0.0, 0.0), 12,
              expected=lambda sd, hk=_hk: dict(v_box=sd["box_m"] * V_SLOW / (sd["box_m"] + sd["dyn_m"]),
                                               v_dyn=sd["box_m"] * V_SLOW / (sd["box_m"] + sd["dyn_m"]),
                                               distance=sd["box_" + hk] + sd["dyn_" + hk]),
              observed=lambda traj, sd, ax=_ax: dict(v_box=traj[-1, W_B + 4 + ax], v_dyn=traj[-1, W_D + 4 + ax],
                                                     distance=traj[-1, W_D + ax] - traj[-1, W_B + ax]),
              tol=None, fields=["box_m", "dyn_m", "box_" + _hk, "dyn_" + _hk], overrides=NO_GROUND))

# ---- steady push: the pair settles where the damper's force equals the box's ground friction
U_PUSH, N_PUSH = 2.0, 16


def push_form(name="push", u=U_PUSH, n=N_PUSH):
    v = lambda sd: u - sd["box_mu_g"] * sd["box_m"] * G / DRIVE_D      # noqa: E731
    return Form(name, lambda sd: parked(sd, robot=(-1.6, Y0), box=(-1.6 + sd["robot_r"] + sd["box_hx"] + 0.05, Y0, 1, 0, 0, 0, 0)),
                (u, 0.0), n,
                expected=lambda sd: dict(v=v(sd), v_box=v(sd), force=-sd["box_mu_g"] * sd["box_m"] * G, distance=sd["robot_r"] + sd["box_hx"]),
                observed=lambda traj, sd: dict(v=traj[n - 1, 4], v_box=traj[n - 1, W_B + 4], force=traj[n - 1, W_FC_R],
                                               distance=traj[n - 1, W_B] - traj[n - 1, 0]),
                tol=dict(v=(1e-3, 0.0), v_box=(1e-3, 0.0), force=(2e-3, 0.0), distance=(0.0, CONTACT_OFFSET)),
                fields=["box_mu_g", "box_m", "robot_r", "box_hx"], robot_only=("v",))


_add(push_form())

# ---- the robot driven into a wall / the obstacle with a tangential command: it rests at the surface (within contact_offset)
# and slides along it at v_t = u_t - mu u_n (the normal force is the damper's, D u_n, below the effort limit).  It starts GAP
# above the surface, at rest: the speculative contact stops the approach there, so the normal direction is steady from the
# first step and the tangential one after the drive's few substeps.
U_N, U_T_WALL, U_T_OBS, N_REST, GAP = 1.0, 2.0, 0.9, 8, 0.002
REST_KINDS = {   # kind: (normal axis, sign of the approach, world, rest position, friction field, other fields)
    "wall_x": (0, +1, lambda sd: parked(sd, robot=(sd["wall"] - sd["robot_r"] - GAP, -1.4)),
               lambda sd: sd["wall"] - sd["robot_r"], "mu_rw", ["wall", "robot_r"]),
    "wall_y": (1, -1, lambda sd: parked(sd, robot=(-0.6, -(sd["wall"] - sd["robot_r"] - GAP))),
               lambda sd: -(sd["wall"] - sd["robot_r"]), "mu_rw", ["wall", "robot_r"]),
    "obs_x": (0, +1, lambda sd: parked(sd, robot=(sd["obs_x"] - sd["obs_hx"] - sd["robot_r"] - GAP, sd["obs_y"] - sd["obs_hy"] + 0.05)),
              lambda sd: sd["obs_x"] - sd["obs_hx"] - sd["robot_r"], "mu_ro", ["obs_x", "obs_hx", "robot_r"]),
    "obs_y": (1, +1, lambda sd: parked(sd, robot=(sd["obs_x"] - sd["obs_hx"] + 0.05, sd["obs_y"] - sd["obs_hy"] - sd["robot_r"] - GAP)),
              lambda sd: sd["obs_y"] - sd["obs_hy"] - sd["robot_r"], "mu_ro", ["obs_y", "obs_hy", "robot_r"]),
}


def rest_form(kind, u_n=U_N, u_t=None, n=N_REST, name=None):
    """the robot pressed at u_n (> 0) into the surface `kind` and commanded u_t (> mu u_n) along it"""
    n_ax, sign, world, rest, mu_key, fields = REST_KINDS[kind]
    u_t = (U_T_WALL if kind.startswith("wall") else U_T_OBS) if u_t is None else u_t
    u = [0.0, 0.0]
    u[n_ax], u[1 - n_ax] = sign * u_n, u_t
    return Form(name or kind, world, u, n,
                expected=lambda sd: dict(rest=rest(sd), v_n=0.0, v_t=u_t - sd[mu_key] * u_n),
                observed=lambda traj, sd: dict(rest=traj[n - 1, n_ax], v_n=traj[n - 1, 4 + n_ax], v_t=traj[n - 1, 5 - n_ax]),
                tol=None, fields=fields + [mu_key], robot_only=("rest", "v_n", "v_t"))


for _kind in REST_KINDS:
    _add(rest_form(_kind))

# ---- a box / the dyn-obs sliding without ground friction into the +x / +y wall: it stops at wall - hx / wall - hy.  (It meets
# the wall after 10 steps; the position is read 1 s later.  Where the two corner rows' six passes leave the body ~1 % of its
# speed and a slow spin it drifts off again at millimetres per second -- nothing damps a body without ground friction.  The
# residual speed along the wall's normal is bounded by what keeps it within contact_offset for that second: contact_offset / 1 s,
# 3 % of the approach speed.)
N_BOXWALL = 30
for _b in ("box", "dyn"):
    for _ax in (0, 1):
        _hk = _b + "_" + ("hx", "hy")[_ax]

        def _boxwall_world(sd, b=_b, ax=_ax, hk=_hk):
            pose = [0.0, Y0, 1, 0, 0, 0, 0] if ax == 0 else [0.0, 0.0, 1, 0, 0, 0, 0]
            pose[ax] = sd["wall"] - sd[hk] - 0.15
            pose[4 + ax] = V_SLOW
            return parked(sd, **_place(b, pose))

        _add(Form(f"{_b}wall_{'xy'[_ax]}", _boxwall_world, (0.0, 0.0), N_BOXWALL,
                  expected=lambda sd, hk=_hk: dict(rest=sd["wall"] - sd[hk], v_n=0.0),
                  observed=lambda traj, sd, b=_b, ax=_ax: dict(rest=traj[N_BOXWALL - 1, _body(b) + ax],
                                                               v_n=traj[N_BOXWALL - 1, _body(b) + 4 + ax]),
                  tol=dict(rest=(0.0, CONTACT_OFFSET), v_n=(0.0, CONTACT_OFFSET / 1.0)), fields=["wall", _hk], overrides=NO_GROUND))


def pair_worlds(sd, n=12, seed=5):
    """oblique, off-centre, spinning hits of the box on the dyn-obs (no ground friction: an isolated pair)"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        th = rng.uniform(-0.7, 0.7)
        box = (-1.2, -0.8 + rng.uniform(-0.2, 0.2), np.cos(th), np.sin(th), rng.uniform(1.0, 2.5), rng.uniform(-0.4, 0.4), rng.uniform(-2, 2))
        dyn = (-0.3, -0.8, 1, 0, rng.uniform(-1.0, 0.0), 0, 0)
        rows.append(parked(sd, box=box, dyn=dyn, robot_right=True))
    return np.array(rows)


def fast_headon_world(sd, ax):
    """the pair head-on at 2 m/s: the solver's Baumgarte term separates it again, so only the conservation laws hold"""
    hk = ("hx", "hy")[ax]
    b = [-1.2, -0.8 if ax == 0 else -1.6, 1, 0, 0, 0, 0]
    d = list(b)
    d[ax] += sd["box_" + hk] + sd["dyn_" + hk] + 0.3
    b[4 + ax] = 2.0
    return parked(sd, box=b, dyn=d, robot_right=True)


def press_world(sd, b):
    """the robot pressed against the box / dyn-obs (`b`) that stands against the +x wall, the other body parked: the scene of
    mu_rb / mu_rd.  (No closed form: on the oracle the blocked body never comes to rest -- it creeps and turns at ~1e-2 m/s
    until the robot slides off it -- so the tests hold the weaker statement that each field acts on its own pair only.)"""
    hx, hy = sd[b + "_hx"], sd[b + "_hy"]
    return parked(sd, robot=(sd["wall"] - 2 * hx - sd["robot_r"] - GAP, Y0 - 0.5 * hy), **_place(b, (sd["wall"] - hx, Y0, 1, 0, 0, 0, 0)))


U_PRESS, N_PRESS = (1.0, 0.6), 6
PAIR_ONLY = {"mu_rb": "box", "mu_rd": "dyn"}      # anchored by "acts on its own pair only", not by a closed form

# ---- one arena per environment (step mode): five arenas, the default among them, neighbours (cyclically) different in robot_m,
# box_mu_g, box_m, wall and robot_r
ROW_ARENAS = [None,
              dict(robot_m=6.0, box_mu_g=0.4, box_m=9.0, box_I=9.0 * 0.32 / 12.0, wall=3.0, robot_r=0.25, mu_rw=0.3),
              dict(robot_m=14.0, box_mu_g=0.9, box_m=24.0, box_I=24.0 * 0.32 / 12.0, wall=2.6, robot_r=0.15, mu_rw=0.6),
              ARENA_A, ARENA_B]
ROW_FORMS = ("drive", "slide_box", "push", "wall_x")


def sample_arena(k):
    """arena of sample k of a fused rollout whose samples share ONE start world: robot_m, box_m, box_mu_g, mu_rw, mu_ro differ
    from sample to sample; robot_r, wall, the obstacle's and the box's half extents differ too, by a d that leaves the
    surfaces the robot meets (wall - robot_r, obs - h - robot_r, robot_r + box_hx) where they are"""
    d = 0.01 * (k % 8)
    box_m = 8.0 + (k * 5) % 9       # (box_m / robot_m <= 2: see test_steady_push_falls_short_for_a_heavy_box_on_a_light_robot)
    return dict(robot_m=8.0 + (k * 7) % 9, mu_rw=0.2 + 0.03 * (k % 11), mu_ro=0.25 + 0.04 * (k % 9), box_m=box_m,
                box_I=box_m * (0.6 ** 2 + 0.3 ** 2) / 12.0, box_mu_g=0.3 + 0.05 * (k % 10), robot_r=0.2 + d, wall=2.5 + d,
                obs_x=-1.0, obs_y=0.5, obs_hx=0.35 - d, obs_hy=0.3 - d, box_hx=0.3 - d, box_hy=0.15)


def sample_control(kind, k):
    """control of sample k, by the kind of form: spread over the range in which the form's closed form holds"""
    a, b = ((k * 37) % 101) / 100.0, ((k * 61) % 103) / 102.0
    if kind == "drive":
        return (-6.0 + 12.0 * a, 0.0 - 3.0 * b)              # (below and at the effort limit; away from the obstacle)
    if kind == "push":
        return (1.5 + a, 0.0)
    if kind.startswith("wall"):
        return (0.6 + 0.8 * a, 1.5 + b)                   # (u_n, u_t): D u_n below the effort limit, u_t > mu u_n
    return (0.5 + 0.3 * a, 0.65 + 0.15 * b)               # the obstacle's faces are short


# which forms' expected values depend on a field (every field of the arena but UNANCHORED appears)
FIELD_FORMS = {}
for _f in FORMS.values():
    for _k in _f.fields:
        FIELD_FORMS.setdefault(_k, []).append(_f.name)
FIELD_FORMS.setdefault("box_I", []).append("pair")      # the pair's angular momentum and energy: momenta()
FIELD_FORMS.setdefault("dyn_I", []).append("pair")
for _k in ("box_m", "dyn_m"):
    FIELD_FORMS[_k].append("pair")


def flat(values):
    """{quantity: array} -> one float64 vector, quantities in sorted order"""
    return np.concatenate([np.ravel(np.asarray(values[k], np.float64)) for k in sorted(values)])
