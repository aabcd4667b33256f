"""Scene tables: the actors of the reference's two environments as plain data.

Values restate the reference's scene description files (they parameterise the kernels):
  point_env  src/m3p2i_aip/config/point_env/{0_point_robot,1..4_wall,5_obs,6_dyn_obs,7_box,
             8_goal,9_yaxis,10_xaxis}.yaml + assets/urdf/pointRobot.urdf
  panda_env  src/m3p2i_aip/config/panda_env/{1_table,2_table_stand,3_shelf_stand,4_obs,
             5_cubeA,6_cubeB,panda}.yaml + franka_panda.urdf link names

ACTOR ORDER.  The reference lists the yaml files with pathlib.iterdir() (actor_utils.py:97),
i.e. in filesystem order, and its suction model writes the robot reaction force to the LAST
rigid body of the env (skill_utils.py:89-90) -- so it only works when the robot is the last
actor.  This build fixes the order: non-robot actors in numeric file order, robot last.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional


@dataclass
class Actor:
    type: str                 # "box" | "robot"
    name: str
    size: List[float] = field(default_factory=lambda: [0.1, 0.1, 0.1])
    init_pos: List[float] = field(default_factory=lambda: [0.0, 0.0, 0.0])
    init_ori: List[float] = field(default_factory=lambda: [0.0, 0.0, 0.0, 1.0])
    fixed: bool = False
    collision: bool = True
    friction: float = 1.0
    gravity: bool = True
    links: List[str] = field(default_factory=lambda: ["box"])
    init_joint_pose: Optional[List[float]] = None
    handle: Optional[int] = None


S = 0.707107

POINT_ENV = [
    Actor("box", "wall-1", [0.1, 8, 0.2], [4.0, 0.0, 0.0], fixed=True),
    Actor("box", "wall-2", [0.1, 8, 0.2], [-4.0, 0.0, 0.0], fixed=True),
    Actor("box", "wall-3", [0.1, 8, 0.2], [0.0, 4.0, 0.0], [0.0, 0.0, S, S], fixed=True),
    Actor("box", "wall-4", [0.1, 8, 0.2], [0.0, -4.0, 0.0], [0.0, 0.0, S, S], fixed=True),
    Actor("box", "obs", [0.3, 0.4, 0.5], [2.0, 2.0, 0.0], fixed=True),
    Actor("box", "dyn-obs", [0.4, 0.4, 0.1], [-2.0, 2.0, 0.0]),
    Actor("box", "box", [0.4, 0.4, 0.1], [0.0, 2.0, 0.0], friction=0.5),
    Actor("box", "goal", [0.45, 0.45, 0.01], [-3.75, -3.75, 0.0], fixed=True, collision=False),
    Actor("box", "yaxis", [0.05, 0.5, 0.01], [0.0, 0.25, 0.01], fixed=True, collision=False),
    Actor("box", "xaxis", [0.5, 0.05, 0.01], [0.25, 0.0, 0.01], fixed=True, collision=False),
    Actor("robot", "point_robot", init_pos=[0.0, 0.0, 0.05], fixed=True, friction=0.05,
          links=["plane", "link_x", "link_y"]),
]

PANDA_LINKS = ["panda_link0", "panda_link1", "panda_link2", "panda_link3", "panda_link4",
               "panda_link5", "panda_link6", "panda_link7", "panda_hand", "panda_leftfinger",
               "panda_rightfinger"]

PANDA_ENV = [
    Actor("box", "table", [1.2, 1.2, 0.05], [0.0, 0.0, 1.0], fixed=True),
    Actor("box", "table_stand", [0.2, 0.2, 0.1], [-0.5, 0.0, 1.075], fixed=True),
    Actor("box", "shelf_stand", [0.2, 0.2, 0.3], [0.5, 0.0, 1.175], fixed=True),
    Actor("box", "dyn-obs", [0.2, 0.2, 0.02], [0.35, 0.0, 1.735], gravity=False),
    Actor("box", "cubeA", [0.05, 0.05, 0.05], [0.2, -0.2, 1.06]),
    Actor("box", "cubeB", [0.05, 0.05, 0.05], [0.2, 0.2, 1.06]),
    Actor("robot", "panda", init_pos=[-0.45, 0.0, 1.125], fixed=True, gravity=False,
          links=PANDA_LINKS,
          init_joint_pose=[0, 0, 0, 0, 0, 0, -2, 0, 0, 0, 1.8675, 0, 0, 0, 0.02, 0, 0.02, 0]),
]
CUBE_A_ON_SHELF = [0.425, 0.0, 1.35]

ENVS = {"point_env": POINT_ENV, "panda_env": PANDA_ENV}
DOFS = {"point_env": 2, "panda_env": 9}


def actor_index(env_type: str, name: str) -> int:
    return [a.name for a in ENVS[env_type]].index(name)


def body_index(env_type: str, actor: str, link: str) -> int:
    """Index of (actor, link) among the env's rigid bodies (DOMAIN_ENV numbering)."""
    b = 0
    for a in ENVS[env_type]:
        if a.name == actor:
            return b + a.links.index(link)
        b += len(a.links)
    raise ValueError(f"unknown actor {actor!r}")


def num_bodies(env_type: str) -> int:
    return sum(len(a.links) for a in ENVS[env_type])


# ---- the point_env arena as the dynamics see it (m3_point_scene; HipEngine.set_point_scene) ----
def mean_footprint_radius(a: float, b: float) -> float:
    """Mean distance of the points of an a x b rectangle from its centre (the lever arm of a box's ground friction, `*_req`):
    d/6 + a^2/(12 b) asinh(b/a) + b^2/(12 a) asinh(a/b) with d = sqrt(a^2 + b^2), in binary64."""
    import math
    d = math.hypot(a, b)
    return d / 6.0 + a * a / (12.0 * b) * math.asinh(b / a) + b * b / (12.0 * a) * math.asinh(a / b)


def point_scene_from_actors(actors) -> dict:
    """The fields of m3_point_scene (keys and order of _lib.POINT_SCENE_DEFAULTS) from an actor list shaped like POINT_ENV, by
    the rules the dynamics' scene constants were derived with:
      * half extents from `size`; the fixed obstacle's centre from `init_pos`;
      * `wall`: the inner face of the walls, |position| - half thickness -- the four walls must be symmetric about the origin
        (the dynamics know one `wall`), otherwise ValueError;
      * mass = 1000 kg/m^3 x volume (the yaml mass is not applied: isaacgym_wrapper.py:293-300), I = m ((2hx)^2 + (2hy)^2) / 12;
      * pair frictions: the average of the two actors' `friction`; the ground and the fixed actors are at 1.0;
      * `*_req` = mean_footprint_radius of the footprint.
    The robot's radius and mass come from its urdf, which an actor list does not carry: they keep their defaults.
    Every value is formed in binary64 and rounded once to binary32.  A derived value within two units in the last place of the
    literal default (the oracle forms box_I, dyn_I and *_req of the shipped arena in binary32, which can differ from the
    rounded binary64 value in the last bit) is PINNED to the literal, so that point_scene_from_actors(POINT_ENV) is the default
    arena bit for bit and the shipped scene stays on the default-scene kernels."""
    import numpy as np
    from ._lib import POINT_SCENE_DEFAULTS
    by = {a.name: a for a in actors}
    for need in ("box", "dyn-obs", "obs", "point_robot", "wall-1", "wall-2", "wall-3", "wall-4"):
        if need not in by:
            raise ValueError(f"point_scene_from_actors: no actor {need!r}")
    faces = []
    for name, axis in (("wall-1", 0), ("wall-2", 0), ("wall-3", 1), ("wall-4", 1)):
        w = by[name]
        if abs(w.init_pos[1 - axis]) > 1e-9:
            raise ValueError(f"point_scene_from_actors: {name} is not centred on its axis (the dynamics know one centred square)")
        faces.append(abs(w.init_pos[axis]) - 0.5 * w.size[0])
    signs = [by["wall-1"].init_pos[0] * by["wall-2"].init_pos[0], by["wall-3"].init_pos[1] * by["wall-4"].init_pos[1]]
    if max(faces) - min(faces) > 1e-9 or any(s >= 0 for s in signs):
        raise ValueError(f"point_scene_from_actors: the four walls are not symmetric about the origin (inner faces {faces}); "
                         "the dynamics know one `wall`")
    d = dict(POINT_SCENE_DEFAULTS)
    d["wall"] = faces[0]
    robot_mu = by["point_robot"].friction

    def pair(x, y):
        return 0.5 * (x + y)

    for key, name in (("box", "box"), ("dyn", "dyn-obs")):
        a = by[name]
        sx, sy, sz = a.size
        m = 1000.0 * sx * sy * sz
        d[f"{key}_hx"], d[f"{key}_hy"], d[f"{key}_m"] = 0.5 * sx, 0.5 * sy, m
        d[f"{key}_I"] = m * (sx * sx + sy * sy) / 12.0
        d[f"{key}_mu_g"] = pair(a.friction, 1.0)
        d[f"{key}_req"] = mean_footprint_radius(sx, sy)
    obs = by["obs"]
    d["obs_x"], d["obs_y"] = obs.init_pos[0], obs.init_pos[1]
    d["obs_hx"], d["obs_hy"] = 0.5 * obs.size[0], 0.5 * obs.size[1]
    fb, fd = by["box"].friction, by["dyn-obs"].friction
    d["mu_rb"], d["mu_rd"], d["mu_ro"], d["mu_rw"] = pair(robot_mu, fb), pair(robot_mu, fd), pair(robot_mu, 1.0), pair(robot_mu, 1.0)
    d["mu_bw"], d["mu_dw"], d["mu_bd"], d["mu_bo"], d["mu_do"] = pair(fb, 1.0), pair(fd, 1.0), pair(fb, fd), pair(fb, 1.0), pair(fd, 1.0)
    out = {}
    for n, lit in POINT_SCENE_DEFAULTS.items():
        v = float(np.float32(d[n]))
        if abs(v - lit) <= 2.0 * float(np.spacing(np.float32(abs(lit)))):
            v = lit
        out[n] = v
    return out


def spread_point_scenes(n, spread, seed=0, base=None, fields=("box_m", "box_mu_g", "mu_rb"), nominal_rows=()):
    """n arenas around `base` (field overrides over _lib.POINT_SCENE_DEFAULTS; None: the reference's arena), as override dicts for
    HipEngine.set_point_rollout_scenes / set_point_scene_rows / IsaacGymWrapper(point_scenes=...): each field of `fields` is
    base's value times a factor uniform in [1 - spread, 1 + spread]; box_I scales with box_m and dyn_I with dyn_m (the shape
    stays, as tools/band_stats.world_arena_of does it).  Row i depends on (seed, i) only, so a shard's rows are the slice of
    the global list.  Rows in `nominal_rows` are `base` unchanged -- a planner keeps its special samples (K - 1; multi-modal: 0
    and K / 2) on its nominal model that way."""
    import numpy as np
    from ._lib import POINT_SCENE_DEFAULTS
    spread = float(spread)
    if not 0.0 <= spread < 1.0:
        raise ValueError(f"spread_point_scenes: spread {spread!r} is not a share in [0, 1)")
    base = dict(base or {})
    fields = tuple(fields)
    unknown = sorted((set(base) | set(fields)) - set(POINT_SCENE_DEFAULTS))
    if unknown:
        raise ValueError(f"spread_point_scenes: unknown point scene field(s) {unknown}: one of {list(POINT_SCENE_DEFAULTS)}")
    full = {**POINT_SCENE_DEFAULTS, **{k: float(v) for k, v in base.items()}}
    follows = {"box_m": "box_I", "dyn_m": "dyn_I"}
    nominal = {int(i) % int(n) for i in nominal_rows} if n else set()
    rows = []
    for i in range(int(n)):
        row = dict(base)
        if i not in nominal and fields:
            f = np.random.default_rng([int(seed), i]).uniform(1.0 - spread, 1.0 + spread, len(fields))
            for name, fac in zip(fields, f):
                row[name] = full[name] * float(fac)
                if name in follows and follows[name] not in fields:
                    row[follows[name]] = full[follows[name]] * float(fac)
        rows.append(row)
    return rows


# ---- the panda_env workspace as the dynamics see it (m3_panda_scene; HipEngine.set_panda_scene) ----
PANDA_CUBE_SIZE = 0.05


def spread_panda_scenes(n, spread, seed=0, base=None, fields=("cube_m", "mu", "obs_m"), nominal_rows=()):
    """n workspaces around `base` (field overrides over _lib.PANDA_SCENE_DEFAULTS; None: the reference's workspace), as override
    dicts for HipEngine.set_panda_rollout_scenes / set_panda_scene_rows / IsaacGymWrapper(panda_scenes=...): each field of `fields`
    is base's value times a factor uniform in [1 - spread, 1 + spread] (an array field: every component by the field's one
    factor).  Row i depends on (seed, i) only, so a shard's rows are the slice of the global list.  Rows in `nominal_rows` are
    `base` unchanged -- a planner keeps its special samples (K - 1; the reach cost's 0 and K / 2, quirk Q8) on its nominal model
    that way.  The cube's size is no field (panda_scene_from_actors says why)."""
    import numpy as np
    from ._lib import PANDA_SCENE_DEFAULTS
    spread = float(spread)
    if not 0.0 <= spread < 1.0:
        raise ValueError(f"spread_panda_scenes: spread {spread!r} is not a share in [0, 1)")
    base = dict(base or {})
    fields = tuple(fields)
    unknown = sorted((set(base) | set(fields)) - set(PANDA_SCENE_DEFAULTS))
    if unknown:
        raise ValueError(f"spread_panda_scenes: unknown panda scene field(s) {unknown}: one of {list(PANDA_SCENE_DEFAULTS)}")
    full = {**PANDA_SCENE_DEFAULTS, **base}
    nominal = {int(i) % int(n) for i in nominal_rows} if n else set()
    rows = []
    for i in range(int(n)):
        row = dict(base)
        if i not in nominal and fields:
            f = np.random.default_rng([int(seed), i]).uniform(1.0 - spread, 1.0 + spread, len(fields))
            for name, fac in zip(fields, f):
                v = full[name]
                row[name] = tuple(float(x) * float(fac) for x in v) if isinstance(PANDA_SCENE_DEFAULTS[name], tuple) else float(v) * float(fac)
        rows.append(row)
    return rows


def panda_scene_from_actors(actors) -> dict:
    """The fields of m3_panda_scene (keys and order of _lib.PANDA_SCENE_DEFAULTS) from an actor list shaped like PANDA_ENV:
      * `table`, `shelf`: centre from `init_pos`, half extents from `size`; `obs_half` from the plate's `size`;
      * `base` from the robot's `init_pos`;
      * masses = 1000 kg/m^3 x volume, as point_scene_from_actors documents (so the plate keeps 0.8 unless its size says
        otherwise); cubeA and cubeB must agree -- the dynamics know one `cube_m` --, otherwise ValueError;
      * `mu`: the `friction` of the table, the shelf stand, the plate, the cubes and the robot, which must agree (the dynamics
        know one contact friction), otherwise ValueError.
    A cube `size` other than 0.05 is a ValueError: the cube's size is not part of m3_panda_scene, because the CPU oracle the
    kernels are held to bit for bit carries the cube's bounding radius as a literal, so another size could not be checked.
    `table_stand` is not part of the dynamics.  Every value is formed in binary64 and rounded once to binary32; a value within
    two units in the last place of the literal default is PINNED to the literal, so that panda_scene_from_actors(PANDA_ENV)
    is the default workspace bit for bit and the shipped scene stays on the default-scene kernels."""
    import numpy as np
    from ._lib import PANDA_SCENE_DEFAULTS
    by = {a.name: a for a in actors}
    for need in ("table", "shelf_stand", "dyn-obs", "cubeA", "cubeB", "panda"):
        if need not in by:
            raise ValueError(f"panda_scene_from_actors: no actor {need!r}")
    for name in ("cubeA", "cubeB"):
        if any(abs(float(x) - PANDA_CUBE_SIZE) > 1e-12 for x in by[name].size):
            raise ValueError(f"panda_scene_from_actors: {name} has size {list(by[name].size)}: the cube's size (0.05) is not part "
                             "of m3_panda_scene -- the oracle the kernels are checked against carries the cube's bounding radius "
                             "as a literal")
    vol = {n: float(np.prod([float(x) for x in by[n].size])) for n in ("cubeA", "cubeB", "dyn-obs")}
    if abs(vol["cubeA"] - vol["cubeB"]) > 1e-15:
        raise ValueError("panda_scene_from_actors: cubeA and cubeB differ in mass (the dynamics know one cube_m)")
    frictions = {n: float(by[n].friction) for n in ("table", "shelf_stand", "dyn-obs", "cubeA", "cubeB", "panda")}
    if len(set(frictions.values())) != 1:
        raise ValueError(f"panda_scene_from_actors: the actors' frictions differ ({frictions}); the dynamics know one contact "
                         "friction `mu`")

    def box6(a):
        return tuple(float(x) for x in a.init_pos) + tuple(0.5 * float(x) for x in a.size)

    d = dict(base=tuple(float(x) for x in by["panda"].init_pos), table=box6(by["table"]), shelf=box6(by["shelf_stand"]),
             obs_half=tuple(0.5 * float(x) for x in by["dyn-obs"].size), obs_m=1000.0 * vol["dyn-obs"],
             cube_m=1000.0 * vol["cubeA"], mu=frictions["table"])

    def pin(v, lit):
        v = float(np.float32(v))
        return lit if abs(v - lit) <= 2.0 * float(np.spacing(np.float32(abs(lit)))) else v

    return {n: tuple(pin(v, l) for v, l in zip(d[n], lit)) if isinstance(lit, tuple) else pin(d[n], lit)
            for n, lit in PANDA_SCENE_DEFAULTS.items()}


def panda_scene_is_default(scene) -> bool:
    """whether a mapping of panda scene fields (overrides; None) is the reference's workspace bit for bit in binary32"""
    from ._lib import PANDA_SCENE_DEFAULTS, panda_scene_fields
    return bytes(panda_scene_fields(scene)) == bytes(panda_scene_fields(PANDA_SCENE_DEFAULTS))
