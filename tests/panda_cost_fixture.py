"""What the CPU and GPU tests of m3_set_panda_cost_weights share: the shapes, the weight tables, the oracle's first command of a
case with the observations of its own per-step worlds (computed once per case and kept read-only), and the restatement
(tests/panda_cost_ref.py) applied to them.

Shapes: K = 61 (no multiple of 4, 8 or 64: the last wavefront is partial in every kernel form), K = 62 for multi-modal (half =
31), T = 6; dt, substeps, bounds and noise scale as tests/panda_scene_fixture.py.

The pick fixture (pick_world, PICK_Q): the collision test of get_motion_cost has to be live in it, or the `collision` and `shelf_force`
weights would be compared on costs they never enter -- tests/test_panda_cost_weights_cpu.py asserts that on the oracle alone.
"""
import functools

import numpy as np

from tests import panda_cost_ref as R
from tests import panda_scene_fixture as X

F = np.float32
K, K_MM, T = 61, 62, 6
GOAL = X.GOAL
# the random table of the issue: rng.uniform(-5, 20, 7), as binary32 values; and the defaults with shelf_force = 3
RANDOM_TABLE = dict(zip(R.NAMES, (float(F(v)) for v in np.random.default_rng(20261019).uniform(-5, 20, 7))))
SHELF3_TABLE = {**R.DEFAULTS, "shelf_force": 3.0}
TABLES = {"random": RANDOM_TABLE, "shelf_force_3": SHELF3_TABLE}
# case name -> (task, gripper command, multi_modal, world)
CASES = {
    "reach": ("reach", 1, False, 36),
    "reach_mm": ("reach", 1, True, 36),
    "pick": ("pick", 2, False, None),        # world: pick_world() below
    "place": ("place", 1, False, 22),
}


def K_of(mm):
    return K_MM if mm else K


@functools.lru_cache(maxsize=4)
def delta_of(k):
    d = np.random.default_rng(1).standard_normal((k, T, 9)).astype(F)
    d.setflags(write=False)
    return d


# The pick case's start.  No fuzz world and not the "shelf" world puts a force on the shelf stand in a K = 61, T = 6 pick rollout
# (f_shelf is exactly zero in every (sample, step) pair of all 43 on the oracle), so the start is perturbed as the fixture
# conditions allow: the gripper of tests/panda_worlds.grasp_world, holding cubeA, with the arm moved (position-only inverse
# kinematics of the hand to (0.400, -0.040, shelf top + 0.100)) so that the held cube touches the front edge of the shelf
# stand's top.  Found by a grid search over such hand positions on the oracle for a start in which the collision indicator is
# live (23 % of the pairs at the default weights) and flips for at least one pair both at shelf_force = 3 and at the random
# table's shelf_force.  The joint angles of that start:
PICK_Q = (-0.3174741268157959, 1.3155889511108398, 0.7100721001625061, -0.6770659685134888, -0.7199498414993286,
          2.6360630989074707, -2.2519545555114746, 0.025000011548399925, 0.025000011548399925)


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


@functools.lru_cache(maxsize=1)
def pick_world():
    """The world of the pick case (above): grasp_world's held cube carried to the arm pose PICK_Q -- the cube's pose is the
    hand's composed with the grasp's relative pose; the grasp and sleep state are inferred from the geometry at the load, as for
    any world."""
    import oracle.panda as P
    from tests.panda_worlds import grasp_world
    sc = P.default_scene()
    w = grasp_world(P, sc, close_gripper=True).astype(F)
    rel_p = w[P.W_RELP:P.W_RELP + 3].astype(np.float64)
    rel_q = w[P.W_RELQ:P.W_RELQ + 4].astype(np.float64)
    q = np.array(PICK_Q, F)
    Lk = P.fk(sc, q)
    hand = {a: Lk[a][8].astype(np.float64) for a in ("pos", "ax", "ay", "az", "quat")}
    cq = _quat_mul(hand["quat"], rel_q)
    w[:9], w[9:18] = q, 0.0
    w[P.W_CUBEA:P.W_CUBEA + 3] = hand["pos"] + rel_p[0] * hand["ax"] + rel_p[1] * hand["ay"] + rel_p[2] * hand["az"]
    w[P.W_CUBEA + 3:P.W_CUBEA + 7] = cq / np.linalg.norm(cq)
    w[P.W_CUBEA + 7:P.W_CUBEA + 13] = 0.0
    w[P.W_HELD:] = 0.0                   # what a load from the 57 raw floats starts from: nothing derived
    w[P.W_RELQ + 3] = 1.0
    w[P.W_AWAKE:P.W_AWAKE + 2] = 1.0
    w.setflags(write=False)
    return w


def world_of(case):
    spec = CASES[case][3]
    return pick_world().copy() if spec is None else X.world_of(spec)


@functools.lru_cache(maxsize=None)
def oracle_case(case, scene_name=None):
    """The first command of an OraclePandaPlanner of the case (default weights, the named scene of panda_scene_fixture or the
    default): actions, states, cost_h, J as [K, T, ...], and obs [T, K, 30] -- oracle.panda.observe of the oracle's own worlds
    after each step of the same actions, with quirk Q8's cube0 / half0 columns filled from samples 0 and K / 2 of that step for
    reach (as tests/test_oracle_panda.py builds them).  Read-only."""
    import oracle.panda as P
    task, grip, mm, _ = CASES[case]
    k = K_of(mm)
    sc = X.oracle_scene(P, X.SCENES[scene_name] if scene_name else None)
    cfg = P.make_cfg(k, T, multi_modal=mm, task=task, goal=np.array(GOAL, F), gripper_cmd=grip)
    opl = P.OraclePandaPlanner(cfg, delta_of(k), sc)
    w0 = world_of(case)
    opl.command(w0)
    out = {n: np.array(opl.last[n]) for n in ("actions", "states", "cost_h", "J")}
    row = np.ascontiguousarray(np.asarray(w0, F).reshape(-1)[:P.WORLD_FLOATS]).copy()
    P.infer_state(sc, row)
    worlds = np.tile(row, (k, 1)).astype(F)
    obs = np.zeros((T, k, P.OBS_FLOATS), F)
    for t in range(T):
        P.step_batch(sc, worlds, np.ascontiguousarray(out["actions"][:, t]))
        o = np.stack([P.observe(sc, worlds[i]) for i in range(k)])
        if task == "reach":
            o[:, 17:20] = o[0, 10:13]
            o[:, 20:24] = o[0, 13:17]
            if mm:
                o[k // 2:, 20:24] = o[k // 2, 13:17]
        obs[t] = o
    out["obs"] = obs
    out["cfg"] = cfg
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def restated_cost_h(case, table=None, scene_name=None):
    """cost_horizon [K, T] of the case by the restatement with the weight table (None: the defaults)"""
    task, _, mm, _ = CASES[case]
    k = K_of(mm)
    ref = oracle_case(case, scene_name)
    w = R.weights(**(table or {}))
    return np.stack([R.cost_of_obs(task, ref["obs"][t], goal=np.array(GOAL, F), w=w, multi_modal=mm, half_K=k // 2)
                     for t in range(T)], axis=1).astype(F)


def oracle_cost_h_from_obs(case, scene_name=None):
    """the oracle's own cost of the same observations (default weights): what validates the replay"""
    import oracle.panda as P
    ref = oracle_case(case, scene_name)
    return np.stack([P.cost_obs(ref["cfg"], ref["obs"][t]) for t in range(T)], axis=1).astype(F)


def collision_pairs(case, table=None):
    """the collision indicator [K, T] of the case's (sample, step) pairs under the table's shelf_force"""
    ref = oracle_case(case)
    w = R.weights(**(table or {}))
    return np.stack([R.collision_indicator(ref["obs"][t][:, 24:26], ref["obs"][t][:, 26:28], ref["obs"][t][:, 28:30], w)
                     for t in range(T)], axis=1)
