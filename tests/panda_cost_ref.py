"""float32 numpy restatement of the three panda_env task costs with the seven weights of m3_panda_cost_weights as arguments.

Written from the reference's cost_functions.py:91-170 (get_panda_reach_cost, get_panda_pick_cost, get_panda_place_cost,
get_pick_tilt_cost, get_motion_cost's panda_env branch) and skill_utils.py:224-290 (get_general_ori_cube2goal,
get_general_ori_ee2cube), with the operation order of m3p2i_aip_amd/csrc/panda_dyn.hpp (panda_cost, ori_ee2cube,
ori_cube2goal, quat2mat): every line below is ONE binary32 operation per element (numpy keeps float32 operands in float32; its
sqrt, multiply, add and subtract are the correctly rounded IEEE ones), so a build of panda_dyn.hpp without contraction must
reproduce these values to the last bit.  A test helper, not a test: tests/test_panda_cost_weights_cpu.py pins it to the
reference's own values (tests/golden/ref_golden.npz, g6p_*) and to the oracle at the default weights.

Inputs are the fields oracle.panda.make_obs takes, arrays over n worlds: left [n, 3], left_q [n, 4] (xyzw), right [n, 3], cube
[n, 3], cube_q [n, 4], cube0 [n, 3] (quirk Q8: environment 0's cube), cube_q_half0 [n, 4] (the first environment of the
sample's half), f_table / f_shelf / f_cubeB [n, 2].  k: the global sample index of every world (default 0 .. n - 1).
"""
import numpy as np

F = np.float32
NAMES = ("reach_dist", "reach_tilt", "pick_goal", "pick_ori", "collision", "shelf_force", "place_grip")
DEFAULTS = dict(zip(NAMES, (10.0, 3.0, 10.0, 15.0, 1000.0, 4.0, 2.0)))
# the weights outside the collision test, per task: what scales the task's cost as a whole
OUTER = dict(reach=("reach_dist", "reach_tilt"), pick=("pick_goal", "pick_ori", "collision"), place=("place_grip",))


def weights(**kw):
    unknown = set(kw) - set(NAMES)
    assert not unknown, unknown
    return {n: F(kw.get(n, DEFAULTS[n])) for n in NAMES}


def weights_from(values):
    """the seven weights in field order"""
    values = list(values)
    assert len(values) == len(NAMES)
    return {n: F(v) for n, v in zip(NAMES, values)}


def _f(a):
    return np.asarray(a, dtype=F)


def quat2mat(q):
    """panda_dyn.hpp quat2mat: q [n, 4] (xyzw) -> the nine entries R[0..8], each [n]"""
    q = _f(q)
    q0, q1, q2, q3 = q[:, 3], q[:, 0], q[:, 1], q[:, 2]
    two, one = F(2), F(1)

    def diag(a):
        s = q0 * q0
        t = a * a
        s = s + t
        s = two * s
        return s - one

    def off(a, b, c, d, sign):
        s = a * b
        t = c * d
        s = s - t if sign < 0 else s + t
        return two * s

    return [diag(q1), off(q1, q2, q0, q3, -1), off(q1, q3, q0, q2, +1),
            off(q1, q2, q0, q3, +1), diag(q2), off(q2, q3, q0, q1, -1),
            off(q1, q3, q0, q2, -1), off(q2, q3, q0, q1, +1), diag(q3)]


def coldot(A, ca, B, cb):
    s = A[ca] * B[cb]
    t = A[3 + ca] * B[3 + cb]
    s = s + t
    t = A[6 + ca] * B[6 + cb]
    return s + t


def _one_minus_abs(x):
    return F(1) - np.abs(x)


def _min3(a, b, c):
    return np.minimum(np.minimum(a, b), c)


def ori_cube2goal(cube_q, goal_q):
    """get_general_ori_cube2goal (skill_utils.py:224-252) in ori_cube2goal's order"""
    C = quat2mat(cube_q)
    G = quat2mat(np.tile(_f(goal_q), (len(cube_q), 1)))
    cx = _min3(_one_minus_abs(coldot(G, 0, C, 0)), _one_minus_abs(coldot(G, 0, C, 1)), _one_minus_abs(coldot(G, 0, C, 2)))
    cy = _min3(_one_minus_abs(coldot(G, 1, C, 0)), _one_minus_abs(coldot(G, 1, C, 1)), _one_minus_abs(coldot(G, 1, C, 2)))
    return cx + cy


def ori_ee2cube(ee_q, cube_q, tilt, cube_q_half0):
    """get_general_ori_ee2cube (skill_utils.py:256-290) in ori_ee2cube's order; tilt [n]: 0 = the untilted term"""
    E, C, C0 = quat2mat(ee_q), quat2mat(cube_q), quat2mat(cube_q_half0)
    flat = _min3(_one_minus_abs(coldot(E, 2, C, 2)), _one_minus_abs(coldot(E, 2, C, 0)), _one_minus_abs(coldot(E, 2, C, 1)))
    sel = np.zeros(len(tilt), int)
    best = np.abs(C0[0])
    for j in (1, 2):
        more = np.abs(C0[j]) > best
        best = np.where(more, np.abs(C0[j]), best)
        sel = np.where(more, j, sel)
    d = np.where(sel == 0, coldot(E, 2, C, 0), np.where(sel == 1, coldot(E, 2, C, 1), coldot(E, 2, C, 2))).astype(F)
    tilted = np.abs(_f(tilt) - d)
    cost_z = np.where(_f(tilt) == 0, flat, tilted).astype(F)
    cost_y = _min3(_one_minus_abs(coldot(E, 1, C, 0)), _one_minus_abs(coldot(E, 1, C, 1)), _one_minus_abs(coldot(E, 1, C, 2)))
    return cost_z + cost_y


def _norm3(dx, dy, dz):
    s = dx * dx
    t = dy * dy
    s = s + t
    t = dz * dz
    s = s + t
    return np.sqrt(s)


def collision_indicator(f_table, f_shelf, f_cubeB, w):
    """get_motion_cost's test (cost_functions.py:158-170): |fx| + |fy| > 0.1 with shelf_force on the shelf stand's force"""
    f_table, f_shelf, f_cubeB = _f(f_table), _f(f_shelf), _f(f_cubeB)
    s = []
    for j in (0, 1):
        t = w["shelf_force"] * f_shelf[:, j]
        t = f_table[:, j] + t
        s.append(t + f_cubeB[:, j])
    coll = np.abs(s[0]) + np.abs(s[1])
    return coll > F(0.1)


def cost(task, left, left_q, right, cube, cube_q, cube0, cube_q_half0, f_table, f_shelf, f_cubeB, goal=None, w=None,
         multi_modal=False, half_K=0, k=None, pre_height_diff=0.05, tilt_cos_theta=0.5):
    """Objective.compute_cost of the panda_env with weights w (weights(...); None = the reference's literals)."""
    w = weights() if w is None else w
    left, right = _f(left), _f(right)
    n = len(left)
    k = np.arange(n) if k is None else np.asarray(k)
    if task == "reach":
        cube0 = _f(cube0)
        phd, tct = F(pre_height_diff), F(tilt_cos_theta)
        second = np.full(n, bool(multi_modal)) & (k >= half_K)
        gx_t = phd * tct
        gx_t = cube0[:, 0] - gx_t
        s = tct * tct
        s = F(1) - s
        s = np.sqrt(s)
        s = phd * s
        gz_t = cube0[:, 2] + s
        gz_f = cube0[:, 2] + phd
        gx = np.where(second, gx_t, cube0[:, 0]).astype(F)
        gz = np.where(second, gz_t, gz_f).astype(F)
        d = []
        for j, g in ((0, gx), (1, cube0[:, 1]), (2, gz)):
            e = left[:, j] + right[:, j]
            e = e / F(2)
            d.append(e - g)
        reach = _norm3(*d)
        tilt = np.where(second, tct, F(0)).astype(F)
        ori = ori_ee2cube(left_q, cube_q, tilt, cube_q_half0)
        a = w["reach_dist"] * reach
        b = w["reach_tilt"] * ori
        return (a + b).astype(F)
    if task == "pick":
        cube, goal = _f(cube), _f(goal)
        gc = _norm3(goal[0] - cube[:, 0], goal[1] - cube[:, 1], goal[2] - cube[:, 2])
        ori = ori_cube2goal(cube_q, goal[3:7])
        a = w["pick_goal"] * gc
        b = w["pick_ori"] * ori
        a = a + b
        pen = np.where(collision_indicator(f_table, f_shelf, f_cubeB, w), w["collision"], F(0)).astype(F)
        return (a + pen).astype(F)
    if task == "place":
        gap = _norm3(left[:, 0] - right[:, 0], left[:, 1] - right[:, 1], left[:, 2] - right[:, 2])
        gap = F(1) - gap
        return (w["place_grip"] * gap).astype(F)
    raise AssertionError(task)


def cost_of_obs(task, obs, **kw):
    """cost() on rows of oracle.panda.make_obs / observe ([n, 30])"""
    o = _f(obs)
    return cost(task, o[:, 0:3], o[:, 3:7], o[:, 7:10], o[:, 10:13], o[:, 13:17], o[:, 17:20], o[:, 20:24], o[:, 24:26],
                o[:, 26:28], o[:, 28:30], **kw)
