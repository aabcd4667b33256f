"""The point_env cost weights (m3_set_point_cost_weights) without a GPU.

1. tests/point_cost_ref.py, the float32 numpy restatement of the four costs with the nine weights as arguments, equals the
   reference's own values (g6_* / g7_* of tests/golden/ref_golden.npz) at the default weights, at the tolerance
   tests/test_oracle_golden.py uses for the same arrays, and is linear in the outer weights term by term.
2. A host build of the product's point_cost.hpp: the weighted form returns the literal form's BITS at the default weights,
   and the restatement's bits at random weights.  Bound: none -- every operation of both is a correctly rounded binary32
   add / multiply / divide / sqrt (numpy's float32 ufuncs and g++'s -O2 -ffp-contract=off code use the same SSE
   instructions; numpy evaluates float32 operands in float32), in the same order, so the values are equal to the last bit.
3. The Python plumbing: config parsing, unknown keys, non-finite weights, the ctypes declarations against the header.
"""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests import point_cost_ref as R
from tests.native_flags import host_flags

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST_FLAGS = ["-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]
F = np.float32
TASK_ID = {"navigation": 0, "push": 1, "pull": 2, "push_pull": 3}
KEYS = ["push_0", "pull_0", "push_pull_1", "navigation_0", "pull_1"]


def _golden_inputs(golden):
    return dict(robot=golden["g6_robot"], vel=golden["g6_vel"], box=golden["g6_box"], dynf=golden["g6_dynf"][:, :2])


# ------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("key", KEYS)
def test_restatement_equals_the_reference_at_default_weights(golden, key):
    task, mm = key.rsplit("_", 1)
    g = _golden_inputs(golden)
    K = len(g["robot"])
    goal = golden[f"g6_goal_{key}"]
    c = R.cost(task, goal=goal, multi_modal=bool(int(mm)), half_K=K // 2, **g)
    np.testing.assert_allclose(c, golden[f"g6_cost_{key}"], rtol=2e-6, atol=1e-5)      # (test_oracle_golden.py's tolerance)
    if f"g7_fbox_{key}" in golden:
        # K > 1: threshold 1.8 (skill_utils.py:75-82); kp_suction of the golden run: read back from the forces' magnitude
        fb = golden[f"g7_fbox_{key}"]
        kp = float(np.round(np.abs(np.hypot(fb[:, 0], fb[:, 1])).max()))
        p = R.pending(task, g["robot"], g["vel"], g["box"], kp, 1.8, multi_modal=bool(int(mm)), half_K=K // 2)
        np.testing.assert_allclose(p[:, 2:4], fb, rtol=1e-6, atol=1e-4)
        np.testing.assert_allclose(p[:, 0:2], golden[f"g7_frobot_{key}"], rtol=1e-6, atol=1e-4)


def test_restatement_is_linear_in_the_outer_weights(golden):
    g = _golden_inputs(golden)
    rng = np.random.default_rng(5)
    w = R.weights(**{n: float(F(v)) for n, v in zip(R.NAMES, rng.uniform(-4, 12, 9))})
    goal = golden["g6_goal_push_0"]
    d, m = R.nav_terms(g["robot"], goal, g["dynf"], w)
    np.testing.assert_array_equal(R.cost("navigation", goal=goal, w=w, **g), w["nav_dist"] * d + m)
    assert set(np.unique(m)) <= {F(0.0), w["collision"]} and 0 < (m != 0).sum() < m.size
    dc, al = R.push_terms(g["robot"], g["box"], goal, w)
    np.testing.assert_array_equal(R.cost("push", goal=goal, w=w, **g), w["push_dist"] * dc + w["push_align"] * al)
    dc, vc, al, _, _ = R.pull_terms(g["robot"], g["vel"], g["box"], goal, w)
    np.testing.assert_array_equal(R.cost("pull", goal=goal, w=w, **g),
                                  w["pull_dist"] * dc + w["pull_vel"] * vc + w["pull_align"] * al)
    assert set(np.unique(vc)) <= {F(0.0), F(0.6)}
    # each outer weight on its own: the cost with only that weight non-zero is weight * term
    for name, term in (("push_dist", dc), ("push_align", R.push_terms(g["robot"], g["box"], goal, w)[1])):
        only = dict(w, push_dist=F(0), push_align=F(0))
        only[name] = w[name]
        np.testing.assert_array_equal(R.cost("push", goal=goal, w=only, **g), (w[name] * term + F(0)).astype(F))
    # the inner pair: dist_cost = robot_box * d1 + d2 * box_goal
    d1, d2, _ = R.dist_terms(g["robot"], g["box"], goal)
    np.testing.assert_array_equal(dc, w["robot_box"] * d1 + d2 * w["box_goal"])
    # avoid_dyn_obs adds the motion term
    np.testing.assert_array_equal(R.cost("push", goal=goal, w=w, avoid_dyn_obs=True, **g),
                                  R.cost("push", goal=goal, w=w, **g) + m)


# ------------------------------------------------------------------ 2. the host build of point_cost.hpp
@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("point_cost") / "libpoint_cost_host.so")
    subprocess.check_call(["g++"] + host_flags(HOST_FLAGS) + ["-I" + os.path.join(HERE, "native", "shim"),
                           os.path.join(HERE, "native", "point_cost_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.pch_cost.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                             C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.pch_cost.restype = None
    return lib


def random_cost_worlds(n, rng):
    """rows of 8: robot x y vx vy | box x y | dyn-obs force x y -- built so that every branch of the costs is taken by a
    good share of the rows: cos_theta of either sign, robot moving toward / away from the box, |box - robot| on either side
    of 0.5 (the pull's velocity term) and of 1 / 1.8 (the suction mask), dyn-obs contact on / off."""
    w = np.zeros((n, 8), F)
    w[:, 4:6] = rng.uniform(-3.5, 3.5, (n, 2))
    r = np.where(rng.random(n) < 0.5, rng.uniform(0.2, 0.7, n), rng.uniform(0.7, 4.0, n))
    th = rng.uniform(-np.pi, np.pi, n)
    w[:, 0] = w[:, 4] + r * np.cos(th)
    w[:, 1] = w[:, 5] + r * np.sin(th)
    w[:, 2:4] = rng.normal(0, 1, (n, 2))
    f = rng.normal(0, 5, (n, 2))
    f[rng.random(n) < 0.5] = 0.0
    f[rng.random(n) < 0.1] *= 0.005
    w[:, 6:8] = f
    return w


def host_cost(lib, worlds, task, wt, goal, multi_modal=False, half_K=0, kp=400.0, thresh=1.8, avoid=False, k0=0):
    n = len(worlds)
    worlds = np.ascontiguousarray(worlds, F)
    cost = np.zeros(n, F)
    pend = np.full((n, 4), 12345.0, F)
    arr = None if wt is None else np.array([wt[k] for k in R.NAMES], F)
    lib.pch_cost(int(wt is not None), None if arr is None else arr.ctypes.data, TASK_ID[task], int(multi_modal), half_K,
                 float(goal[0]), float(goal[1]), kp, thresh, int(avoid), worlds.ctypes.data, n, k0, cost.ctypes.data,
                 pend.ctypes.data)
    return cost, pend


CASES = [("navigation", False, False), ("push", False, False), ("pull", False, False), ("push_pull", True, False),
         ("push", False, True), ("pull", True, True), ("push_pull", True, True)]


def _branches_covered(worlds, goal):
    g = dict(robot=worlds[:, 0:2], vel=worlds[:, 2:4], box=worlds[:, 4:6])
    _, _, cos_theta = R.dist_terms(g["robot"], g["box"], goal)
    _, _, _, toward, rdist = R.pull_terms(g["robot"], g["vel"], g["box"], goal, R.weights())
    coll = np.abs(worlds[:, 6]) + np.abs(worlds[:, 7]) > F(0.1)
    mask = F(1.0) / rdist > F(1.8)
    for flag in (cos_theta > 0, toward, rdist <= F(0.5), mask, coll, toward & (rdist <= F(0.5)), mask & ~toward):
        assert 0.03 < flag.mean() < 0.97, flag.mean()


@pytest.mark.parametrize("task,mm,avoid", CASES)
def test_weighted_form_returns_the_literal_forms_bits_at_default_weights(host_lib, task, mm, avoid):
    rng = np.random.default_rng(11)
    n, goal = 4096, (-1.0, 0.5)
    worlds = random_cost_worlds(n, rng)
    _branches_covered(worlds, goal)
    kw = dict(goal=goal, multi_modal=mm, half_K=n // 2, avoid=avoid)
    c0, p0 = host_cost(host_lib, worlds, task, None, **kw)
    c1, p1 = host_cost(host_lib, worlds, task, R.weights(), **kw)
    assert c0.tobytes() == c1.tobytes() and p0.tobytes() == p1.tobytes()
    assert np.isfinite(c0).all()


@pytest.mark.parametrize("task,mm,avoid", CASES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_host_build_equals_the_restatement_at_random_weights(host_lib, task, mm, avoid, seed):
    rng = np.random.default_rng([seed, TASK_ID[task]])
    n, goal = 2048, tuple(rng.uniform(-3, 3, 2))
    worlds = random_cost_worlds(n, rng)
    vals = rng.uniform(-5, 20, 9)
    vals[rng.integers(0, 9)] = 0.0             # zero and negative weights are legal
    vals[rng.integers(0, 9)] = -abs(vals[0]) - 0.5
    wt = R.weights(**dict(zip(R.NAMES, map(float, vals.astype(F)))))
    k0 = 100 if seed == 2 else 0              # (a shard: global sample indices start at k_offset)
    half = n // 2 + k0
    c, p = host_cost(host_lib, worlds, task, wt, goal=goal, multi_modal=mm, half_K=half, avoid=avoid, k0=k0)
    g = dict(robot=worlds[:, 0:2], vel=worlds[:, 2:4], box=worlds[:, 4:6], dynf=worlds[:, 6:8])
    k = np.arange(k0, k0 + n)
    ref = R.cost(task, goal=np.array(goal, F), w=wt, multi_modal=mm, half_K=half, k=k, avoid_dyn_obs=avoid, **g)
    assert c.tobytes() == ref.astype(F).tobytes()                      # the bound of this file's docstring: none
    pr = R.pending(task, g["robot"], g["vel"], g["box"], 400.0, 1.8, multi_modal=mm, half_K=half, k=k)
    if pr is None:
        assert (p == F(12345.0)).all()                                 # no suction staged: the pending force is left alone
    else:
        assert p.tobytes() == pr.tobytes()
        # ... and the weights do not touch it
        assert p.tobytes() == host_cost(host_lib, worlds, task, None, goal=goal, multi_modal=mm, half_K=half, avoid=avoid,
                                        k0=k0)[1].tobytes()


# ------------------------------------------------------------------ 3. Python plumbing
def _cfg(**kw):
    mppi = types.SimpleNamespace(num_samples=64, device="cpu")
    return types.SimpleNamespace(multi_modal=False, mppi=mppi, task="push", goal=[-1.0, -1.0], **kw)


def test_objective_reads_cost_weights_from_the_config():
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.cost_functions import Objective
    o = Objective(_cfg())
    assert o.cost_weights == L.COST_WEIGHT_DEFAULTS and o.has_default_cost_weights
    o = Objective(_cfg(cost_weights={"push_align": 2.5, "box_goal": 0}))
    assert o.cost_weights == {**L.COST_WEIGHT_DEFAULTS, "push_align": 2.5, "box_goal": 0.0} and not o.has_default_cost_weights
    o.set_cost_weights(push_align=1.0, box_goal=10)
    assert o.has_default_cost_weights
    with pytest.raises(ValueError, match="push_alignment"):
        Objective(_cfg(cost_weights={"push_alignment": 2.0}))
    with pytest.raises(ValueError, match="pull_vel is not finite"):
        o.set_cost_weights(pull_vel=float("nan"))
    with pytest.raises(ValueError, match="point_env only"):
        Objective(_cfg(cost_weights={"push_align": 2.0}, env_type="panda_env"))
    assert tuple(L.COST_WEIGHT_DEFAULTS) == R.NAMES and L.COST_WEIGHT_DEFAULTS == R.DEFAULTS


def test_compat_config_passes_the_key_through():
    from m3p2i_aip_amd import compat
    from m3p2i_aip_amd.cost_functions import Objective
    cfg = compat.make_config("config_point", ["cost_weights={push_align: 2.5, pull_vel: -1}"])
    assert cfg.cost_weights == {"push_align": 2.5, "pull_vel": -1}
    assert Objective(cfg).cost_weights["pull_vel"] == -1.0
    assert compat.make_config("config_point").cost_weights is None


class _StubEngine:
    """What Objective.push_cost_weights and the planner see of an engine; refuses as the library does."""

    def __init__(self):
        self.pushed = []

    def set_point_cost_weights(self, w):
        from m3p2i_aip_amd import _lib as L
        for k, v in w.items():
            if not np.isfinite(v):
                raise L.M3Error(f"m3p2i_hip error -1: m3_set_point_cost_weights: {k} is not finite")
        self.pushed.append(dict(w))


def test_weights_are_pushed_only_when_they_differ_from_what_the_engine_holds():
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.cost_functions import Objective
    o, eng = Objective(_cfg()), _StubEngine()
    o.push_cost_weights(eng)
    assert eng.pushed == []                              # defaults on a fresh engine: no call
    o.push_cost_weights(object())                        # ... so an engine without the method serves such an Objective
    o.set_cost_weights(push_align=2.5)
    o.push_cost_weights(eng)
    o.push_cost_weights(eng)
    assert len(eng.pushed) == 1 and eng.pushed[0]["push_align"] == 2.5
    with pytest.raises(TypeError, match="set_point_cost_weights"):
        o.push_cost_weights(object())
    o.set_cost_weights(push_align=1.0)
    o.push_cost_weights(eng)                             # back to the defaults: the engine must learn it
    assert len(eng.pushed) == 2 and eng.pushed[1] == L.COST_WEIGHT_DEFAULTS
    o._cost_weights["pull_dist"] = float("inf")          # (past the Objective's own check: the library's refusal surfaces)
    with pytest.raises(L.M3Error, match="pull_dist is not finite"):
        o.push_cost_weights(eng)


def test_ctypes_declarations_match_the_header():
    from m3p2i_aip_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    m = re.search(r"typedef struct m3_point_cost_weights \{(.*?)\} m3_point_cost_weights;", hdr, re.S)
    fields = re.findall(r"float\s+(\w+);\s*/\*\s*([0-9.]+)", m.group(1))
    assert [f for f, _ in fields] == [n for n, _ in L.PointCostWeights._fields_] == list(R.NAMES)
    assert {f: float(v) for f, v in fields} == L.COST_WEIGHT_DEFAULTS
    assert C.sizeof(L.PointCostWeights) == 36 and all(t is C.c_float for _, t in L.PointCostWeights._fields_)
    bound = {n: (r, a) for n, r, a in L.SYMBOLS}
    P = C.POINTER(L.PointCostWeights)
    assert bound["m3_default_point_cost_weights"] == (None, [P])
    assert bound["m3_set_point_cost_weights"] == (C.c_int, [C.c_void_p, P])
    assert bound["m3_get_point_cost_weights"] == (C.c_int, [C.c_void_p, P])
    assert bound["m3_set_weighted_cost_instance"] == (C.c_int, [C.c_void_p, C.c_int])
    for name in bound:
        if "cost_weight" in name or "weighted_cost" in name:
            assert re.search(r"\b%s\s*\(" % name, hdr), name
    # host-only entry points: the library's defaults are the header's, and a NULL handle is refused
    lib = L.load()
    w = L.PointCostWeights()
    lib.m3_default_point_cost_weights(C.byref(w))
    assert {n: getattr(w, n) for n in R.NAMES} == L.COST_WEIGHT_DEFAULTS
    assert lib.m3_set_point_cost_weights(None, C.byref(w)) < 0 and lib.m3_get_point_cost_weights(None, C.byref(w)) < 0
    assert lib.m3_set_weighted_cost_instance(None, 1) < 0
