"""The run-time point_env arena (m3_set_point_scene) without a GPU.

1. A host build of the product's planar_dyn.hpp through PointSceneRT (tests/native/point_scene_host.cpp): the device source
   with the arena as run-time values equals oracle.step_batch with the same arena BIT FOR BIT -- at the default values, at the
   custom arena of tests/point_scene_fixture.py, and with each of the 28 fields varied alone; the compile-time scene type
   gives the same bits as the run-time one at the default values.  Bound: none (the spec is a fixed sequence of binary32
   operations; tests/test_device_dynamics_on_host.py holds the default scene to the same standard).
2. The broad-phase radii are upper bounds of the boxes' half diagonals, evaluated in binary64.
3. Plumbing: header <-> ctypes layout, the defaults against the oracle's, scenes.point_scene_from_actors, the config key.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from m3p2i_aip_amd import _lib as L
from tests import point_scene_fixture as X
from tests.native_flags import host_flags
from tests.test_device_dynamics_on_host import HOST_FLAGS, fma_flag

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
# robot (c, s, w) do not exist on the device
COLS_STEP = [c for c in range(31) if c not in (2, 3, 6)]
COLS_ROLL = [c for c in range(25) if c not in (2, 3, 6)] + [29, 30]


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("point_scene") / "libpoint_scene_host.so")
    subprocess.check_call(["g++"] + host_flags(HOST_FLAGS) + fma_flag() + ["-I" + os.path.join(HERE, "native", "shim"),
                           os.path.join(HERE, "native", "point_scene_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    VP = C.c_void_p
    lib.psh_step_rt.argtypes = [VP, C.c_float, C.c_int, C.c_int, VP, C.c_int, VP, C.c_int]
    lib.psh_step_ct.argtypes = [C.c_float, C.c_int, C.c_int, VP, C.c_int, VP, C.c_int]
    lib.psh_default_scene.argtypes = [VP]
    lib.psh_radii.argtypes = [VP, VP]
    lib.psh_bounding_radius.argtypes = [C.c_float, C.c_float]
    lib.psh_bounding_radius.restype = C.c_float
    return lib


def worlds_near_contacts(O, n, rng, sd):
    """random worlds drawn next to the contacts of arena `sd`: bodies at its walls and corners, at its obstacle, at each
    other; rotated, moving, with pending forces"""
    w = O.init_world(n)
    wall, ox, oy = sd["wall"], sd["obs_x"], sd["obs_y"]

    def place(k):
        p = rng.uniform(-wall + 0.1, wall - 0.1, (k, 2))
        spot = rng.integers(0, 3, k)
        for i in range(k):
            if spot[i] == 1:
                p[i, rng.integers(0, 2)] = rng.choice([-1, 1]) * rng.uniform(wall - 0.5, wall - 0.1)
                if rng.random() < 0.5:
                    p[i] = rng.choice([-1, 1], 2) * rng.uniform(wall - 0.55, wall - 0.15, 2)
            elif spot[i] == 2:
                p[i] = np.array([ox, oy]) + rng.uniform(-0.6, 0.6, 2)
        return p

    w[:, 0:2] = place(n)
    w[:, 4:6] = rng.normal(0, 1, (n, 2))
    for base in (O.W_B, O.W_D):
        yaw = rng.uniform(-np.pi, np.pi, n)
        p = place(n)
        near = rng.random(n) < 0.5      # next to the robot
        p[near] = w[near, 0:2] + rng.uniform(-0.55, 0.55, (int(near.sum()), 2))
        w[:, base:base + 2] = p
        w[:, base + 2], w[:, base + 3] = np.cos(yaw), np.sin(yaw)
        mv = rng.random(n) < 0.5
        w[mv, base + 4:base + 6] = rng.normal(0, 0.5, (int(mv.sum()), 2))
        w[mv, base + 6] = rng.normal(0, 1, int(mv.sum()))
    w[:, O.W_FEXT_B:O.W_FEXT_B + 2] = rng.normal(0, 100, (n, 2)) * (rng.random((n, 1)) < 0.3)
    w[:, O.W_FEXT_R:O.W_FEXT_R + 2] = rng.normal(0, 100, (n, 2)) * (rng.random((n, 1)) < 0.3)
    return w.astype(F)


def run_both(O, lib, worlds, overrides, steps, mode, seed=0, ct=False):
    """`steps` steps of `worlds` on the oracle and on the host build; asserts equal bits after every step; returns the
    oracle's final worlds"""
    rng = np.random.default_rng(seed)
    a, b = worlds.copy(), worlds.copy()
    sc = X.oracle_scene(O, overrides)
    arr = X.scene_array(overrides)
    cols = COLS_STEP if mode == 0 else COLS_ROLL
    for t in range(steps):
        u = rng.uniform(-3, 3, (len(a), 2)).astype(F)
        O.step_batch(sc, a, u)
        if ct:
            lib.psh_step_ct(0.05, 2, 6, b.ctypes.data, len(b), u.ctypes.data, mode)
        else:
            lib.psh_step_rt(arr.ctypes.data, 0.05, 2, 6, b.ctypes.data, len(b), u.ctypes.data, mode)
        neq = a[:, cols].view(np.uint32) != b[:, cols].view(np.uint32)
        if neq.any():
            r, c = np.argwhere(neq)[0]
            raise AssertionError(f"step {t} world {r} column {cols[c]}: oracle {a[r, cols[c]]!r} device-source {b[r, cols[c]]!r} "
                                 f"({int(neq.sum())} values differ)")
    return a


SCENES = {"default": None, "custom": X.CUSTOM, "custom_b": X.CUSTOM_B}


@pytest.mark.parametrize("mode", [0, 1], ids=["step_mode", "rollout_dispatch"])
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("steps", [1, 8])
def test_three_worlds_equal_the_oracle(oracle, host_lib, name, steps, mode):
    run_both(oracle, host_lib, X.start_worlds(oracle), SCENES[name], steps, mode)


@pytest.mark.parametrize("mode", [0, 1], ids=["step_mode", "rollout_dispatch"])
@pytest.mark.parametrize("name", list(SCENES))
def test_random_worlds_next_to_contacts_equal_the_oracle(oracle, host_lib, name, mode):
    sd = X.scene_dict(SCENES[name])
    w = worlds_near_contacts(oracle, 2000, np.random.default_rng(3), sd)
    a1 = run_both(oracle, host_lib, w, SCENES[name], 1, mode)
    a = run_both(oracle, host_lib, w, SCENES[name], 8, mode)
    # (the worlds really are in contact: robot, box and dyn-obs feel contact forces in a good share of them)
    assert (np.abs(a1[:, 29:31]).sum(1) > 0).sum() > 200 and (np.abs(a[:, 29:31]).sum(1) > 0).sum() > 100


def test_the_custom_arena_changes_the_dynamics(oracle):
    """the condition of every scene case: on the oracle alone, the custom arena moves at least a quarter of the samples"""
    w = np.repeat(X.start_worlds(oracle), 64, axis=0)
    rng = np.random.default_rng(1)
    a, b = w.copy(), w.copy()
    for t in range(8):
        u = rng.uniform(-3, 3, (len(w), 2)).astype(F)
        oracle.step_batch(X.oracle_scene(oracle, X.CUSTOM), a, u)
        oracle.step_batch(X.oracle_scene(oracle), b, u)
    differs = (a[:, COLS_ROLL].view(np.uint32) != b[:, COLS_ROLL].view(np.uint32)).any(1).reshape(3, 64).mean(1)
    assert (differs >= 0.25).all(), differs


@pytest.mark.parametrize("mode", [0, 1], ids=["step_mode", "rollout_dispatch"])
def test_compile_time_scene_equals_run_time_scene_at_the_defaults(oracle, host_lib, mode):
    w = np.concatenate([X.start_worlds(oracle), worlds_near_contacts(oracle, 1500, np.random.default_rng(4), X.scene_dict())])
    a = run_both(oracle, host_lib, w, None, 8, mode, ct=True)
    b = run_both(oracle, host_lib, w, None, 8, mode, ct=False)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("field", X.FIELDS)
def test_each_field_alone(oracle, host_lib, field):
    """one field varied, everything else at the default: bit-equal to the oracle with that field varied, at a world in which
    every pair is in or next to contact in the default arena's corner (positions are moved with the obstacle / wall)"""
    base = L.POINT_SCENE_DEFAULTS[field]
    value = {"obs_x": 1.8, "obs_y": 2.3, "wall": 3.0}.get(field, base * 1.25 if not field.startswith("mu") else base * 0.6 + 0.05)
    ov = {field: float(F(value))}
    sd = X.scene_dict(ov)
    w = worlds_near_contacts(oracle, 600, np.random.default_rng(7), sd)
    a = run_both(oracle, host_lib, w, ov, 6, 0)
    run_both(oracle, host_lib, w, ov, 6, 1)
    ref = w.copy()       # ... and the field does something: the default arena gives other bits
    rng = np.random.default_rng(0)
    sc0 = X.oracle_scene(oracle)
    for t in range(6):
        oracle.step_batch(sc0, ref, rng.uniform(-3, 3, (len(ref), 2)).astype(F))
    assert (a.view(np.uint32) != ref.view(np.uint32)).any(), field


# ------------------------------------------------------------------ 2. broad-phase radii
def test_bounding_radii_are_upper_bounds(host_lib):
    rng = np.random.default_rng(11)
    h = np.concatenate([rng.uniform(1e-3, 3.0, (4000, 2)), 10.0 ** rng.uniform(-6, 3, (1000, 2))]).astype(F)
    for hx, hy in h:
        r = host_lib.psh_bounding_radius(float(hx), float(hy))
        assert float(r) >= np.sqrt(float(hx) ** 2 + float(hy) ** 2), (hx, hy, r)
    out = np.zeros(3, F)
    arr = X.scene_array(X.CUSTOM)
    host_lib.psh_radii(arr.ctypes.data, out.ctypes.data)
    d = X.scene_dict(X.CUSTOM)
    for r, (hx, hy) in zip(out, (("box_hx", "box_hy"), ("dyn_hx", "dyn_hy"), ("obs_hx", "obs_hy"))):
        hx, hy = float(F(d[hx])), float(F(d[hy]))
        assert float(r) >= np.sqrt(hx * hx + hy * hy) and float(r) < np.sqrt(hx * hx + hy * hy) + 2e-4


# ------------------------------------------------------------------ 3. plumbing
def test_header_and_ctypes_layout_agree(host_lib):
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    m = re.search(r"typedef struct m3_point_scene \{(.*?)\} m3_point_scene;", hdr, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("float", "").split(",")]
    assert names == X.FIELDS == [f[0] for f in L.PointSceneFields._fields_]
    assert all(f[1] is C.c_float for f in L.PointSceneFields._fields_)
    assert C.sizeof(L.PointSceneFields) == 4 * len(names) == 4 * host_lib.psh_scene_floats() == 112
    assert "#define M3_ABI_VERSION 4" in hdr
    bound = {s[0]: (s[1], list(s[2])) for s in L.SYMBOLS}
    P = C.POINTER(L.PointSceneFields)
    assert bound["m3_default_point_scene"] == (None, [P])
    assert bound["m3_set_point_scene"] == (C.c_int, [L._H, P]) and bound["m3_get_point_scene"] == (C.c_int, [L._H, P])
    assert bound["m3_set_point_scene_instance"] == (C.c_int, [L._H, C.c_int])
    for name in ("m3_default_point_scene", "m3_set_point_scene", "m3_get_point_scene", "m3_set_point_scene_instance"):
        assert re.search(r"^\w+\s+%s\(" % name, hdr, re.M), name


def test_defaults_equal_the_oracles_field_by_field(oracle, host_lib):
    sc = oracle.default_scene()
    want = np.array([getattr(sc, n) for n in X.FIELDS], F)
    got = np.zeros(len(X.FIELDS), F)
    host_lib.psh_default_scene(got.ctypes.data)           # the constant m3_default_point_scene copies
    lib_sc = L.PointSceneFields()
    L.load().m3_default_point_scene(C.byref(lib_sc))      # the library's entry point itself
    from_lib = np.array([getattr(lib_sc, n) for n in X.FIELDS], F)
    table = X.scene_array()                               # _lib.POINT_SCENE_DEFAULTS
    for i, n in enumerate(X.FIELDS):
        assert want[i:i + 1].view(np.uint32)[0] == got[i:i + 1].view(np.uint32)[0] == from_lib[i:i + 1].view(np.uint32)[0] \
            == table[i:i + 1].view(np.uint32)[0], n


def test_null_handle_and_bad_switch_are_refused():
    lib = L.load()
    sc = L.PointSceneFields()
    assert lib.m3_set_point_scene(None, C.byref(sc)) == -1 and lib.m3_get_point_scene(None, C.byref(sc)) == -1
    assert lib.m3_set_point_scene_instance(None, 1) == -1


def test_scene_from_actors_returns_the_literal_defaults():
    from m3p2i_aip_amd import scenes
    d = scenes.point_scene_from_actors(scenes.POINT_ENV)
    assert list(d) == X.FIELDS
    np.testing.assert_array_equal(np.array([d[n] for n in X.FIELDS], F).view(np.uint32), X.scene_array().view(np.uint32))


def test_scene_from_actors_rules():
    import copy
    from m3p2i_aip_amd import scenes
    actors = copy.deepcopy(scenes.POINT_ENV)
    by = {a.name: a for a in actors}
    by["obs"].init_pos = [-1.0, 0.5, by["obs"].init_pos[2]]
    by["obs"].size = [0.5, 0.2, by["obs"].size[2]]
    by["box"].size = [0.6, 0.3, 0.05]
    by["box"].friction = 0.3
    d = scenes.point_scene_from_actors(actors)
    assert (d["obs_x"], d["obs_y"]) == (-1.0, 0.5) and F(d["obs_hx"]) == F(0.25) and F(d["obs_hy"]) == F(0.1)
    assert F(d["box_hx"]) == F(0.3) and F(d["box_hy"]) == F(0.15)
    m = 1000.0 * 0.6 * 0.3 * 0.05
    assert F(d["box_m"]) == F(m) and F(d["box_I"]) == F(m * (0.6 ** 2 + 0.3 ** 2) / 12.0)
    assert F(d["box_mu_g"]) == F((0.3 + 1.0) / 2) and F(d["mu_bw"]) == F((0.3 + 1.0) / 2) and F(d["mu_bd"]) == F((0.3 + 1.0) / 2)
    assert F(d["mu_rb"]) == F((0.05 + 0.3) / 2)
    assert F(d["box_req"]) == F(scenes.mean_footprint_radius(0.6, 0.3))


def test_mean_footprint_radius_closed_form():
    from m3p2i_aip_amd import scenes
    assert abs(scenes.mean_footprint_radius(0.4, 0.4) - 0.3825978 * 0.4) <= 1e-6 * 0.3825978 * 0.4
    for a, b in ((0.4, 0.4), (0.6, 0.3), (0.1, 1.0), (2.0, 0.5)):     # midpoint quadrature, 800 x 800 cells: error O(h^2)
        n = 800
        x = (np.arange(n) + 0.5) / n * a - a / 2
        y = (np.arange(n) + 0.5) / n * b - b / 2
        q = np.hypot(x[:, None], y[None, :]).mean()
        assert abs(scenes.mean_footprint_radius(a, b) - q) < 1e-5 * max(a, b), (a, b)


def test_asymmetric_walls_are_refused():
    import copy
    from m3p2i_aip_amd import scenes
    actors = copy.deepcopy(scenes.POINT_ENV)
    wall = next(a for a in actors if a.name == "wall-3")
    wall.init_pos = [p * 0.5 for p in wall.init_pos]
    with pytest.raises(ValueError):
        scenes.point_scene_from_actors(actors)


def test_point_scene_config_key_through_compat():
    from m3p2i_aip_amd import compat
    cfg = compat.make_config("config_point", ["point_scene={obs_x: -1.0, wall: 2.95}"])
    assert dict(cfg.point_scene) == {"obs_x": -1.0, "wall": 2.95}
    assert compat.make_config("config_point").point_scene is None


# ------------------------------------------------------------------ 4. the rollout plan (host only)
def _plan(task, mm, scene=0, weighted=0, form_request=0, K=2000, T=30, lanes=64, dt=0.05, substeps=2, iters=6, minima=0, **kw):
    out = (C.c_int * 8)()
    rc = L.load().m3_point_rollout_plan(task, int(mm), kw.get("mode_simple", 0), kw.get("sampling_random", 0), kw.get("avoid", 0),
                                        K, T, lanes, dt, substeps, iters, weighted, scene, form_request, minima, out)
    assert rc == 0
    return dict(zip(("instance", "ref", "form", "weighted", "scene", "blocks", "rows", "lanes"), out))


@pytest.mark.parametrize("task,mm", [(0, False), (1, False), (2, False), (3, True)])
@pytest.mark.parametrize("form_request", [0, 1, -1])
def test_default_scene_keeps_todays_plan(task, mm, form_request):
    """a handle at the default arena: the per-task instance with the reference's solver settings compiled in, the two-wavefront
    form for navigation and push where it is asked for, rows of minima only from the push_pull instance -- as before"""
    for minima in (0, 1):
        p = _plan(task, mm, form_request=form_request, minima=minima)
        two = task in (0, 1) and form_request != 0       # (32 workgroups: rollout_companion_pays)
        assert p == dict(instance=task, ref=1, form=int(two), weighted=0, scene=0, blocks=32, rows=32 * minima * (task == 3), lanes=64)
    p = _plan(task, mm, form_request=form_request, dt=0.04, substeps=3, iters=4)           # other solver settings: no _ref build
    assert (p["instance"], p["ref"], p["scene"]) == (task, 0, 0)
    p = _plan(task, mm, form_request=form_request, weighted=1)                             # tuned weights: as before
    assert p == dict(instance=-1, ref=1, form=0, weighted=1, scene=0, blocks=32, rows=0, lanes=64)
    p = _plan(task, mm, form_request=form_request, avoid=1)
    assert (p["instance"], p["weighted"], p["scene"]) == (-1, 0, 0)


@pytest.mark.parametrize("task,mm", [(0, False), (1, False), (2, False), (3, True)])
@pytest.mark.parametrize("weighted", [0, 1])
def test_custom_scene_or_forced_switch_takes_the_scene_build(task, mm, weighted):
    """what a custom arena or m3_set_point_scene_instance(1) amounts to (`scene`): instance -1, form 0, ref 0, the scene flag --
    whatever the task, the weights, the form request, the sampler and the solver settings"""
    for form_request in (0, 1, -1):
        for kw in ({}, dict(sampling_random=1), dict(mode_simple=1, sampling_random=1), dict(avoid=1), dict(dt=0.04, substeps=3, iters=4)):
            for minima in (0, 1):
                p = _plan(task, mm, scene=1, weighted=weighted, form_request=form_request, minima=minima, **kw)
                assert p == dict(instance=-1, ref=0, form=0, weighted=1, scene=1, blocks=32, rows=32 * minima, lanes=64), (kw, p)
    # partly filled last wavefront, narrow wavefronts: the workgroup count of every launcher
    assert _plan(task, mm, scene=1, K=100)["blocks"] == 2 and _plan(task, mm, scene=1, K=1025, lanes=1)["blocks"] == 1025
