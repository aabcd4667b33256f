"""The run-time panda_env workspace (m3_set_panda_scene) without a GPU.

1. A host build of the product's panda_dyn.hpp through PandaSceneRT and make_panda_scene_rt (tests/native/panda_scene_host.cpp):
   the device source with the workspace as run-time values equals the oracle in the same workspace BIT FOR BIT -- in step mode
   (65 worlds x 25 steps, all 77 world floats the device carries) in every probe scene of tests/panda_scene_fixture.py and in
   COMBINED, and in the rollout's stepping (pick: forces + lazy kinematics; reach: no forces) at n = 64; at the default values
   the run-time scene type gives the bits of the compile-time one.  Bound: none (the spec is a fixed sequence of binary32
   operations; tests/test_device_dynamics_on_host.py holds the default workspace to the same standard).
2. A stand-alone program (tests/native/panda_scene_check.cpp, its own main) for make_panda_scene with masses,
   make_panda_scene_rt and the validation helper, built plain and with -fsanitize=address,undefined and run directly.
3. Plumbing: header <-> ctypes layout, the defaults against the oracle's, scenes.panda_scene_from_actors, the config keys, the
   wrapper's workspace from actors plus overrides, the planner's follow logic on a recording stand-in engine, the Python-side
   refusals of the batched paths.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from m3p2i_aip_amd import _lib as L
from tests import panda_scene_fixture as X
from tests.native_flags import host_flags
from tests.test_device_dynamics_on_host import HOST_FLAGS, fma_flag, random_panda_worlds

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
NATIVE = os.path.join(HERE, "native")


@pytest.fixture(scope="module")
def P():
    import oracle.panda as P
    P.lib()
    return P


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("panda_scene") / "libpanda_scene_host.so")
    subprocess.check_call(["g++"] + host_flags(HOST_FLAGS) + fma_flag() + ["-Wno-unknown-pragmas", "-I" + os.path.join(NATIVE, "shim"),
                           os.path.join(NATIVE, "panda_scene_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    VP = C.c_void_p
    lib.pss_step.argtypes = [VP, C.c_float, C.c_int, VP, C.c_int, VP, VP, C.c_int, VP, VP]
    lib.pss_infer_held.argtypes = [VP, C.c_float, C.c_int, VP, C.c_int, VP]
    lib.pss_fk.argtypes = [VP, VP, VP]
    lib.pss_default_scene.argtypes = [VP]
    return lib


def device_cols(P, mode):
    """the world floats the device carries: not the plate's orientation and angular velocity (77 of the oracle's 84); the reach
    rollout forms no contact forces"""
    return [c for c in range(P.WORLD_FLOATS) if not (P.W_OBS + 3 <= c < P.W_OBS + 7) and not (P.W_OBS + 10 <= c < P.W_OBS + 13)
            and not (mode == 2 and P.W_FT <= c < P.W_FT + 9)]


def run_both(P, lib, fields, n, steps, mode, seed, rt=True):
    """n random worlds loaded (grasp and sleep state inferred) and stepped `steps` times on the oracle in the workspace
    `fields` and on the host build; asserts equal bits after the load and after every step; returns the final worlds of both
    (the oracle's, the host build's)"""
    sc = X.oracle_scene(P, fields)
    arr = X.flat21(fields)
    ptr = arr.ctypes.data if rt else None
    rng = np.random.default_rng(seed)
    a = random_panda_worlds(P, P.default_scene(), n, rng)
    b = a.copy()
    hp, trav, obs = np.zeros((n, 3), F), np.zeros(n, F), np.zeros((n, 10), F)
    for i in range(n):
        row = np.ascontiguousarray(a[i])
        P.infer_state(sc, row)
        a[i] = row
    lib.pss_infer_held(ptr, 0.01, 2, b.ctypes.data, n, hp.ctypes.data)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    cols = device_cols(P, mode)
    assert len(cols) == (77 if mode != 2 else 68)
    grip = rng.integers(0, 3, n)
    for t in range(steps):
        u = rng.uniform(-2, 2, (n, 9)).astype(F)
        u[:, 7:] = rng.uniform(-1.5, 1.5, (n, 2))
        u[grip == 1, 7:] = 1.5
        u[grip == 2, 7:] = -1.5
        P.step_batch(sc, a, u)
        lib.pss_step(ptr, 0.01, 2, b.ctypes.data, n, u.ctypes.data, obs.ctypes.data, mode, hp.ctypes.data, trav.ctypes.data)
        neq = a[:, cols].view(np.uint32) != b[:, cols].view(np.uint32)
        if neq.any():
            r, c = np.argwhere(neq)[0]
            raise AssertionError(f"mode {mode} step {t} world {r} column {cols[c]}: oracle {a[r, cols[c]]!r} device-source "
                                 f"{b[r, cols[c]]!r} ({int(neq.sum())} values differ)")
        for i in range(0, n, 13):       # what the costs read: the finger links at the final joint values, in the scene's base
            Lk = P.fk(sc, a[i, :9])
            want = np.concatenate([Lk["pos"][9], Lk["quat"][9], Lk["pos"][10]]).astype(F)
            np.testing.assert_array_equal(want.view(np.uint32), obs[i].view(np.uint32))
    assert np.isfinite(a[:, cols]).all()
    return a, b


# ------------------------------------------------------------------ 1. the device source through PandaSceneRT
@pytest.mark.parametrize("name", list(X.SCENES))
def test_step_mode_in_every_probe_scene_equals_the_oracle(P, host_lib, name):
    got, _ = run_both(P, host_lib, X.SCENES[name], X.STEP_ENVS, X.STEP_STEPS, 0, seed=70)
    # the scene is live here too: the same worlds under the same controls end elsewhere in the default workspace
    ref, _ = run_both(P, host_lib, None, X.STEP_ENVS, X.STEP_STEPS, 0, seed=70)
    assert (got.view(np.uint32) != ref.view(np.uint32)).any(axis=1).sum() >= 1


@pytest.mark.parametrize("mode", [1, 2], ids=["pick_rollout_lazy_fk", "reach_rollout_lazy_fk_no_forces"])
@pytest.mark.parametrize("name", list(X.SCENES))
def test_rollout_stepping_in_every_probe_scene_equals_the_oracle(P, host_lib, name, mode):
    run_both(P, host_lib, X.SCENES[name], 64, 25, mode, seed=40 + mode)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_default_values_through_the_run_time_scene_equal_the_compile_time_build(P, host_lib, mode):
    n, steps = 64, 25
    _, rt = run_both(P, host_lib, None, n, steps, mode, seed=11, rt=True)       # the host build's worlds through PandaSceneRT
    _, ct = run_both(P, host_lib, None, n, steps, mode, seed=11, rt=False)      # ... and through PandaScene
    cols = device_cols(P, mode)
    np.testing.assert_array_equal(rt[:, cols].view(np.uint32), ct[:, cols].view(np.uint32))


def test_link_poses_follow_the_base(P, host_lib):
    fields = X.PROBES["base"][0]
    sc = X.oracle_scene(P, fields)
    arr = X.flat21(fields)
    rng = np.random.default_rng(5)
    for _ in range(8):
        q = (np.array(sc.qlo) + rng.uniform(0.05, 0.95, 9) * (np.array(sc.qhi) - np.array(sc.qlo))).astype(F)
        out = np.zeros(77, F)
        host_lib.pss_fk(arr.ctypes.data, q.ctypes.data, out.ctypes.data)
        Lk = P.fk(sc, q)
        want = np.concatenate([Lk["pos"], Lk["quat"]], axis=1).astype(F)
        np.testing.assert_array_equal(out.reshape(11, 7).view(np.uint32), want.view(np.uint32))
    assert np.allclose(out[:3], fields["base"])


# ------------------------------------------------------------------ 2. the stand-alone program, plain and sanitized
@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_host_side_program(tmp_path, san):
    exe = str(tmp_path / "panda_scene_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas"] + san +
                          ["-I" + os.path.join(NATIVE, "shim"), os.path.join(NATIVE, "panda_scene_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)     # (run directly: nothing sanitized is loaded into python)
    assert r.returncode == 0 and "panda_scene_check: ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------ 3. plumbing
def test_struct_layout_header_and_ctypes(P, host_lib):
    text = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    body = re.search(r"typedef struct m3_panda_scene \{(.*?)\} m3_panda_scene;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(m.group(1), int(m.group(2) or 1)) for m in re.finditer(r"float\s+(\w+)(?:\[(\d+)\])?\s*;", body)]
    assert fields == [("base", 3), ("table", 6), ("shelf", 6), ("obs_half", 3), ("obs_m", 1), ("cube_m", 1), ("mu", 1)]
    assert [(n, C.sizeof(t) // 4) for n, t in L.PandaSceneFields._fields_] == fields
    assert C.sizeof(L.PandaSceneFields) == 21 * 4
    assert list(L.PANDA_SCENE_DEFAULTS) == [n for n, _ in fields] and L.PANDA_SCENE_DEFAULTS == X.DEFAULTS
    # the defaults: the library's header constants, the ctypes table and the oracle's default scene, bit for bit
    d = np.zeros(21, F)
    host_lib.pss_default_scene(d.ctypes.data)
    np.testing.assert_array_equal(d.view(np.uint32), X.flat21(None).view(np.uint32))
    np.testing.assert_array_equal(np.frombuffer(bytes(L.panda_scene_fields(None)), F).view(np.uint32), d.view(np.uint32))
    sc = P.default_scene()
    orc = np.array(list(sc.base) + list(sc.table) + list(sc.shelf) + list(sc.obs_half) + [sc.obs_m, sc.cube_m, sc.mu], F)
    np.testing.assert_array_equal(orc.view(np.uint32), d.view(np.uint32))
    assert sc.cube_mu == 1.0 and sc.cube_half == F(0.025)
    # every symbol of the feature is declared in the header and bound
    bound = {n for n, _, _ in L.SYMBOLS}
    for sym in ("m3_default_panda_scene", "m3_set_panda_scene", "m3_get_panda_scene", "m3_set_panda_scene_instance",
                "m3_panda_scene_instance_used"):
        assert sym in bound and re.search(r"\b%s\(" % sym, text)
    assert "#define M3_ABI_VERSION 4" in text
    with pytest.raises(ValueError, match=r"unknown panda scene field\(s\) \['tabel'\]: one of \['base', 'table'"):
        L.panda_scene_fields(dict(tabel=(0,) * 6))
    with pytest.raises(ValueError, match="'table': 3 values, it has 6"):
        L.panda_scene_fields(dict(table=(0, 0, 1)))


def test_panda_scene_from_actors():
    from m3p2i_aip_amd import scenes

    def actors(**changes):
        out = [scenes.Actor(**vars(a)) for a in scenes.PANDA_ENV]
        for a in out:
            for k, v in changes.get(a.name.replace("-", "_"), {}).items():
                setattr(a, k, v)
        return out

    d = scenes.panda_scene_from_actors(scenes.PANDA_ENV)
    assert d == L.PANDA_SCENE_DEFAULTS and list(d) == list(L.PANDA_SCENE_DEFAULTS) and scenes.panda_scene_is_default(d)
    assert bytes(L.panda_scene_fields(d)) == bytes(L.panda_scene_fields(None))          # bit for bit
    low = scenes.panda_scene_from_actors(actors(table=dict(init_pos=[0.0, 0.0, 0.99]), shelf_stand=dict(size=[0.2, 0.2, 0.24]),
                                                panda=dict(init_pos=[-0.40, 0.0, 1.10]), dyn_obs=dict(size=[0.32, 0.2, 0.04])))
    assert low["table"] == (0.0, 0.0, float(F(0.99)), 0.6, 0.6, 0.025) and low["shelf"][3:] == (0.1, 0.1, float(F(0.12)))
    assert low["base"] == (float(F(-0.40)), 0.0, float(F(1.10))) and low["obs_half"] == (float(F(0.16)), 0.1, float(F(0.02)))
    assert low["obs_m"] == pytest.approx(1000 * 0.32 * 0.2 * 0.04, rel=1e-6) and low["cube_m"] == 0.125 and low["mu"] == 1.0
    assert not scenes.panda_scene_is_default(low)
    slip = scenes.panda_scene_from_actors(actors(**{n: dict(friction=0.3) for n in ("table", "shelf_stand", "dyn_obs", "cubeA", "cubeB", "panda")}))
    assert slip["mu"] == float(F(0.3))
    with pytest.raises(ValueError, match="cubeA has size .* bounding radius"):
        scenes.panda_scene_from_actors(actors(cubeA=dict(size=[0.06, 0.06, 0.06]), cubeB=dict(size=[0.06, 0.06, 0.06])))
    with pytest.raises(ValueError, match="cubeB has size"):
        scenes.panda_scene_from_actors(actors(cubeB=dict(size=[0.05, 0.05, 0.04])))       # (disagreeing cubes: one cube_m)
    with pytest.raises(ValueError, match="frictions differ"):
        scenes.panda_scene_from_actors(actors(table=dict(friction=0.5)))
    with pytest.raises(ValueError, match="no actor 'shelf_stand'"):
        scenes.panda_scene_from_actors([a for a in scenes.PANDA_ENV if a.name != "shelf_stand"])


def test_cube_masses_that_disagree_raise():
    """the dynamics know one cube_m.  Two cubes of the fixed size have the same volume, so the rule is reached only through the
    tolerances: a 5e-13 change of one edge passes the size check (1e-12) while the volumes differ by more than the 1e-15 the mass
    check allows"""
    from m3p2i_aip_amd import scenes
    acts = [scenes.Actor(**vars(a)) for a in scenes.PANDA_ENV]
    next(a for a in acts if a.name == "cubeB").size = [0.05, 0.05, 0.05 + 5e-13]      # (inside the size tolerance, another volume)
    with pytest.raises(ValueError, match="cubeA and cubeB differ in mass"):
        scenes.panda_scene_from_actors(acts)


def test_config_keys():
    from m3p2i_aip_amd import compat
    plain = compat.make_config("config_panda")
    assert plain.panda_scene is None and plain.world_panda_scene is None and plain.isaacgym.panda_scene is None
    assert compat.world_isaacgym_config(plain) is plain.isaacgym and compat.world_panda_scene(plain) == {}
    cfg = compat.make_config("config_panda", ["panda_scene={mu: 0.5, table: [0, 0, 0.99, 0.6, 0.6, 0.025]}",
                                              "world_panda_scene={mu: 0.3, cube_m: 0.4}"])
    assert cfg.isaacgym.panda_scene == dict(mu=0.5, table=[0, 0, 0.99, 0.6, 0.6, 0.025])      # the planner's side
    world = compat.world_isaacgym_config(cfg)
    assert world is not cfg.isaacgym and world.panda_scene == dict(mu=0.3, cube_m=0.4, table=[0, 0, 0.99, 0.6, 0.6, 0.025])
    assert cfg.isaacgym.panda_scene["mu"] == 0.5                                              # ... keeps panda_scene
    only_world = compat.make_config("config_panda", ["world_panda_scene={cube_m: 0.4}"])
    assert only_world.isaacgym.panda_scene is None and compat.world_isaacgym_config(only_world).panda_scene == dict(cube_m=0.4)
    for key in ("panda_scene", "world_panda_scene"):
        with pytest.raises(ValueError, match=f"^{key}: panda_env only"):
            compat.make_config("config_point", [key + "={mu: 0.5}"])
        with pytest.raises(ValueError, match=f"^{key}: unknown panda scene field"):
            compat.make_config("config_panda", [key + "={friction: 0.5}"])
    with pytest.raises(ValueError, match="point_scene: point_env only"):                      # (as before)
        compat.make_config("config_panda", ["point_scene={wall: 3.0}"])


def test_wrapper_workspace_from_actors_and_overrides():
    from m3p2i_aip_amd import scenes
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper, panda_workspace
    ws, env = panda_workspace(None, None)
    assert ws is None and [vars(a) for a in env] == [vars(a) for a in scenes.PANDA_ENV]
    assert panda_workspace([scenes.Actor(**vars(a)) for a in scenes.PANDA_ENV], None)[0] is None     # the reference's: None
    acts = [scenes.Actor(**vars(a)) for a in scenes.PANDA_ENV]
    by = {a.name: a for a in acts}
    by["table"].init_pos = [0.0, 0.0, 0.99]
    by["cubeA"].init_pos = [0.2, -0.2, 1.05]
    ws, env = panda_workspace(acts, dict(mu=0.3, shelf=(0.42, 0.0, 1.175, 0.1, 0.1, 0.12)))
    assert ws["table"][2] == float(F(0.99)) and ws["mu"] == float(F(0.3)) and ws["shelf"][0] == float(F(0.42))
    assert ws["base"] == tuple(float(F(x)) for x in L.PANDA_SCENE_DEFAULTS["base"]) and ws["cube_m"] == 0.125   # (binary32 values)
    e = {a.name: a for a in env}
    assert e["cubeA"].init_pos == [0.2, -0.2, 1.05]                       # the actors place the cubes, as always
    assert e["shelf_stand"].init_pos == list(ws["shelf"][:3]) and e["shelf_stand"].size == [2.0 * x for x in ws["shelf"][3:]]
    assert e["table_stand"].init_pos == by["table_stand"].init_pos        # not part of the dynamics
    masses_only, _ = panda_workspace(None, dict(cube_m=0.4))
    assert masses_only is not None and masses_only["cube_m"] == float(F(0.4))
    with pytest.raises(ValueError, match=r"panda_scene: unknown field\(s\) \['table_z'\]: one of \['base', 'table', 'shelf', 'obs_half', "
                                         r"'obs_m', 'cube_m', 'mu'\]"):
        IsaacGymWrapper(IsaacGymConfig(dt=0.01, panda_scene=dict(table_z=0.99)), "panda_env", num_envs=2)
    with pytest.raises(ValueError, match="names and the order of scenes.PANDA_ENV"):
        IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=2, actors=acts[::-1])
    with pytest.raises(ValueError, match="panda_scene: panda_env only"):
        IsaacGymWrapper(IsaacGymConfig(dt=0.05, panda_scene=dict(mu=0.3)), "point_env", num_envs=2)
    # point_scene / point_scenes on the panda_env keep raising exactly as they did
    with pytest.raises(ValueError, match="^actors / point_scene: point_env only$"):
        IsaacGymWrapper(IsaacGymConfig(dt=0.01, point_scene=dict(wall=3.0)), "panda_env", num_envs=2)
    with pytest.raises(ValueError, match="^point_scenes: point_env only$"):
        IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=2, point_scenes=[None, None])


class _Engine:
    def __init__(self, held=None):
        self.calls, self.held = [], held

    def set_panda_scene(self, scene=None, **kw):
        self.calls.append(("panda_scene", scene))
        self.held = scene

    def set_point_scene(self, arena=None, **kw):
        self.calls.append(("scene", arena))

    def panda_scene(self):
        return {**L.PANDA_SCENE_DEFAULTS, **(self.held or {})}


class _Sim:
    def __init__(self, panda_scene=None):
        self.num_envs, self.panda_scene, self.point_scene, self.point_scenes = 8, panda_scene, None, None


def _planner(sim=None, held=None):
    from m3p2i_aip_amd import planner
    p = object.__new__(planner.MPPI)
    p.env_type, p.K, p.K_local, p.k_offset = "panda_env", 8, 8, 0
    p._engine, p._sim = _Engine(held), sim
    p._bound_sim = sim
    p._fused, p.world_size, p.collective = True, 1, None
    return p


def test_planner_follows_the_workspace_of_its_wrapper():
    ws = {**L.PANDA_SCENE_DEFAULTS, "mu": 0.3}
    sim = _Sim(ws)
    p = _planner(sim)
    assert p.needs_panda_scene_instance
    p._bind_world(); p._bind_world()
    assert p._engine.calls == [("panda_scene", ws)]                     # once
    sim.panda_scene = dict(ws)                                           # equal fields: nothing to push
    p._bind_world()
    assert len(p._engine.calls) == 1
    sim.panda_scene = {**ws, "cube_m": 0.4}
    p._bind_world()
    assert p._engine.calls[-1] == ("panda_scene", {**ws, "cube_m": 0.4}) and len(p._engine.calls) == 2
    sim.panda_scene = None                                               # back to the reference's workspace
    p._bind_world(); p._bind_world()
    assert p._engine.calls[2:] == [("panda_scene", None)] and not p.needs_panda_scene_instance
    # follow off: the planner owns its engine's workspace
    q = _planner(_Sim(ws), held=dict(table=(0.0, 0.0, 0.99, 0.6, 0.6, 0.025)))
    q.follow_sim_scene = False
    q._bind_world()
    assert q._engine.calls == [] and q.needs_panda_scene_instance
    m = _planner(_Sim({**L.PANDA_SCENE_DEFAULTS, "cube_m": 0.4, "obs_m": 0.2}))
    assert not m.needs_panda_scene_instance                              # the masses alone stay on today's kernels
    # a point_env planner is not touched by any of this
    from m3p2i_aip_amd import planner
    pt = _planner(_Sim(ws))
    pt.env_type = "point_env"
    assert not pt.needs_panda_scene_instance


def test_the_planners_reading_of_its_workspace_is_kept_between_ticks():
    """command_batch asks every planner on every tick: the engine is asked again only after a set_panda_scene, a followed
    wrapper's fields are compared, not converted"""
    class Counting(_Engine):
        panda_scene_sets, asked = 0, 0

        def set_panda_scene(self, scene=None, **kw):
            super().set_panda_scene(scene, **kw)
            self.panda_scene_sets += 1

        def panda_scene(self):
            self.asked += 1
            return super().panda_scene()

    p = _planner(_Sim(None))
    p._engine = Counting(dict(mu=0.3))
    p.follow_sim_scene = False
    assert [p.needs_panda_scene_instance for _ in range(5)] == [True] * 5 and p._engine.asked == 1
    p._engine.set_panda_scene(dict(cube_m=0.4))
    assert [p.needs_panda_scene_instance for _ in range(5)] == [False] * 5 and p._engine.asked == 2
    p.follow_sim_scene = True                                            # following: the wrapper's fields, the engine is not asked
    p._sim.panda_scene = {**L.PANDA_SCENE_DEFAULTS, "mu": 0.3}
    assert p.needs_panda_scene_instance and p.needs_panda_scene_instance and p._engine.asked == 2
    p._sim.panda_scene["mu"] = 1.0                                       # changed in place: seen
    assert not p.needs_panda_scene_instance
    p._sim.panda_scene = None
    assert not p.needs_panda_scene_instance and p._engine.asked == 2


def test_batched_paths_refuse_a_workspace_that_needs_the_run_time_instance(monkeypatch):
    from m3p2i_aip_amd import planner
    from m3p2i_aip_amd.episodes import build_panda_set, run_panda_episodes
    monkeypatch.setattr(planner, "HipEngine", _Engine)
    good, bad = _planner(_Sim(None)), _planner(_Sim({**L.PANDA_SCENE_DEFAULTS, "mu": 0.3}))
    with pytest.raises(ValueError, match="planner 1 plans in a workspace of its own \\(m3_set_panda_scene"):
        planner.command_batch([good, bad], [np.zeros(18, F)] * 2)
    assert good._engine.calls == [] and bad._engine.calls == []          # before any call
    eps = [("config_panda", [], None), ("config_panda", ["panda_scene={mu: 0.3}"], None)]
    for run in (run_panda_episodes, build_panda_set):
        with pytest.raises(ValueError, match="episode 1: `panda_scene` .*m3_set_panda_scene"):
            run(eps, max_ticks=4)
    with pytest.raises(ValueError, match="episode 0: `world_panda_scene`"):
        run_panda_episodes([("config_panda", ["world_panda_scene={base: [-0.4, 0, 1.1]}"], None)], max_ticks=4)
    # the masses alone too: the set has one world handle built from its first episode, so an episode's own masses would be
    # dropped -- refused, not ignored
    for ov in ("world_panda_scene={cube_m: 0.4}", "panda_scene={obs_m: 0.2}"):
        for run in (run_panda_episodes, build_panda_set):
            with pytest.raises(ValueError, match="episode 1: `(world_)?panda_scene` .*m3_set_panda_scene"):
                run([("config_panda", [], None), ("config_panda", [ov], None)], max_ticks=4)


def test_probe_scenes_show_on_the_oracle(P):
    """the condition every GPU rollout case repeats, here for all of them at once: each probe changes the costs of >= 80 % of the
    samples in its world; COMBINED does in >= 30 of the 42 fuzz worlds (>= 50 % of the samples)"""
    for name, (_, world, task, grip, _) in X.PROBES.items():
        assert X.share(name, world, task, grip) >= 0.8, name
    assert X.share("shelf_hz", "shelf", "reach", 1) == 1.0
    assert len(X.qualifying_fuzz_worlds()) >= 30
    assert X.share("COMBINED", 41, "reach", 2, X.K_RAGGED) >= 0.8
