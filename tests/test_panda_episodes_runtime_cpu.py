"""Lockstep panda episodes with run-time workspaces, weights and rows (m3_panda_episodes_create_ex with
M3_PANDA_EPISODES_RUNTIME), the parts that need no GPU: the declarations; the decision of what such a
set refuses (csrc/panda_variant.hpp, walked by tests/native/panda_episodes_mode_host.cpp); the two workspace tables and the two
lane bodies on them (csrc/panda_episode_tables.hpp through tests/native/panda_episode_tables_host.cpp, a stand-alone program,
plain and under the address and undefined-behaviour sanitizers, against the oracle's step_batch); the Python layer on recording
stand-in engines."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from m3p2i_aip_amd import _lib as L
from tests import panda_rollout_scenes_ref as R
from tests import panda_scene_fixture as X
from tests.test_device_dynamics_on_host import fma_flag, random_panda_worlds

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NATIVE = os.path.join(HERE, "native")
F = np.float32
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def P():
    import oracle.panda as P
    P.lib()
    return P


# ------------------------------------------------------------------ 1. symbols
def test_the_two_entry_points_and_the_flag_are_declared_and_bound():
    main = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    assert "#define M3_ABI_VERSION 4" in main                       # additive: the version stays
    # the additive entry points live in the companion header and table: the list of m3p2i_hip.h and _lib.SYMBOLS, which
    # tests/test_host_cpu.py and tests/test_panda_episodes_cpu.py hold name for name, stay as they are
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip_ext.h")).read()
    assert '#include "m3p2i_hip.h"' in hdr and "m3p2i_hip_ext.h" in main
    assert set(re.findall(r"\b(m3_[a-z_0-9]+)\s*\(", hdr)) >= {n for n, _, _ in L.SYMBOLS_EXT}
    assert not {n for n, _, _ in L.SYMBOLS_EXT} & {n for n, _, _ in L.SYMBOLS}
    assert re.search(r"^#define M3_PANDA_EPISODES_RUNTIME 1$", hdr, re.M) and L.PANDA_EPISODES_RUNTIME == 1
    assert re.search(r"^int m3_panda_episodes_create_ex\(m3_handle\* world, m3_handle\* const\* planners, int n, int max_ticks, "
                     r"int settle_ticks, int trace,\n\s+int flags, m3_panda_episodes\*\* out\);", hdr, re.M)
    assert re.search(r"^int m3_panda_episodes_flags\(const m3_panda_episodes\* eps\);", hdr, re.M)
    bound = {s[0]: (s[1], list(s[2])) for s in L.SYMBOLS_EXT}
    H = L._H
    assert bound["m3_panda_episodes_create_ex"] == (C.c_int, [H, C.POINTER(H), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(H)])
    assert bound["m3_panda_episodes_flags"] == (C.c_int, [H])
    lib = L.load()
    assert lib.m3_panda_episodes_flags(None) == -1                  # M3_ERR_BAD_ARG
    out = C.c_void_p(7)
    # unknown bits are refused before anything else is looked at (no handle can be created without a device)
    assert lib.m3_panda_episodes_create_ex(None, None, 1, 1, 0, 0, 2, C.byref(out)) == -1 and not out.value
    assert b"unknown flag bits" in lib.m3_panda_episodes_last_error(None)
    assert lib.m3_panda_episodes_create_ex(None, None, 1, 1, 0, 0, 0, C.byref(out)) == -1
    assert lib.m3_panda_episodes_last_error(None) == b"m3_panda_episodes_create: null argument"      # flags == 0: that call's words


def test_the_new_translation_unit_is_built_under_the_panda_rollouts_flags_and_holds_the_two_kernels():
    from m3p2i_aip_amd import build
    assert "rollout_panda_episodes_rt.hip" in build.SOURCES
    assert build.PER_SOURCE["rollout_panda_episodes_rt.hip"] == build.PER_SOURCE["rollout_panda.hip"] == ["-fno-slp-vectorize", "-O2"]
    blob = open(build.OUT, "rb").read()
    for name in (b"k_panda_episodes_pre_v", b"k_panda_episodes_post_v", b"k_panda_episodes_pre", b"k_panda_episodes_post"):
        assert name in blob, name


# ------------------------------------------------------------------ 2. the decision (stand-alone program)
def _build_mode(tmp, extra=("-O2",)):
    out = str(tmp / "panda_episodes_mode_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + list(extra) +
                          [os.path.join(NATIVE, "panda_episodes_mode_host.cpp"), "-o", out])
    return out


def _run_mode(prog, env=None):
    r = subprocess.run([prog], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    m = re.fullmatch(r"(\d+) checks, 0 failures\n", r.stdout)
    # 288 inputs x 2 orders x 6 facts
    assert m and int(m.group(1)) >= 288 * 12, r.stdout
    return r.stderr


def test_flag_off_is_panda_unbatched_and_flag_on_leaves_the_forced_off_refusals(tmp_path):
    _run_mode(_build_mode(tmp_path))


def test_the_decision_program_is_clean_under_asan_and_ubsan(tmp_path):
    prog = _build_mode(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    err = _run_mode(prog, env=env)
    assert "AddressSanitizer" not in err and "runtime error" not in err, err[-2000:]


def test_m3_api_asks_the_header_and_adds_no_chain_of_its_own():
    src = open(os.path.join(ROOT, "m3p2i_aip_amd", "csrc", "m3_api.hip")).read()
    body = src[src.index("static int peps_create("):src.index('extern "C" int m3_panda_episodes_ticks_done')]
    assert "panda_episodes_refusal(" in body and "panda_unbatched(" not in body
    # what the episodes refuse is not decided on the handle's fields here
    for field in ("panda_scene_instance", "panda_weighted_instance", "geometry_default", "weights_default"):
        assert field not in body, field


# ------------------------------------------------------------------ 3. the tables and the two lanes (stand-alone program)
@pytest.fixture(scope="module", params=[[], SAN], ids=["plain", "asan_ubsan"])
def host_program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("panda_episode_tables") / "panda_episode_tables_host")
    opt = ["-O1", "-g"] if request.param else ["-O2"]
    subprocess.check_call(["g++"] + opt + ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas"] + fma_flag() +
                          request.param + ["-I" + os.path.join(NATIVE, "shim"), os.path.join(NATIVE, "panda_episode_tables_host.cpp"), "-o", exe])
    return exe


CYCLE = (None, "table_z", "mu", "base", "COMBINED")     # (every field of the table differs somewhere)


def run_host(exe, tmp_path, scenes, plan_of, world_of, worlds, kept, u, dt=0.01, substeps=2):
    """the program on n episodes (run as an executable: nothing sanitized is loaded into python); returns (plan_rt [n, 74],
    world_rt [n, 74], pre [n, 84], post [steps, n, 84])"""
    n, steps = len(plan_of), len(u)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4if", n, steps, len(scenes), substeps, dt))
        f.write(np.stack([X.flat21(s) for s in scenes]).astype(F).tobytes())
        f.write(np.asarray(plan_of, np.int32).tobytes())
        f.write(np.asarray(world_of, np.int32).tobytes())
        f.write(np.ascontiguousarray(worlds, F).tobytes())
        f.write(np.ascontiguousarray(kept, F).tobytes())
        f.write(np.ascontiguousarray(u, F).tobytes())
    env = dict(os.environ)
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "panda_episode_tables_host: ok" in r.stdout, r.stdout + r.stderr
    out = np.fromfile(fout, F)
    assert out.size == 2 * n * 74 + (1 + steps) * n * 84
    rt = out[:2 * n * 74].reshape(2, n, 74)
    rest = out[2 * n * 74:].reshape(1 + steps, n, 84)
    return rt[0], rt[1], rest[0], rest[1:]


@pytest.mark.parametrize("n", [1, 61, 64, 65])
def test_every_row_of_both_tables_reads_back_as_make_panda_scene_rt_of_its_workspace(P, host_program, tmp_path, n):
    """the program compares each row read back through panda_scene_row_scene with make_panda_scene_rt of the row byte for byte,
    and that a refresh packs exactly the rows that changed (exit status); here also: the workspace words are the row's own"""
    scenes = [R.fields_of(s) for s in CYCLE]
    plan_of = [i % 5 for i in range(n)]
    world_of = [(i + 2) % 5 for i in range(n)]          # another 5-cycle: the two sides differ in every row
    w = P.init_world(n)
    plan_rt, world_rt, _, _ = run_host(host_program, tmp_path, scenes, plan_of, world_of, w, np.zeros((n, 9), F), np.zeros((0, n, 9), F))
    for rt, of in ((plan_rt, plan_of), (world_rt, world_of)):
        for i in range(n):
            f = X.full(scenes[of[i]])
            want = np.array(list(f["base"]) + list(f["table"]) + list(f["shelf"]) + list(f["obs_half"]) + [f["mu"]], F)
            np.testing.assert_array_equal(rt[i, 55:74].view(np.uint32), want.view(np.uint32))      # PandaSceneRT's own members
            inv = np.array([F(1) / F(f["cube_m"]), F(1) / F(f["obs_m"])], F)
            np.testing.assert_array_equal(rt[i, [50, 52]].view(np.uint32), inv.view(np.uint32))     # invm_cube, invm_obs
            np.testing.assert_array_equal(rt[i, :50].view(np.uint32), rt[0, :50].view(np.uint32))    # the uniform part
        assert len({rt[i, 50:].tobytes() for i in range(n)}) == min(n, 5)
    assert all(plan_rt[i, 50:].tobytes() != world_rt[i, 50:].tobytes() for i in range(n))


def test_the_pre_lane_steps_in_the_planning_row_and_the_post_lane_in_the_world_row(P, host_program, tmp_path):
    """65 episodes whose planning and world rows differ: the pre lane's step equals the oracle's in the PLANNING workspace, the
    post lane's in the WORLD workspace -- and neither equals the oracle in the other side's workspace"""
    n, steps = X.STEP_ENVS, 3
    scenes = [R.fields_of(s) for s in CYCLE]
    plan_of = np.array([i % 5 for i in range(n)])
    world_of = np.array([(i + 2) % 5 for i in range(n)])
    assert (plan_of != world_of).all()
    rng = np.random.default_rng(71)
    w = random_panda_worlds(P, P.default_scene(), n, rng)
    grip = rng.integers(0, 3, n)

    def controls(shape):
        u = rng.uniform(-2, 2, shape + (n, 9)).astype(F)
        u[..., 7:] = rng.uniform(-1.5, 1.5, shape + (n, 2))
        u[..., grip == 1, 7:] = 1.5
        u[..., grip == 2, 7:] = -1.5
        return u

    kept, u = controls(()), controls((steps,))
    _, _, pre, post = run_host(host_program, tmp_path, scenes, plan_of, world_of, w, kept, u)
    cols = [c for c in range(P.WORLD_FLOATS) if not (P.W_OBS + 3 <= c < P.W_OBS + 7) and not (P.W_OBS + 10 <= c < P.W_OBS + 13)]
    osc = [X.oracle_scene(P, s) for s in scenes]

    def oracle_pre(of):
        ref = w.copy()
        for i in range(n):
            row = np.ascontiguousarray(ref[i])
            P.infer_state(osc[of[i]], row)
            ref[i] = row
        for g in range(5):
            idx = np.flatnonzero(of == g)
            sub = np.ascontiguousarray(ref[idx])
            P.step_batch(osc[g], sub, np.ascontiguousarray(kept[idx]))
            ref[idx] = sub
        return ref

    def oracle_post(of):
        ref, out = w.copy(), []
        for t in range(steps):
            for g in range(5):
                idx = np.flatnonzero(of == g)
                sub = np.ascontiguousarray(ref[idx])
                P.step_batch(osc[g], sub, np.ascontiguousarray(u[t, idx]))
                ref[idx] = sub
            out.append(ref.copy())
        return np.stack(out)

    bits = lambda a: np.ascontiguousarray(a[..., cols]).view(np.uint32)      # noqa: E731
    neq = bits(pre) != bits(oracle_pre(plan_of))
    assert not neq.any(), f"pre lane: first (episode, column) {np.argwhere(neq)[0]} of {int(neq.sum())}"
    neq = bits(post) != bits(oracle_post(world_of))
    assert not neq.any(), f"post lane: first (tick, episode, column) {np.argwhere(neq)[0]} of {int(neq.sum())}"
    assert np.isfinite(post[..., cols]).all() and np.isfinite(pre[:, cols]).all()
    # the rows are live: in the other side's workspace most episodes end elsewhere
    assert (bits(pre) != bits(oracle_pre(world_of))).any(axis=1).mean() >= 0.5
    assert (bits(post[-1]) != bits(oracle_post(plan_of)[-1])).any(axis=1).mean() >= 0.5


# ------------------------------------------------------------------ 4. the Python layer on recording stand-ins
LOG = []      # what the stand-ins saw, in order


class _Engine:
    def __init__(self, name):
        self.name = name

    def _rec(self, what, *a):
        LOG.append((self.name, what) + a)

    def use_torch_stream(self): self._rec("stream")
    def set_action_out(self, out): self._rec("action_out")
    def set_point_scene(self, arena=None, **kw): self._rec("point", arena)
    def set_panda_scene(self, ws=None, **kw): self._rec("scene", ws)
    def set_panda_rollout_scenes(self, rows=None): self._rec("rows", None if rows is None else list(rows))
    def set_panda_cost_weights(self, w): self._rec("weights", dict(w))
    def bind_sim_panda(self, *a): self._rec("bind")
    def close(self): pass


class _Wrapper:
    """what PandaEpisodeSet and a planner's _bind_world touch of an IsaacGymWrapper; panda_scene / panda_scenes as the real one
    forms them"""
    made = []

    def __init__(self, cfg, env_type, num_envs=1, viewer=False, device="cpu", cube_on_shelf=False, panda_scenes=None, **kw):
        import torch
        from m3p2i_aip_amd import isaacgym_wrapper as W
        assert not kw, kw
        self.num_envs, self.env_type, self.given_panda_scenes = int(num_envs), env_type, panda_scenes
        self.panda_scene = W.panda_workspace(None, cfg.panda_scene)[0] if getattr(cfg, "panda_scene", None) else None
        self.panda_scenes = None if panda_scenes is None else [L.panda_scene_dict(L.panda_scene_fields(g)) for g in panda_scenes]
        self.point_scene = self.point_scenes = None
        self._dof_state = torch.zeros(self.num_envs, 18)
        self._root_state = torch.zeros(self.num_envs, 7, 13)
        self._engine = _Engine(f"sim{len(_Wrapper.made)}")
        _Wrapper.made.append(self)
        LOG.append((self._engine.name, "wrapper", self.num_envs))

    def _get_actor_index_by_name(self, name): return 4
    def set_actor_root_state_tensor(self, t): pass
    def stop_sim(self): pass


class _Episodes:
    def __init__(self, world, engines, max_ticks, settle_ticks=0, trace=False, panda_runtime=False):
        LOG.append(("episodes", "create", world.name, [e.name for e in engines], panda_runtime))

    def close(self): pass


class _Batch:
    def __init__(self, max_handles, device=0, panda_runtime=False):
        LOG.append(("batch", "create", max_handles, panda_runtime))

    def close(self): pass


@pytest.fixture()
def standins(monkeypatch):
    torch = pytest.importorskip("torch")
    from m3p2i_aip_amd import episodes, isaacgym_wrapper, planner
    count = [0]

    class _M3P2I(planner.MPPI):      # the real _bind_world on a recording engine; nothing is launched
        def __init__(self, cfg, dynamics=None, running_cost=None):
            owner = dynamics.__self__
            self.env_type, self.K, self.K_local, self.k_offset = cfg.env_type, cfg.mppi.num_samples, cfg.mppi.num_samples, 0
            self.T, self.nu, self.device = cfg.mppi.horizon, 9, torch.device("cpu")
            self._engine, self._sim, self._objective = _Engine(f"planner{count[0]}"), owner.sim, owner.objective
            self._fused, self.world_size, self.collective = True, 1, None
            count[0] += 1

        def _ensure_noise(self): self._engine._rec("noise")

    del LOG[:]
    _Wrapper.made = []
    monkeypatch.setattr(isaacgym_wrapper, "IsaacGymWrapper", _Wrapper)
    monkeypatch.setattr(planner, "M3P2I", _M3P2I)
    monkeypatch.setattr(episodes, "HipPandaEpisodes", _Episodes)
    monkeypatch.setattr(episodes, "HipBatch", _Batch)
    yield episodes
    from m3p2i_aip_amd import compat
    monkeypatch.undo()
    compat.install(force_standins=True)       # (the stand-in modules name the real classes again)


CPU = ["mppi.num_samples=8", "mppi.horizon=4", "mppi.device=cpu"]
WS = "panda_scene={table: [0, 0, 0.99, 0.6, 0.6, 0.025], mu: 0.5}"
MIXED = [[WS], ["world_panda_scene={cube_m: 0.2}"], ["panda_cost_weights={pick_ori: 25.0}"],
         ["world_panda_scene={cube_m: 0.2}", "rollout_workspace_spread={spread: 0.3, seed: 1}"]]


def test_a_run_time_set_builds_the_world_rows_pushes_every_planner_and_flags_the_batch(standins):
    from m3p2i_aip_amd import compat
    eps = [("config_panda", CPU + ov, dict(cube=(0.01, -0.01))) for ov in MIXED]
    es = standins.build_panda_set(eps, max_ticks=5, panda_runtime=True)
    try:
        assert es.panda_runtime
        # the planners' simulators in episode order, then the world: one row per episode, in episode order
        sims, world = _Wrapper.made[:4], _Wrapper.made[4]
        assert [s.num_envs for s in sims] == [8] * 4 and world.num_envs == 4
        f32 = lambda v: float(F(v))      # noqa: E731
        assert world.given_panda_scenes == [dict(table=[0, 0, 0.99, 0.6, 0.6, 0.025], mu=0.5), dict(cube_m=0.2), None, dict(cube_m=0.2)]
        assert world.panda_scene is None          # (the set's world is built from the rows, not from episode 0's config)
        # each simulator as closed_loop.Tamp builds it: the spread's rows on episode 3's alone
        cfg3 = compat.make_config("config_panda", CPU + MIXED[3])
        assert [s.given_panda_scenes for s in sims[:3]] == [None] * 3 and sims[3].given_panda_scenes == compat.rollout_panda_scenes(cfg3)
        assert len(sims[3].given_panda_scenes) == 8
        # what reached each planner's handle, and that all of it came before the set (whose first observe reads the handles)
        made = LOG.index(("episodes", "create", "sim4", ["planner0", "planner1", "planner2", "planner3"], True))
        before = LOG[:made]
        pushed = lambda name: [x[1:] for x in before if x[0] == name and x[1] in ("scene", "rows", "weights")]      # noqa: E731
        assert [(k, v["table"][2], v["mu"]) for k, v in pushed("planner0")] == [("scene", f32(0.99), f32(0.5))]
        assert pushed("planner1") == []           # (`world_panda_scene` is the world's alone)
        assert [(k, v["pick_ori"]) for k, v in pushed("planner2")] == [("weights", 25.0)]
        assert [(k, len(v)) for k, v in pushed("planner3")] == [("rows", 8)] and pushed("planner3")[0][1] == sims[3].panda_scenes
        assert not [x for x in LOG[made:] if x[1] in ("scene", "rows", "weights")]
        assert LOG[made + 1] == ("batch", "create", 4, True)
    finally:
        es.close()


def test_without_the_keyword_nothing_changes(standins):
    base = ("config_panda", CPU, None)
    es = standins.build_panda_set([base, base], max_ticks=5)
    try:
        assert not es.panda_runtime
        assert all(w.given_panda_scenes is None for w in _Wrapper.made) and _Wrapper.made[-1].num_envs == 2
        assert ("episodes", "create", "sim2", ["planner0", "planner1"], False) in LOG and ("batch", "create", 2, False) in LOG
        assert not [x for x in LOG if x[1] in ("scene", "rows", "weights", "bind")]      # (no push ahead of the first command)
    finally:
        es.close()
    messages = {
        0: r"build_panda_set: episode 1: `panda_scene` asks for a workspace of its own \(m3_set_panda_scene\), which the lockstep "
           r"panda episodes do not run \(one world handle, one scene\); use closed_loop.run",
        1: r"build_panda_set: episode 1: `world_panda_scene` asks for a workspace of its own \(m3_set_panda_scene\), which the "
           r"lockstep panda episodes do not run \(one world handle, one scene\); use closed_loop.run",
        2: r"build_panda_set: episode 1: `panda_cost_weights` asks for cost weights of its own \(m3_set_panda_cost_weights\), which "
           r"the lockstep panda episodes do not run \(their planners' batched command forms the literal cost\); use closed_loop.run",
        3: r"build_panda_set: episode 1: `rollout_workspace_spread` asks for a workspace per sample \(m3_set_panda_rollout_scenes\), "
           r"which the lockstep panda episodes do not run \(their planners' batched command carries one scene\); use closed_loop.run",
    }
    for k, ov in enumerate(MIXED):
        if k == 3:
            ov = ov[1:]
        for kw in ({}, dict(panda_runtime=False)):
            with pytest.raises(ValueError, match=messages[k]):
                standins.build_panda_set([base, ("config_panda", CPU + ov, None)], max_ticks=5, **kw)
            with pytest.raises(ValueError, match=messages[k].replace("build_panda_set", "run_panda_episodes")):
                standins.run_panda_episodes([base, ("config_panda", CPU + ov, None)], max_ticks=5, **kw)


def test_the_episodes_still_group_by_the_world_alone(standins):
    eps = [("config_panda", CPU + ov, None) for ov in MIXED]
    assert len(standins._panda_groups(eps, "t", True)) == 1
    eps.append(("config_panda", CPU + ["isaacgym.dt=0.02"], None))
    assert len(standins._panda_groups(eps, "t", True)) == 2
    with pytest.raises(ValueError, match="build_panda_set: the episodes' worlds differ"):
        standins.build_panda_set(eps, max_ticks=5, panda_runtime=True)


def test_the_tools_take_the_switch():
    import importlib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    bs = importlib.import_module("band_stats")
    import inspect
    assert "runtime" in inspect.signature(bs.panda_episodes_batched).parameters
    src = open(os.path.join(ROOT, "tools", "band_stats.py")).read()
    assert "--runtime" in src
    assert "_rt" in open(os.path.join(ROOT, "tools", "panda_episode_bench.py")).read()
