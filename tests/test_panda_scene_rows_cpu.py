"""One panda_env workspace per environment (m3_set_panda_scene_rows) and per sample of the fused rollout
(m3_set_panda_rollout_scenes), the parts that need no GPU: the six entry points, the device table and
the per-row step through the host build of the product's headers (tests/native/panda_scene_rows_host.cpp, a stand-alone
program, plain and under the address and undefined-behaviour sanitizers), the stitched oracle the GPU tests compare against,
the guard that the GPU cases' cycles of workspaces show, and the Python plumbing on a recording stand-in engine."""
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
D = L.PANDA_SCENE_DEFAULTS
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def P():
    import oracle.panda as P
    P.lib()
    return P


# ------------------------------------------------------------------ 1. symbols
def test_the_six_entry_points_exist_with_their_prototypes():
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    assert "#define M3_ABI_VERSION 4" in hdr
    bound = {s[0]: (s[1], list(s[2])) for s in L.SYMBOLS}
    PS = C.POINTER(L.PandaSceneFields)
    for setter, getter, flag in (("m3_set_panda_scene_rows", "m3_get_panda_scene_row", "m3_panda_scene_rows_set"),
                                 ("m3_set_panda_rollout_scenes", "m3_get_panda_rollout_scene", "m3_panda_rollout_scenes_set")):
        assert bound[setter] == (C.c_int, [L._H, PS, C.c_int])
        assert bound[getter] == (C.c_int, [L._H, C.c_int, PS])
        assert bound[flag] == (C.c_int, [L._H])
        assert re.search(r"^int %s\(m3_handle\* h, const m3_panda_scene\* scenes, int n\);" % setter, hdr, re.M)
        assert re.search(r"^int %s\(const m3_handle\* h, int row, m3_panda_scene\* out\);" % getter, hdr, re.M)
        assert re.search(r"^int %s\(const m3_handle\* h\);" % flag, hdr, re.M)
    lib = L.load()
    sc = L.PandaSceneFields()
    # (no handle can be created without a device -- the handle's answers are checked in tests/test_panda_scene_rows_gpu.py)
    for setter, getter, flag in ((lib.m3_set_panda_scene_rows, lib.m3_get_panda_scene_row, lib.m3_panda_scene_rows_set),
                                 (lib.m3_set_panda_rollout_scenes, lib.m3_get_panda_rollout_scene, lib.m3_panda_rollout_scenes_set)):
        assert setter(None, C.byref(sc), 1) == -1 and getter(None, 0, C.byref(sc)) == -1 and flag(None) == -1


# ------------------------------------------------------------------ 2. the table and the per-row step (stand-alone program)
@pytest.fixture(scope="module", params=[[], SAN], ids=["plain", "asan_ubsan"])
def host_program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("panda_scene_rows") / "panda_scene_rows_host")
    opt = ["-O1", "-g"] if request.param else ["-O2"]
    subprocess.check_call(["g++"] + opt + ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas"] + fma_flag() +
                          request.param + ["-I" + os.path.join(NATIVE, "shim"), os.path.join(NATIVE, "panda_scene_rows_host.cpp"),
                                           "-o", exe])
    return exe


STEP_CYCLE = (None, "table_z", "mu", "base", "COMBINED")     # (step mode: every field of the table differs somewhere)


def run_host(exe, tmp_path, scenes, scene_of, worlds, u, dt=0.01, substeps=2):
    """the program on n rows (run as an executable: nothing sanitized is loaded into python); returns (scenes_rt [n, 74],
    worlds [1 + steps, n, 84])"""
    n, steps = len(scene_of), len(u)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4if", n, steps, len(scenes), substeps, dt))
        f.write(np.stack([X.flat21(s) for s in scenes]).astype(F).tobytes())
        f.write(np.asarray(scene_of, np.int32).tobytes())
        f.write(np.ascontiguousarray(worlds, F).tobytes())
        f.write(np.ascontiguousarray(u, F).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and "panda_scene_rows_host: ok" in r.stdout, r.stdout + r.stderr
    out = np.fromfile(fout, F)
    assert out.size == n * 74 + (1 + steps) * n * 84
    return out[:n * 74].reshape(n, 74), out[n * 74:].reshape(1 + steps, n, 84)


@pytest.mark.parametrize("n", [1, 61, 64, 65])
def test_rows_read_back_from_the_table_are_make_panda_scene_rt_of_the_row(P, host_program, tmp_path, n):
    """the program itself compares each row's PandaSceneRT read back from the table with make_panda_scene_rt of the row byte for
    byte (exit status); here also: the workspace words are the row's, whatever the handle's own scene holds"""
    scenes = [R.fields_of(s) for s in STEP_CYCLE]
    scene_of = [i % 5 for i in range(n)]
    w = P.init_world(n)
    rt, _ = run_host(host_program, tmp_path, scenes, scene_of, w, np.zeros((0, n, 9), F))
    for i in range(n):
        f = X.full(scenes[scene_of[i]])
        want = np.array(list(f["base"]) + list(f["table"]) + list(f["shelf"]) + list(f["obs_half"]) + [f["mu"]], F)
        np.testing.assert_array_equal(rt[i, 55:74].view(np.uint32), want.view(np.uint32))     # PandaSceneRT's own members
        inv = np.array([F(1) / F(f["cube_m"]), F(1) / F(f["obs_m"])], F)
        np.testing.assert_array_equal(rt[i, [50, 52]].view(np.uint32), inv.view(np.uint32))    # invm_cube, invm_obs
        np.testing.assert_array_equal(rt[i, :50].view(np.uint32), rt[0, :50].view(np.uint32))   # the uniform part
    assert len({rt[i, 50:].tobytes() for i in range(n)}) == min(n, 5)


def test_step_of_65_environments_in_a_cycle_of_workspaces_equals_the_oracle_per_group(P, host_program, tmp_path):
    n, steps = X.STEP_ENVS, X.STEP_STEPS
    scenes = [R.fields_of(s) for s in STEP_CYCLE]
    scene_of = np.array([i % 5 for i in range(n)])
    rng = np.random.default_rng(70)
    w = random_panda_worlds(P, P.default_scene(), n, rng)
    grip = rng.integers(0, 3, n)
    u = rng.uniform(-2, 2, (steps, n, 9)).astype(F)
    u[:, :, 7:] = rng.uniform(-1.5, 1.5, (steps, n, 2))
    u[:, grip == 1, 7:] = 1.5
    u[:, grip == 2, 7:] = -1.5
    _, got = run_host(host_program, tmp_path, scenes, scene_of, w, u)
    # the oracle: step_batch per group of equal scenes
    cols = [c for c in range(P.WORLD_FLOATS) if not (P.W_OBS + 3 <= c < P.W_OBS + 7) and not (P.W_OBS + 10 <= c < P.W_OBS + 13)]
    ref = w.copy()
    osc = [X.oracle_scene(P, s) for s in scenes]
    for i in range(n):
        row = np.ascontiguousarray(ref[i])
        P.infer_state(osc[scene_of[i]], row)
        ref[i] = row
    np.testing.assert_array_equal(got[0][:, cols].view(np.uint32), ref[:, cols].view(np.uint32))
    for t in range(steps):
        for g in range(5):
            idx = np.flatnonzero(scene_of == g)
            sub = np.ascontiguousarray(ref[idx])
            P.step_batch(osc[g], sub, np.ascontiguousarray(u[t, idx]))
            ref[idx] = sub
        neq = got[1 + t][:, cols].view(np.uint32) != ref[:, cols].view(np.uint32)
        assert not neq.any(), f"step {t}: first (environment, column) {np.argwhere(neq)[0]} of {int(neq.sum())}"
    assert np.isfinite(ref[:, cols]).all()
    # the rows are live: the same worlds under the same controls end elsewhere in one workspace
    one = w.copy()
    for i in range(n):
        row = np.ascontiguousarray(one[i])
        P.infer_state(osc[0], row)
        one[i] = row
    for t in range(steps):
        P.step_batch(osc[0], one, u[t])
    differ = (one[:, cols].view(np.uint32) != ref[:, cols].view(np.uint32)).any(axis=1)
    assert not differ[scene_of == 0].any() and differ[scene_of != 0].mean() >= 0.5


# ------------------------------------------------------------------ 3. the reference of the GPU tests
@pytest.mark.parametrize("task,grip,world,mm", [("reach", 2, 41, False), ("reach", 2, 41, True), ("pick", 2, 40, False),
                                                ("place", 1, 22, False)])
def test_stitched_oracle_with_equal_rows_is_the_single_scene_oracle(P, task, grip, world, mm):
    K = X.K
    w0 = X.world_of(world)
    mk = lambda: P.make_cfg(K, X.T, multi_modal=mm, task=task, goal=np.array(X.GOAL, F), gripper_cmd=grip)  # noqa: E731
    a = R.stitched_planner(P, mk(), X.delta_of(K), task, [X.COMBINED] * K)
    b = P.OraclePandaPlanner(mk(), X.delta_of(K), X.oracle_scene(P, X.COMBINED))
    c = R.stitched_planner(P, mk(), X.delta_of(K), task, [X.COMBINED if i % 2 else dict(X.COMBINED) for i in range(K)])
    for call in range(2):
        ua, ub, uc = a.command(w0), b.command(w0), c.command(w0)
        assert ua.tobytes() == ub.tobytes() == uc.tobytes(), call
        for name in ("states", "actions", "cost_h", "J"):
            assert a.last[name].tobytes() == b.last[name].tobytes() == c.last[name].tobytes(), (call, name)
    assert np.isfinite(a.last["cost_h"]).all() and a.last["cost_h"].std() > 0


def test_stitched_oracle_reads_the_cube_of_sample_0_in_its_own_row(P):
    """quirk Q8 under per-sample workspaces: with row 0 alone in another workspace, every sample's reach cost moves"""
    K, (world, task, grip, _) = X.K, R.CYCLES["reach"]
    w0 = X.world_of(world)
    cfg = P.make_cfg(K, X.T, multi_modal=False, task=task, goal=np.array(X.GOAL, F), gripper_cmd=grip)
    base = R.stitched_planner(P, cfg, X.delta_of(K), task, [None] * K)
    moved = R.stitched_planner(P, cfg, X.delta_of(K), task, [X.SCENES["table_z"]] + [None] * (K - 1))
    base.command(w0); moved.command(w0)
    assert base.last["states"][1:].tobytes() == moved.last["states"][1:].tobytes()        # the other samples' simulations stand
    differ = (base.last["cost_h"].view(np.uint32) != moved.last["cost_h"].view(np.uint32)).any(axis=1)
    assert differ.mean() >= 0.8                                                            # ... their costs do not


# ------------------------------------------------------------------ 4. the guard of the GPU cases
@pytest.mark.parametrize("k", [X.K, X.K_RAGGED])
@pytest.mark.parametrize("cycle", list(R.CYCLES))
def test_every_pair_of_scenes_of_a_cycle_shows(P, cycle, k):
    shares = R.pair_shares(cycle, k)
    assert len(shares) == 10
    for pair, s in shares.items():
        assert s >= 0.8, (cycle, k, pair, s)


# ------------------------------------------------------------------ 5. Python plumbing on a recording engine
class _Engine:
    def __init__(self):
        self.calls = []

    def set_point_scene(self, arena=None, **kw):
        self.calls.append(("point", arena))

    def set_panda_scene(self, ws=None, **kw):
        self.calls.append(("scene", ws))

    def set_panda_rollout_scenes(self, rows=None):
        self.calls.append(("rows", None if rows is None else list(rows)))


class _Sim:
    def __init__(self, num_envs, panda_scenes=None, panda_scene=None):
        self.num_envs, self.panda_scenes, self.panda_scene = num_envs, panda_scenes, panda_scene


def _planner(K=8, K_local=8, k_offset=0, sim=None):
    from m3p2i_aip_amd import planner
    p = object.__new__(planner.MPPI)
    p.env_type, p.K, p.K_local, p.k_offset = "panda_env", K, K_local, k_offset
    p._engine, p._sim = _Engine(), sim
    p._bound_sim = sim            # (the binding of the views is not what these cases are about)
    p._fused, p.world_size, p.collective = True, 1, None
    return p


def test_planner_follows_the_rows_of_its_wrapper_and_pushes_only_on_change():
    rows = [{**D, "cube_m": 0.1 + 0.01 * i} for i in range(8)]
    sim = _Sim(8, rows)
    p = _planner(sim=sim)
    assert p.has_panda_rollout_scenes and not p.has_rollout_scenes
    p._bind_world(); p._bind_world()
    assert p._engine.calls == [("rows", rows)]                      # once
    sim.panda_scenes = [dict(r) for r in rows]                      # another list with the same rows: nothing to push
    p._bind_world()
    assert len(p._engine.calls) == 1
    sim.panda_scenes = rows[::-1]
    p._bind_world()
    assert p._engine.calls[-1] == ("rows", rows[::-1]) and len(p._engine.calls) == 2
    sim.panda_scene = dict(mu=0.5)                                  # the single workspace changes: it is pushed, and the rows again
    p._bind_world()
    assert p._engine.calls[2:] == [("scene", dict(mu=0.5)), ("rows", rows[::-1])]
    sim.panda_scenes = None                                         # the wrapper drops its rows: so does the planner
    p._bind_world(); p._bind_world()
    assert p._engine.calls[4:] == [("rows", None)] and not p.has_panda_rollout_scenes


def test_set_panda_rollout_scenes_takes_the_global_list_and_pushes_the_shards_slice():
    mine = [dict(mu=0.01 * (i + 1)) for i in range(16)]
    p = _planner(K=16, K_local=8, k_offset=8, sim=_Sim(16, [dict(D)] * 16))      # num_envs != K_local: not followed
    p._bind_world()
    assert p._engine.calls == [] and not p.has_panda_rollout_scenes
    p.set_panda_rollout_scenes(mine)
    assert p._engine.calls == [("rows", mine[8:16])] and p.has_panda_rollout_scenes
    p._bind_world()
    assert len(p._engine.calls) == 1
    with pytest.raises(ValueError, match="global list"):
        p.set_panda_rollout_scenes(mine[:8])
    p.set_panda_rollout_scenes(None)
    assert p._engine.calls[-1] == ("rows", None) and not p.has_panda_rollout_scenes
    # follow off keeps what was set by hand; following again, the wrapper's rows win
    rows = [{**D, "mu": 0.9}] * 8
    q = _planner(sim=_Sim(8, rows))
    q.follow_sim_scene = False
    q.set_panda_rollout_scenes(mine[:8])
    q._bind_world()
    assert q._engine.calls == [("rows", mine[:8])]
    q.follow_sim_scene = True
    q._bind_world()
    assert q._engine.calls[-1] == ("rows", rows)
    q.follow_sim_scene = False
    q._bind_world()
    assert q._engine.calls[-1] == ("rows", mine[:8]) and len(q._engine.calls) == 3
    # a point_env planner has no such rows
    from m3p2i_aip_amd import planner
    pt = object.__new__(planner.MPPI)
    pt.env_type = "point_env"
    with pytest.raises(ValueError, match="panda_env only"):
        pt.set_panda_rollout_scenes(mine)


def test_spread_panda_scenes():
    from m3p2i_aip_amd.scenes import spread_panda_scenes
    a = spread_panda_scenes(128, 0.3, seed=5)
    assert a == spread_panda_scenes(128, 0.3, seed=5) and a != spread_panda_scenes(128, 0.3, seed=6)
    assert spread_panda_scenes(64, 0.3, seed=5) == a[:64]                       # row i depends on (seed, i) only
    assert len({r["cube_m"] for r in a}) == 128 and set(a[0]) == {"cube_m", "mu", "obs_m"}
    for r in a:
        for n in ("cube_m", "mu", "obs_m"):
            assert 0.7 * D[n] <= r[n] <= 1.3 * D[n]
        L.panda_scene_fields(r)                                                 # every row is a legal override dict
    base = dict(mu=0.5, table=(0.0, 0.0, 0.99, 0.6, 0.6, 0.025))
    rows = spread_panda_scenes(64, 0.3, seed=2, base=base, fields=("mu", "obs_half"), nominal_rows=(0, 32, 63))
    assert rows[0] == rows[32] == rows[63] == base                              # the nominal rows stay nominal
    assert all(rows[i] != base and rows[i]["table"] == base["table"] for i in range(64) if i not in (0, 32, 63))
    assert spread_panda_scenes(64, 0.3, seed=2, base=base, fields=("mu", "obs_half"))[1:32] == rows[1:32]
    r = rows[1]["obs_half"]
    assert len(r) == 3 and abs(r[0] / 0.1 - r[2] / 0.01) < 1e-12                # an array field: one factor
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            spread_panda_scenes(4, bad)
    with pytest.raises(ValueError, match="unknown panda scene field"):
        spread_panda_scenes(4, 0.1, fields=("cube_size",))


def test_rollout_workspace_spread_config_key():
    from m3p2i_aip_amd import compat, scenes
    assert compat.make_config("config_panda").rollout_workspace_spread is None
    assert compat.rollout_panda_scenes(compat.make_config("config_panda")) is None
    cfg = compat.make_config("config_panda", ["mppi.num_samples=64", "panda_scene={mu: 0.5}",
                                              "rollout_workspace_spread={spread: 0.3, seed: 4, fields: [cube_m, mu]}"])
    assert cfg.rollout_workspace_spread == dict(spread=0.3, seed=4, fields=["cube_m", "mu"])
    rows = compat.rollout_panda_scenes(cfg)
    assert rows == scenes.spread_panda_scenes(64, 0.3, 4, base=dict(mu=0.5), fields=("cube_m", "mu"), nominal_rows=(0, 32, 63))
    assert rows[0] == rows[32] == rows[63] == dict(mu=0.5) and set(rows[1]) == {"cube_m", "mu"}
    assert compat.rollout_panda_scenes(cfg, k_offset=32, n=32) == rows[32:]
    for bad in ("rollout_workspace_spread={spread: 1.0}", "rollout_workspace_spread={seed: 1}",
                "rollout_workspace_spread={spread: 0.1, sed: 1}", "rollout_workspace_spread={spread: 0.1, fields: [cube_size]}"):
        with pytest.raises(ValueError):
            compat.make_config("config_panda", [bad])
    with pytest.raises(ValueError, match="panda_env only"):
        compat.make_config("config_point", ["rollout_workspace_spread={spread: 0.3}"])


def test_batched_paths_refuse_per_sample_workspaces_before_any_engine_call(monkeypatch):
    from m3p2i_aip_amd import planner
    from m3p2i_aip_amd.episodes import build_panda_set, run_panda_episodes
    monkeypatch.setattr(planner, "HipEngine", _Engine)      # (the stand-in passes for the library's engine: planner 0 is accepted)
    p = _planner(sim=_Sim(8, [dict(D)] * 8))
    with pytest.raises(ValueError, match="workspace per sample"):
        planner.command_batch([p], [np.zeros(18, F)])
    q = _planner(sim=_Sim(8))
    q._panda_rollout_scenes = [{}] * 8
    with pytest.raises(ValueError, match="planner 1 has a workspace per sample"):
        planner.command_batch([_planner(sim=_Sim(8)), q], [np.zeros(18, F)] * 2)
    assert p._engine.calls == [] and q._engine.calls == []                # before any call
    eps = [("config_panda", [], None), ("config_panda", ["rollout_workspace_spread={spread: 0.2}"], None)]
    for run in (run_panda_episodes, build_panda_set):
        with pytest.raises(ValueError, match="episode 1: .*rollout_workspace_spread"):
            run(eps, max_ticks=4)


def test_wrapper_checks_panda_scenes_before_it_touches_a_device():
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    with pytest.raises(ValueError, match="panda_scenes: panda_env only"):
        IsaacGymWrapper(IsaacGymConfig(), "point_env", num_envs=2, panda_scenes=[None, None])
    with pytest.raises(ValueError, match="panda_scenes: 3 entries for num_envs = 2"):
        IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=2, panda_scenes=[None] * 3)
    with pytest.raises(ValueError, match=r"panda_scenes\[1\]: unknown field"):
        IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=2, panda_scenes=[None, dict(cube_size=0.1)])
    with pytest.raises(ValueError, match=r"panda_scenes\[0\]: .*'table'"):
        IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=2, panda_scenes=[dict(table=(0.0, 0.0, 1.0)), None])
