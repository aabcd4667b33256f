"""One arena per SAMPLE of the fused point_env rollout (m3_set_point_rollout_scenes), the parts that need no GPU: the spread
helper, the rollout plan, the planner's precedence rules on a recording stand-in engine, the config key, the Python-side
refusals, the stitched oracle the GPU tests compare against, and the header / ctypes layout of the three entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from m3p2i_aip_amd import _lib as L
from tests import point_scene_fixture as X
from tests import rollout_scenes_fixture as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
D = L.POINT_SCENE_DEFAULTS


# ------------------------------------------------------------------ 1. spread_point_scenes
def test_spread_is_deterministic_and_row_i_depends_on_seed_and_i_only():
    from m3p2i_aip_amd.scenes import spread_point_scenes
    a, b = spread_point_scenes(128, 0.3, seed=5), spread_point_scenes(128, 0.3, seed=5)
    assert a == b and len(a) == 128
    assert spread_point_scenes(128, 0.3, seed=6) != a
    # a shard's slice is the slice of the global list, and a longer list starts with the shorter one
    assert spread_point_scenes(64, 0.3, seed=5) == a[:64]
    assert [spread_point_scenes(128, 0.3, seed=5)[i] for i in range(64, 128)] == a[64:128]
    assert len({r["box_m"] for r in a}) == 128


def test_spread_factors_stay_in_range_and_the_inertia_follows_the_mass():
    from m3p2i_aip_amd.scenes import spread_point_scenes
    base = dict(box_m=9.0, box_I=0.3375, wall=2.95)
    rows = spread_point_scenes(500, 0.25, seed=1, base=base, fields=("box_m", "box_mu_g", "mu_rb", "dyn_m"))
    full = {**D, **base}
    for r in rows:
        assert r["wall"] == 2.95 and set(r) == {"wall", "box_m", "box_I", "box_mu_g", "mu_rb", "dyn_m", "dyn_I"}
        for n in ("box_m", "box_mu_g", "mu_rb", "dyn_m"):
            assert 0.75 * full[n] <= r[n] <= 1.25 * full[n], (n, r[n])
        assert abs(r["box_I"] / r["box_m"] - full["box_I"] / full["box_m"]) <= 1e-12
        assert abs(r["dyn_I"] / r["dyn_m"] - full["dyn_I"] / full["dyn_m"]) <= 1e-12
    f = np.array([r["box_m"] / 9.0 for r in rows])
    assert f.min() < 0.8 and f.max() > 1.2            # (500 uniform draws: the range is used)
    assert all(r == {} for r in spread_point_scenes(8, 0.0, fields=()))


def test_spread_keeps_the_nominal_rows_and_refuses_a_bad_spread():
    from m3p2i_aip_amd.scenes import spread_point_scenes
    base = dict(mu_rb=0.4)
    rows = spread_point_scenes(64, 0.3, seed=2, base=base, nominal_rows=(0, 32, 63))
    assert rows[0] == rows[32] == rows[63] == base
    assert all(rows[i] != base for i in range(64) if i not in (0, 32, 63))
    assert spread_point_scenes(64, 0.3, seed=2, base=base)[1:32] == rows[1:32]       # the other rows are what they were
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            spread_point_scenes(4, bad)
    with pytest.raises(ValueError):
        spread_point_scenes(4, 0.1, fields=("box_mass",))


# ------------------------------------------------------------------ 2. the rollout plan (host only)
def _plan(task, mm, scene, K, lanes=64, weighted=0, form_request=0, minima=0):
    out = (C.c_int * 8)()
    assert L.load().m3_point_rollout_plan(task, int(mm), 0, 0, 0, K, 30, lanes, 0.05, 2, 6, weighted, scene, form_request, minima, out) == 0
    return dict(zip(("instance", "ref", "form", "weighted", "scene", "blocks", "rows", "lanes"), out))


@pytest.mark.parametrize("task,mm", [(0, False), (1, False), (2, False), (3, True)])
def test_the_plan_of_a_handle_with_rows(task, mm):
    for K, blocks in ((64, 1), (65, 2), (65537, 1025)):
        for form_request in (0, 1, -1):
            for weighted in (0, 1):
                p = _plan(task, mm, 2, K, weighted=weighted, form_request=form_request)
                assert p == dict(instance=-1, ref=0, form=0, weighted=1, scene=2, blocks=blocks, rows=0, lanes=64), (K, p)
        # scene = 0 and 1 keep their answers
        assert _plan(task, mm, 1, K) == dict(instance=-1, ref=0, form=0, weighted=1, scene=1, blocks=blocks, rows=0, lanes=64)
        p0 = _plan(task, mm, 0, K)
        assert (p0["instance"], p0["ref"], p0["weighted"], p0["scene"], p0["blocks"]) == (task, 1, 0, 0, blocks)
    assert _plan(task, mm, 2, 2000, minima=1)["rows"] == 32
    out = (C.c_int * 8)()
    assert L.load().m3_point_rollout_plan(task, int(mm), 0, 0, 0, 64, 30, 64, 0.05, 2, 6, 0, 3, 0, 0, out) == -1


# ------------------------------------------------------------------ 3. planner precedence on a recording engine
class _Engine:
    def __init__(self):
        self.calls = []

    def set_point_scene(self, arena=None, **kw):
        self.calls.append(("scene", arena))

    def set_point_rollout_scenes(self, rows=None):
        self.calls.append(("rows", None if rows is None else list(rows)))


class _Sim:
    def __init__(self, num_envs, point_scenes=None, point_scene=None):
        self.num_envs, self.point_scenes, self.point_scene = num_envs, point_scenes, point_scene


def _planner(K=8, K_local=8, k_offset=0, sim=None):
    from m3p2i_aip_amd import planner
    p = object.__new__(planner.MPPI)
    p.env_type, p.K, p.K_local, p.k_offset = "point_env", K, K_local, k_offset
    p._engine, p._sim = _Engine(), sim
    p._bound_sim = sim            # (the binding of the views is not what these cases are about)
    p._fused, p.world_size, p.collective = True, 1, None
    return p


def test_planner_follows_the_rows_of_its_wrapper_and_pushes_only_on_change():
    rows = [{**D, "box_m": 10.0 + i} for i in range(8)]
    sim = _Sim(8, rows)
    p = _planner(sim=sim)
    assert p.has_rollout_scenes
    p._bind_world(); p._bind_world()
    assert p._engine.calls == [("rows", rows)]                      # once
    sim.point_scenes = [dict(r) for r in rows]                      # another list with the same rows: nothing to push
    p._bind_world()
    assert len(p._engine.calls) == 1
    sim.point_scenes = rows[::-1]
    p._bind_world()
    assert p._engine.calls[-1] == ("rows", rows[::-1]) and len(p._engine.calls) == 2
    sim.point_scene = dict(wall=2.95)                               # the single arena changes: it is pushed, and the rows again
    p._bind_world()
    assert p._engine.calls[2:] == [("scene", dict(wall=2.95)), ("rows", rows[::-1])]
    sim.point_scenes = None                                         # the wrapper drops its rows: so does the planner
    p._bind_world(); p._bind_world()
    assert p._engine.calls[4:] == [("rows", None)] and not p.has_rollout_scenes


def test_planner_with_follow_off_keeps_what_was_set_by_hand():
    rows = [{**D, "box_m": 10.0 + i} for i in range(8)]
    mine = [dict(mu_rb=0.1 * (i + 1)) for i in range(8)]
    p = _planner(sim=_Sim(8, rows))
    p.follow_sim_scene = False
    p.set_rollout_scenes(mine)
    p._bind_world()
    assert p._engine.calls == [("rows", mine)] and p.has_rollout_scenes
    p.follow_sim_scene = True                                       # following again: the wrapper's rows win
    p._bind_world()
    assert p._engine.calls[-1] == ("rows", rows)
    p.follow_sim_scene = False                                      # ... and off again: back to the rows set by hand
    p._bind_world()
    assert p._engine.calls[-1] == ("rows", mine) and len(p._engine.calls) == 3
    p.set_rollout_scenes(None)
    assert p._engine.calls[-1] == ("rows", None) and not p.has_rollout_scenes


def test_planner_pushes_its_shards_slice_and_ignores_a_wrapper_of_another_size():
    mine = [dict(mu_rb=0.01 * (i + 1)) for i in range(16)]
    p = _planner(K=16, K_local=8, k_offset=8, sim=_Sim(16, [dict(D)] * 16))      # num_envs != K_local: not followed
    p._bind_world()
    assert p._engine.calls == [] and not p.has_rollout_scenes
    p.set_rollout_scenes(mine)
    assert p._engine.calls == [("rows", mine[8:16])]
    p._bind_world()
    assert len(p._engine.calls) == 1
    with pytest.raises(ValueError):
        p.set_rollout_scenes(mine[:8])                                          # the global list, not the slice
    # a wrapper without rows behaves as before: the arena alone, and rows set by hand come back behind it
    q = _planner(sim=_Sim(8, None, dict(wall=2.0)))
    q._bind_world()
    assert q._engine.calls == [("scene", dict(wall=2.0))]
    q.set_rollout_scenes(mine[:8])
    q._sim.point_scene = dict(wall=2.5)
    q._bind_world()
    assert q._engine.calls[1:] == [("rows", mine[:8]), ("scene", dict(wall=2.5)), ("rows", mine[:8])]


# ------------------------------------------------------------------ 4. the config key and the Python-side refusals
def test_rollout_arena_spread_config_key():
    from m3p2i_aip_amd import compat, scenes
    assert compat.make_config("config_point").rollout_arena_spread is None
    assert compat.rollout_point_scenes(compat.make_config("config_point")) is None
    cfg = compat.make_config("config_point", ["mppi.num_samples=64", "point_scene={wall: 2.95}",
                                              "rollout_arena_spread={spread: 0.3, seed: 4, fields: [box_m, mu_rb]}"])
    assert cfg.rollout_arena_spread == dict(spread=0.3, seed=4, fields=["box_m", "mu_rb"])
    rows = compat.rollout_point_scenes(cfg)
    assert rows == scenes.spread_point_scenes(64, 0.3, 4, base=dict(wall=2.95), fields=("box_m", "mu_rb"), nominal_rows=(0, 32, 63))
    assert rows[0] == rows[32] == rows[63] == dict(wall=2.95) and set(rows[1]) == {"wall", "box_m", "box_I", "mu_rb"}
    assert compat.rollout_point_scenes(cfg, k_offset=32, n=32) == rows[32:]
    for bad in ("rollout_arena_spread={spread: 1.0}", "rollout_arena_spread={seed: 1}", "rollout_arena_spread={spread: 0.1, sed: 1}"):
        with pytest.raises(ValueError):
            compat.make_config("config_point", [bad])
    with pytest.raises(ValueError, match="point_env only"):
        compat.make_config("config_panda", ["rollout_arena_spread={spread: 0.3}"])


def test_batched_paths_refuse_a_planner_with_rollout_scenes(monkeypatch):
    from m3p2i_aip_amd import planner
    from m3p2i_aip_amd.episodes import build_set, run_point_episodes
    monkeypatch.setattr(planner, "HipEngine", _Engine)      # (the stand-in passes for the library's engine: planner 0 is accepted)
    p = _planner(sim=_Sim(8, [dict(D)] * 8))
    with pytest.raises(ValueError, match="arena per sample"):
        planner.command_batch([p], [np.zeros(4, F)])
    q = _planner(sim=_Sim(8))
    q._rollout_scenes = [{}] * 8
    with pytest.raises(ValueError, match="planner 1 has an arena per sample"):
        planner.command_batch([_planner(sim=_Sim(8)), q], [np.zeros(4, F)] * 2)
    assert p._engine.calls == [] and q._engine.calls == []                # before any call
    eps = [("config_point", ["task=push"], None), ("config_point", ["task=push", "rollout_arena_spread={spread: 0.2}"], None)]
    for run in (run_point_episodes, build_set):
        with pytest.raises(ValueError, match="episode 1 .*rollout_arena_spread"):
            run(eps, max_ticks=4)


# ------------------------------------------------------------------ 5. the reference of the GPU tests
@pytest.mark.parametrize("task,mm", [("push", False), ("push_pull", True)])
def test_stitched_oracle_with_equal_rows_is_the_single_scene_oracle(oracle, task, mm):
    K = 64
    w0 = X.start_worlds(oracle)[2]
    mk = lambda: oracle.make_cfg(K, X.T, 2, task=task, goal=X.GOAL, multi_modal=mm, filter_u=False)
    a = R.make_stitched(oracle, mk(), X.actions(K, X.T), [X.CUSTOM] * K)
    b = oracle.OraclePointPlanner(mk(), X.actions(K, X.T), scene=X.oracle_scene(oracle, X.CUSTOM))
    c = R.make_stitched(oracle, mk(), X.actions(K, X.T), [X.CUSTOM if i % 2 else dict(X.CUSTOM) for i in range(K)])
    for call in range(3):
        ua, ub, uc = a.command(w0), b.command(w0), c.command(w0)
        assert ua.tobytes() == ub.tobytes() == uc.tobytes(), call
        for name in ("states", "actions", "cost_h", "J"):
            assert a.last[name].tobytes() == b.last[name].tobytes() == c.last[name].tobytes(), (call, name)
        assert a.pend.tobytes() == b.pend.tobytes()


def test_the_cycle_of_rows_is_felt_by_the_samples(oracle):
    """the guard of the GPU cases, at its smallest margin (push_pull, K = 64, the start world at the walls)"""
    nxt, prv, dflt = R.row_shares(oracle, "push_pull", True, 64, X.start_worlds(oracle)[1])
    assert (nxt, prv, dflt) == (0.859375, 0.875, 0.5625)


# ------------------------------------------------------------------ 6. symbols
def test_the_three_entry_points_exist_with_their_prototypes():
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    assert "#define M3_ABI_VERSION 4" in hdr
    bound = {s[0]: (s[1], list(s[2])) for s in L.SYMBOLS}
    P = C.POINTER(L.PointSceneFields)
    assert bound["m3_set_point_rollout_scenes"] == (C.c_int, [L._H, P, C.c_int])
    assert bound["m3_get_point_rollout_scene"] == (C.c_int, [L._H, C.c_int, P])
    assert bound["m3_point_rollout_scenes_set"] == (C.c_int, [L._H])
    assert re.search(r"^int m3_set_point_rollout_scenes\(m3_handle\* h, const m3_point_scene\* scenes, int n\);", hdr, re.M)
    assert re.search(r"^int m3_get_point_rollout_scene\(const m3_handle\* h, int row, m3_point_scene\* out\);", hdr, re.M)
    assert re.search(r"^int m3_point_rollout_scenes_set\(const m3_handle\* h\);", hdr, re.M)
    lib = L.load()
    sc = L.PointSceneFields()
    # (no handle can be created without a device -- the handle's answers are checked in tests/test_point_rollout_scenes_gpu.py)
    assert lib.m3_set_point_rollout_scenes(None, C.byref(sc), 1) == -1 and lib.m3_get_point_rollout_scene(None, 0, C.byref(sc)) == -1
    assert lib.m3_point_rollout_scenes_set(None) == -1
