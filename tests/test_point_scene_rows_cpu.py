"""One point_env arena per environment (m3_set_point_scene_rows) without a GPU.

1. The three entry points exist with the documented prototypes (header, ctypes table, library).
2. A host program (tests/native/point_scene_rows_host.cpp, its own main) packs three arenas -- the default, CUSTOM and CUSTOM_B
   of tests/point_scene_fixture.py -- into the word-major table as the library does, rebuilds each row's PointSceneRT as the
   kernels do and steps 65 worlds 8 times; row i in arena i % 3, from start world (i // 3) % 3, with rng(1).uniform(-3, 3)
   actions.  It equals oracle.step_batch with the row's own scene BIT FOR BIT (bound: none, the spec is a fixed sequence of
   binary32 operations).  Condition, on the oracle alone: at least half of the rows end in a state that differs in some bit
   from what EACH of the other two arenas gives that row -- a row mix-up cannot pass.  The same program is built and run once
   under -fsanitize=address,undefined.
3. Plumbing: the `world_point_scene` config key, the wrapper's argument checks, band_stats --world-arena-spread 0.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from m3p2i_aip_amd import _lib as L
from tests import point_scene_fixture as X
from tests.native_flags import host_flags
from tests.test_device_dynamics_on_host import HOST_FLAGS, fma_flag

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
N, STEPS = 65, 8
ARENAS = [None, X.CUSTOM, X.CUSTOM_B]
COLS = [c for c in range(31) if c not in (2, 3, 6)]     # robot (c, s, w) do not exist on the device


# ------------------------------------------------------------------ the recipe, shared with tests/test_point_scene_rows_gpu.py
def arena_of_row(n=N):
    return [i % 3 for i in range(n)]


def row_worlds(O, n=N):
    return X.start_worlds(O)[[(i // 3) % 3 for i in range(n)]].copy()


def row_actions(n=N, steps=STEPS):
    rng = np.random.default_rng(1)
    return np.stack([rng.uniform(-3, 3, (n, 2)).astype(F) for _ in range(steps)])


_ORACLE = {}


def oracle_rows(O, n=N, steps=STEPS):
    """[steps][n][31]: the oracle's worlds after each step, row i in its own arena; and the same with every row in arena
    (i + 1) % 3 and (i + 2) % 3.  Computed once per process, read-only."""
    if (n, steps) not in _ORACLE:
        u = row_actions(n, steps)
        outs = []
        for shift in range(3):
            w = row_worlds(O, n)
            hist = np.zeros((steps, n, 31), F)
            idx = [np.array([i for i in range(n) if (i + shift) % 3 == a]) for a in range(3)]
            for t in range(steps):
                for a in range(3):
                    part = w[idx[a]].copy()
                    O.step_batch(X.oracle_scene(O, ARENAS[a]), part, u[t][idx[a]].copy())
                    w[idx[a]] = part
                hist[t] = w
            hist.setflags(write=False)
            outs.append(hist)
        _ORACLE[(n, steps)] = outs
    return _ORACLE[(n, steps)]


# ------------------------------------------------------------------ 1. symbols
def test_the_three_entry_points_exist_with_their_prototypes():
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    assert "#define M3_ABI_VERSION 4" in hdr
    bound = {s[0]: (s[1], list(s[2])) for s in L.SYMBOLS}
    P = C.POINTER(L.PointSceneFields)
    assert bound["m3_set_point_scene_rows"] == (C.c_int, [L._H, P, C.c_int])
    assert bound["m3_get_point_scene_row"] == (C.c_int, [L._H, C.c_int, P])
    assert bound["m3_point_scene_rows_set"] == (C.c_int, [L._H])
    assert re.search(r"^int m3_set_point_scene_rows\(m3_handle\* h, const m3_point_scene\* scenes, int n\);", hdr, re.M)
    assert re.search(r"^int m3_get_point_scene_row\(const m3_handle\* h, int row, m3_point_scene\* out\);", hdr, re.M)
    assert re.search(r"^int m3_point_scene_rows_set\(const m3_handle\* h\);", hdr, re.M)
    lib = L.load()
    sc = L.PointSceneFields()
    for name in ("m3_set_point_scene_rows", "m3_get_point_scene_row", "m3_point_scene_rows_set"):
        assert hasattr(lib, name), name
    # (no handle can be created without a device -- the fresh handle's 0 is checked in tests/test_point_scene_rows_gpu.py)
    assert lib.m3_set_point_scene_rows(None, C.byref(sc), 1) == -1 and lib.m3_get_point_scene_row(None, 0, C.byref(sc)) == -1
    assert lib.m3_point_scene_rows_set(None) == -1


# ------------------------------------------------------------------ 2. the host program
def _build(tmp, extra=()):
    out = str(tmp / "point_scene_rows_host")
    flags = [f for f in host_flags(HOST_FLAGS) if f != "-shared"]
    subprocess.check_call(["g++"] + flags + fma_flag() + list(extra) + ["-I" + os.path.join(HERE, "native", "shim"),
                           os.path.join(HERE, "native", "point_scene_rows_host.cpp"), "-o", out])
    return out


def _run(O, prog, tmp, env=None):
    scenes = np.stack([X.scene_array(a) for a in ARENAS]).astype(F)
    head = np.array([N, STEPS, len(ARENAS), 2, 6], np.int32)
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(fin, "wb") as f:
        for part in (head, np.array([0.05], F), scenes, np.array(arena_of_row(), np.int32), row_worlds(O).astype(F), row_actions()):
            f.write(np.ascontiguousarray(part).tobytes())
    r = subprocess.run([prog, fin, fout], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return np.fromfile(fout, F).reshape(STEPS, N, 31), r.stderr


def _assert_rows_equal_the_oracle(O, got):
    want = oracle_rows(O)[0]
    neq = got[:, :, COLS].view(np.uint32) != want[:, :, COLS].view(np.uint32)
    if neq.any():
        t, r, c = np.argwhere(neq)[0]
        raise AssertionError(f"step {t} row {r} (arena {r % 3}) column {COLS[c]}: oracle {want[t, r, COLS[c]]!r} "
                             f"device-source {got[t, r, COLS[c]]!r} ({int(neq.sum())} values differ)")


def test_the_arenas_tell_the_rows_apart(oracle):
    """the condition of every case of this feature, on the oracle alone"""
    own, a, b = (h[-1][:, COLS].view(np.uint32) for h in oracle_rows(oracle))
    assert np.isfinite(oracle_rows(oracle)[0]).all()
    differs = (own != a).any(1) & (own != b).any(1)
    assert differs.mean() >= 0.5, differs.mean()


def test_rows_through_the_table_equal_the_oracle_row_by_row(oracle, tmp_path):
    got, _ = _run(oracle, _build(tmp_path), tmp_path)
    _assert_rows_equal_the_oracle(oracle, got)


def test_the_host_program_is_clean_under_asan_and_ubsan(oracle, tmp_path):
    prog = _build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    got, err = _run(oracle, prog, tmp_path, env=env)
    assert "AddressSanitizer" not in err and "runtime error" not in err, err[-2000:]
    _assert_rows_equal_the_oracle(oracle, got)


# ------------------------------------------------------------------ 3. plumbing
def test_world_point_scene_config_key():
    from m3p2i_aip_amd import compat
    cfg = compat.make_config("config_point", ["point_scene={obs_x: -1.0, wall: 2.95}", "world_point_scene={box_m: 20.0, wall: 3.0}"])
    assert dict(cfg.world_point_scene) == {"box_m": 20.0, "wall": 3.0}
    assert dict(cfg.isaacgym.point_scene) == {"obs_x": -1.0, "wall": 2.95}          # what the planner's simulator is built from
    assert compat.world_point_scene(cfg) == {"obs_x": -1.0, "wall": 3.0, "box_m": 20.0}
    world = compat.world_isaacgym_config(cfg)
    assert world is not cfg.isaacgym and dict(world.point_scene) == {"obs_x": -1.0, "wall": 3.0, "box_m": 20.0}
    assert (world.dt, world.substeps) == (cfg.isaacgym.dt, cfg.isaacgym.substeps)
    plain = compat.make_config("config_point", ["point_scene={obs_x: -1.0}"])
    assert plain.world_point_scene is None and compat.world_isaacgym_config(plain) is plain.isaacgym
    assert compat.world_point_scene(compat.make_config("config_point")) == {}
    with pytest.raises(ValueError, match="world_point_scene"):
        compat.make_config("config_panda", ["world_point_scene={box_m: 20.0}"])


def test_wrapper_refuses_a_wrong_length_and_unknown_fields():
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    with pytest.raises(ValueError, match="3 entries for num_envs = 4"):
        IsaacGymWrapper(IsaacGymConfig(dt=0.05), "point_env", num_envs=4, point_scenes=[None, {}, dict(wall=2.0)])
    with pytest.raises(ValueError, match=r"point_scenes\[1\].*box_mass"):
        IsaacGymWrapper(IsaacGymConfig(dt=0.05), "point_env", num_envs=2, point_scenes=[None, dict(box_mass=3.0)])
    with pytest.raises(ValueError, match="point_env only"):
        IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=2, point_scenes=[None, None])


def test_band_stats_spread_zero_builds_the_same_episodes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import band_stats as bs
    pairs = [("case2_halton_push_coll", "default"), ("corner2_hybrid", "baseline")]
    items, eps = bs.batched_episode_list(pairs, 5)
    items0, eps0 = bs.batched_episode_list(pairs, 5, world_arena_spread=0.0)
    assert repr((items, eps)) == repr((items0, eps0))
    assert eps == [("config_point", bs.overrides(sc, size), bs.jitter_of(sc, e)) for sc, size in pairs for e in range(5)]
    # and with a spread: episode 0 nominal, the others carry four fields inside the band, box_I in step with box_m
    from m3p2i_aip_amd import compat
    _, eps2 = bs.batched_episode_list(pairs, 5, world_arena_spread=0.2)
    assert eps2[0] == eps[0] and [j for *_, j in eps2] == [j for *_, j in eps]
    D = L.POINT_SCENE_DEFAULTS
    seen = set()
    for (cn, ov, _), (_, ov_plain, _) in zip(eps2[1:5], eps[1:5]):
        assert ov[:-1] == ov_plain
        w = compat.make_config(cn, ov).world_point_scene
        assert sorted(w) == ["box_I", "box_m", "box_mu_g", "mu_rb"]
        for k in w:
            assert 0.8 * D[k] <= w[k] <= 1.2 * D[k], (k, w[k])
        assert abs(w["box_I"] / D["box_I"] - w["box_m"] / D["box_m"]) < 1e-12
        seen.add(w["box_m"])
    assert len(seen) == 4
