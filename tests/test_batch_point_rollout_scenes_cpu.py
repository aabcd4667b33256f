"""Batched command and lockstep episodes of point_env planners with an arena per sample (m3_batch_create_sections,
m3_episodes_create_ex; DESIGN.md sections 7b.3 and 7c3), the parts that need no GPU: the symbols and the ABI, the four-section
layout of the argument table as a host program (tests/native/batch_table_layout_host.cpp in its mode `sv`, once plain and once under
-fsanitize=address,undefined), and the Python paths on the recording stand-in engine of tests/test_point_rollout_scenes_cpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from m3p2i_aip_amd import _lib as L
from tests.test_point_rollout_scenes_cpu import _Engine, _Sim, _planner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
D = L.POINT_SCENE_DEFAULTS


# ------------------------------------------------------------------ 1. symbols and ABI
def test_the_entry_points_and_defines_are_in_the_ext_header_only():
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    ext = open(os.path.join(ROOT, "include", "m3p2i_hip_ext.h")).read()
    assert "#define M3_ABI_VERSION 4" in hdr and L.ABI_VERSION == 4
    for define, value in (("M3_BATCH_SECTION_PANDA_RUNTIME", 1), ("M3_BATCH_SECTION_POINT_ROLLOUT_SCENES", 2),
                          ("M3_EPISODES_ROLLOUT_SCENES", 1)):
        assert re.search(rf"^#define {define} {value}$", ext, re.M), define
        assert define not in hdr
    assert (L.BATCH_SECTION_PANDA_RUNTIME, L.BATCH_SECTION_POINT_ROLLOUT_SCENES, L.EPISODES_ROLLOUT_SCENES) == (1, 2, 1)
    assert L.BATCH_SECTION_PANDA_RUNTIME == L.BATCH_PANDA_RUNTIME
    assert re.search(r"^int m3_batch_create_sections\(int device, int max_handles, int sections, m3_batch\*\* out\);", ext, re.M)
    assert re.search(r"^int m3_episodes_create_ex\(m3_handle\* world, m3_handle\* const\* planners, const m3_episode_spec\* specs, "
                     r"int n, int max_ticks,\n\s+int trace, int flags, m3_episodes\*\* out\);", ext, re.M)
    assert re.search(r"^int m3_episodes_flags\(const m3_episodes\* eps\);", ext, re.M)
    main, extra = {s[0] for s in L.SYMBOLS}, {s[0]: (s[1], list(s[2])) for s in L.SYMBOLS_EXT}
    PH = C.POINTER(L._H)
    assert extra["m3_batch_create_sections"] == (C.c_int, [C.c_int, C.c_int, C.c_int, PH])
    assert extra["m3_episodes_create_ex"] == (C.c_int, [L._H, PH, C.POINTER(L.EpisodeSpec), C.c_int, C.c_int, C.c_int, C.c_int, PH])
    assert extra["m3_episodes_flags"] == (C.c_int, [L._H])
    for name in ("m3_batch_create_sections", "m3_episodes_create_ex", "m3_episodes_flags"):
        assert name not in main
        assert name not in hdr
    # the main header points at the ext header where it used to say "stay refused"
    assert "stay refused by the batches of this\n * header; m3p2i_hip_ext.h declares the call" in hdr


def test_unknown_bits_and_null_objects_are_refused_without_a_device():
    lib = L.load()
    assert lib.m3_abi_version() == 4
    for bits in (4, 8, 1 | 4, 2 | 16, -1):
        assert lib.m3_batch_create_sections(0, 1, bits, None) == -1
        assert b"unknown section bits" in lib.m3_batch_last_error(None)
    for bits in (2, 4, 1 | 2, -1):
        assert lib.m3_episodes_create_ex(None, None, None, 1, 1, 0, bits, None) == -1
        assert b"unknown flag bits" in lib.m3_episodes_last_error(None)
    # known bits: the checks of the calls they extend, in their words
    assert lib.m3_batch_create_sections(0, 1, 2, None) == -1 and b"m3_batch_create: null argument" in lib.m3_batch_last_error(None)
    out = C.c_void_p(1)
    assert lib.m3_batch_create_sections(0, 0, 3, C.byref(out)) == -1 and out.value is None
    assert b"max_handles must be in 1 .. 65535" in lib.m3_batch_last_error(None)
    assert lib.m3_batch_create_sections(0, 4, 8, C.byref(out)) == -1 and out.value is None
    for flags in (0, 1):
        eps = C.c_void_p(1)
        assert lib.m3_episodes_create_ex(None, None, None, 1, 1, 0, flags, C.byref(eps)) == -1 and eps.value is None
        assert lib.m3_episodes_last_error(None) == b"m3_episodes_create: null argument"
    assert lib.m3_episodes_flags(None) == -1 and lib.m3_batch_flags(None) == -1


# ------------------------------------------------------------------ 2. the four-section layout, as a host program
def _build(tmp, extra=("-O2",)):
    out = str(tmp / "batch_table_layout_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + list(extra) +
                          [os.path.join(HERE, "native", "batch_table_layout_host.cpp"), "-o", out])
    return out


def _run(prog, env=None):
    r = subprocess.run([prog, "sv"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    m = re.fullmatch(r"(\d+) checks, 0 failures\n", r.stdout)
    assert m and int(m.group(1)) > 10000, r.stdout
    return r.stderr


def test_every_four_section_split_is_aligned_ordered_disjoint_and_fits_the_slot(tmp_path):
    _run(_build(tmp_path))


def test_the_four_section_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    prog = _build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    err = _run(prog, env=env)
    assert "AddressSanitizer" not in err and "runtime error" not in err, err[-2000:]


def test_the_entry_sizes_of_the_host_program_are_the_pinned_ones():
    src = open(os.path.join(ROOT, "m3p2i_aip_amd", "csrc", "m3_internal.hpp")).read()
    assert re.search(r"sizeof\(BatchRolloutEntrySV\) == 768 && offsetof\(BatchRolloutEntrySV, sc\) == 528 &&\s+"
                     r"offsetof\(BatchRolloutEntrySV, wt\) == 724 && offsetof\(BatchRolloutEntrySV, rows\) == 760", src)
    assert "sizeof(BatchRolloutEntryS) == 760" in src and "sizeof(BatchRolloutEntryW) == 616" in src and "sizeof(BatchRolloutEntry) == 584" in src


# ------------------------------------------------------------------ 3. the Python paths on a recording engine
class _BatchEngine(_Engine):
    """the stand-in of tests/test_point_rollout_scenes_cpu.py with what command_batch touches of an engine"""

    class cfg:
        env_type = "point_env"

    class device:
        index = 0

    def use_torch_stream(self):
        self.calls.append(("stream",))


class _Batch:
    made = []

    def __init__(self, max_handles, device=0, panda_runtime=False, point_runtime=False):
        self.max_handles, self.kw, self.commands = max_handles, dict(panda_runtime=panda_runtime, point_runtime=point_runtime), []
        _Batch.made.append(self)

    def command(self, engines):
        self.commands.append(list(engines))

    def close(self):
        pass


@pytest.fixture
def batch_planner(monkeypatch):
    import torch
    from m3p2i_aip_amd import planner
    monkeypatch.setattr(planner, "HipEngine", _BatchEngine)
    monkeypatch.setattr(planner, "HipBatch", _Batch)
    for cache in ("_BATCHES", "_BATCHES_PANDA_RUNTIME", "_BATCHES_POINT_RUNTIME"):
        monkeypatch.setattr(planner, cache, {})
    for name in ("_ensure_noise", "_push_objective"):
        monkeypatch.setattr(planner.MPPI, name, lambda self: None)
    monkeypatch.setattr(planner.MPPI, "_next_action_slot", lambda self: "slot")
    _Batch.made = []

    def make(rows):
        p = _planner(sim=_Sim(8, rows))
        p._engine = _BatchEngine()
        p.tensor_args = dict(device="cpu", dtype=torch.float32)
        return p
    return planner, make


def test_command_batch_default_still_raises_and_point_runtime_reaches_the_engine(batch_planner):
    planner, make = batch_planner
    rows = [{**D, "box_m": 10.0 + i} for i in range(8)]
    p, q = make(rows), make(None)
    with pytest.raises(ValueError, match="planner 0 has an arena per sample"):
        planner.command_batch([p, q], [np.zeros(4, F)] * 2)
    with pytest.raises(ValueError, match="planner 0 has an arena per sample"):
        planner.command_batch([p, q], [np.zeros(4, F)] * 2, panda_runtime=True)
    assert p._engine.calls == [] and q._engine.calls == [] and _Batch.made == []
    outs = planner.command_batch([p, q], [np.zeros(4, F)] * 2, point_runtime=True)
    assert outs == ["slot", "slot"]
    assert ("rows", rows) in p._engine.calls and all(c[0] != "rows" for c in q._engine.calls)   # the planner's own _bind_world
    assert len(_Batch.made) == 1
    b = _Batch.made[0]
    assert b.kw == dict(panda_runtime=False, point_runtime=True) and b.commands == [[p._engine, q._engine]]
    # the batch is cached per device, next to the default one and the panda one
    planner.command_batch([p, q], [np.zeros(4, F)] * 2, point_runtime=True)
    assert len(_Batch.made) == 1 and len(b.commands) == 2
    planner.command_batch([q], [np.zeros(4, F)])
    planner.command_batch([q], [np.zeros(4, F)], panda_runtime=True)
    planner.command_batch([q], [np.zeros(4, F)], panda_runtime=True, point_runtime=True)
    assert [m.kw for m in _Batch.made[1:]] == [dict(panda_runtime=False, point_runtime=False), dict(panda_runtime=True, point_runtime=False),
                                               dict(panda_runtime=True, point_runtime=True)]
    assert len(b.commands) == 2


class _Stop(Exception):
    pass


def test_build_set_hands_the_planners_sim_the_rollout_rows(monkeypatch):
    from m3p2i_aip_amd import compat, isaacgym_wrapper
    from m3p2i_aip_amd.episodes import build_set, run_point_episodes
    seen = []

    def wrapper(*a, **kw):
        seen.append(kw)
        raise _Stop()
    monkeypatch.setattr(isaacgym_wrapper, "IsaacGymWrapper", wrapper)
    spread = ["task=push", "mppi.num_samples=64", "rollout_arena_spread={spread: 0.3, seed: 1}"]
    nominal = ["task=push", "mppi.num_samples=64", "point_scene={wall: 2.95}"]
    # the default: today's errors, before any simulator is built
    for run in (run_point_episodes, build_set):
        with pytest.raises(ValueError, match="episode 1 .*rollout_arena_spread"):
            run([("config_point", nominal, None), ("config_point", spread, None)], max_ticks=4)
    assert seen == []
    # point_runtime: the first planner's K-env simulator gets the rows closed_loop.Tamp would give it
    for run in (run_point_episodes, build_set):
        seen.clear()
        with pytest.raises(_Stop):
            run([("config_point", spread, None), ("config_point", nominal, None)], max_ticks=4, point_runtime=True)
        rows = compat.rollout_point_scenes(compat.make_config("config_point", spread))
        assert len(seen) == 1 and seen[0]["num_envs"] == 64 and seen[0]["point_scenes"] == rows and len(rows) == 64
        assert rows[0] == rows[32] == rows[63] and rows[1] != rows[0]
    # ... and a planner without the key none: compat.rollout_point_scenes is None for it
    seen.clear()
    with pytest.raises(_Stop):
        build_set([("config_point", nominal, None), ("config_point", spread, None)], max_ticks=4, point_runtime=True)
    assert len(seen) == 1 and seen[0].get("point_scenes") is None
    # without point_runtime the wrapper is built exactly as before (no such keyword)
    seen.clear()
    with pytest.raises(_Stop):
        build_set([("config_point", nominal, None)], max_ticks=4)
    assert len(seen) == 1 and "point_scenes" not in seen[0]
