"""The batched command for panda_env planners with a run-time workspace, tuned weights or a workspace per sample (a batch created
with M3_BATCH_PANDA_RUNTIME; include/m3p2i_hip.h) without a GPU:

1. the two-section panda table of csrc/batch_table_layout.hpp, run by a host program with its own main
   (tests/native/batch_table_layout_host.cpp in its mode `rt`, plain and under ASan + UBSan) on the entry sizes that a second host program
   (tests/native/batch_panda_entry_sizes.hip, the host side of the library's own header) derives with sizeof;
2. the ctypes declarations against the header, and the thirteen kernels in the built library;
3. planner.command_batch(..., panda_runtime=True): the three panda refusals are lifted and a batch created with the flag is
   used and kept next to the default one; without the keyword each planner is refused with its existing message.
"""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32


# ------------------------------------------------------------------ 1. the layout
@pytest.fixture(scope="module")
def entry_sizes(tmp_path_factory):
    """sizeof / alignof of BatchPandaEntry, BatchPandaEntryRT and UpdateArgs from the library's header (host side only)"""
    out = str(tmp_path_factory.mktemp("entry_sizes") / "batch_panda_entry_sizes")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only", "-std=c++17", "-I" + os.path.join(ROOT, "m3p2i_aip_amd", "csrc"),
                           os.path.join(HERE, "native", "batch_panda_entry_sizes.hip"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    v = [int(x) for x in r.stdout.split()]
    assert len(v) == 6 and all(x > 0 for x in v), r.stdout
    return v


def _build_layout(tmp, extra=("-O2",)):
    out = str(tmp / "batch_table_layout_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + list(extra) +
                          [os.path.join(HERE, "native", "batch_table_layout_host.cpp"), "-o", out])
    return out


def _run_layout(prog, sizes, env=None):
    r = subprocess.run([prog, "rt"] + [str(x) for x in sizes], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    m = re.fullmatch(r"(\d+) checks, 0 failures\n", r.stdout)
    assert m and int(m.group(1)) > 500, r.stdout
    return r.stderr


def test_the_run_time_entry_is_the_larger_one_and_needs_no_more_than_the_sections_alignment(entry_sizes):
    entry, entry_rt, update, a_entry, a_rt, a_update = entry_sizes
    assert entry_rt > entry                      # why the capability is opt-in at create: the slots are sized for the largest entry
    assert 16 % a_entry == 0 and 16 % a_rt == 0 and 16 % a_update == 0


def test_two_sections_for_1_5_and_64_handles_in_every_split(tmp_path, entry_sizes):
    _run_layout(_build_layout(tmp_path), entry_sizes)


def test_the_layout_program_is_clean_under_asan_and_ubsan(tmp_path, entry_sizes):
    prog = _build_layout(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    err = _run_layout(prog, entry_sizes, env=env)
    assert "AddressSanitizer" not in err and "runtime error" not in err, err[-2000:]


# ------------------------------------------------------------------ 2. declarations and kernels
def test_ctypes_declarations_match_the_header():
    from m3p2i_aip_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    assert L.BATCH_PANDA_RUNTIME == 1 and re.search(r"^#define M3_BATCH_PANDA_RUNTIME 1$", hdr, re.M)
    assert "#define M3_ABI_VERSION 4" in hdr
    bound = {n: (r, a) for n, r, a in L.SYMBOLS}
    assert bound["m3_batch_create_ex"] == (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)])
    assert bound["m3_batch_flags"] == (C.c_int, [C.c_void_p])
    assert bound["m3_batch_create"] == (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)])          # (as before)
    assert re.search(r"\bint m3_batch_create_ex\(int device, int max_handles, int flags, m3_batch\*\* out\);", hdr)
    assert re.search(r"\bint m3_batch_flags\(const m3_batch\* b\);", hdr)
    # the three paragraphs no longer say NOT batched for the panda setters; the point_env one still does
    for setter in ("m3_set_panda_scene", "m3_set_panda_cost_weights", "m3_set_panda_rollout_scenes"):
        doc = hdr[:hdr.index("int %s(" % setter)]
        doc = doc[doc.rindex("/*"):]
        assert "NOT batched" not in doc and "M3_BATCH_PANDA_RUNTIME" in doc, setter
    doc = hdr[:hdr.index("int m3_set_point_rollout_scenes(")]
    assert "NOT batched" in doc[doc.rindex("/*"):]
    # host-only entry points: no device is needed to refuse
    lib = L.load()
    out = C.c_void_p()
    assert lib.m3_batch_flags(None) < 0
    assert lib.m3_batch_create_ex(0, 4, 2, C.byref(out)) == -1 and not out          # unknown flag bits: M3_ERR_BAD_ARG
    assert lib.m3_batch_create_ex(0, 4, 1 | 4, C.byref(out)) == -1 and not out
    assert b"unknown flag bits" in lib.m3_batch_last_error(None)
    assert lib.m3_batch_create_ex(0, 0, 1, C.byref(out)) == -1 and b"max_handles" in lib.m3_batch_last_error(None)


def test_the_thirteen_kernels_are_in_the_library_and_gain_no_scratch_over_their_twins():
    from tests.test_batch_panda_cpu import _kernels
    ks, names = _kernels()
    by = dict(zip(names, ks))

    def one(prefix):
        hit = [n for n in by if n.startswith(prefix)]
        assert len(hit) == 1, (prefix, hit)
        return by[hit[0]]

    new = 0
    for family in ("w", "v"):
        for forces in ("true", "false"):
            for lps in (1, 8, 16):
                k = one(f"void m3::kb_rollout_panda_{family}<{forces}, {lps}>(")
                twin = one(f"void m3::k_rollout_panda_{family}<{forces}, {lps}>(")
                new += 1
                assert k["private_segment_fixed_size"] <= twin["private_segment_fixed_size"], (family, forces, lps, k, twin)
                assert k["group_segment_fixed_size"] == twin["group_segment_fixed_size"]
    k, twin = one("m3::kb_panda_reach_cost_w("), one("m3::k_panda_reach_cost_w(")
    assert k["private_segment_fixed_size"] == twin["private_segment_fixed_size"] == 0
    assert new + 1 == 13
    assert not [n for n in by if "kb_rollout_panda_s<" in n]        # (a scene-only handle goes through kb_rollout_panda_w)


def test_the_new_translation_unit_is_built_under_the_panda_rollouts_flags():
    from m3p2i_aip_amd import build
    assert "rollout_panda_batch_rt.hip" in build.SOURCES
    assert build.PER_SOURCE["rollout_panda_batch_rt.hip"] == build.PER_SOURCE["rollout_panda.hip"] == ["-fno-slp-vectorize", "-O2"]


# ------------------------------------------------------------------ 3. the planner
class _Engine:
    """what command_batch sees of an engine (tests/test_panda_cost_weights_cpu.py's recording engine, + the batched path's calls)"""

    def __init__(self, scene=None):
        from m3p2i_aip_amd import _lib as L
        self.calls = []
        self._scene = {**L.PANDA_SCENE_DEFAULTS, **(scene or {})}
        self.device = types.SimpleNamespace(index=0)
        self.cfg = types.SimpleNamespace(env_type=1)

    def panda_scene(self):
        return dict(self._scene)

    def set_panda_cost_weights(self, w):
        self.calls.append(("panda", dict(w)))

    def use_torch_stream(self):
        self.calls.append(("stream",))


class _Batch:
    made = []

    def __init__(self, max_handles, device=0, panda_runtime=False):
        self.max_handles, self.device, self.panda_runtime, self.commands, self.closed = max_handles, device, panda_runtime, [], False
        _Batch.made.append(self)

    def command(self, engines):
        self.commands.append(list(engines))

    def close(self):
        self.closed = True


def _cfg(**over):
    from tests.test_panda_cost_weights_cpu import _cfg as cfg
    return cfg(**over)


@pytest.fixture()
def planners(monkeypatch):
    torch = pytest.importorskip("torch")
    from m3p2i_aip_amd import planner
    from m3p2i_aip_amd.cost_functions import Objective

    class _Planner(planner.MPPI):            # the preparation steps of a fused command, recorded instead of run
        def _ensure_noise(self): self._engine.calls.append(("noise",))
        def _push_objective(self): self._engine.calls.append(("objective",))
        def _bind_world(self): self._engine.calls.append(("bind",))
        def _next_action_slot(self): return ("slot", id(self))

    def make(objective=None, scene=None, rows=None):
        p = object.__new__(_Planner)
        p.env_type, p.K, p.K_local, p.k_offset = "panda_env", 8, 8, 0
        p._engine = _Engine()
        p._sim = types.SimpleNamespace(num_envs=8, panda_scene=None if scene is None else {**p._engine._scene, **scene},
                                       point_scene=None, point_scenes=None)
        p._bound_sim, p._objective = p._sim, objective or Objective(_cfg())
        p._fused, p.world_size, p.collective = True, 1, None
        p.tensor_args = dict(device="cpu", dtype=torch.float32)
        if rows is not None:
            p._panda_rollout_scenes = rows
        return p

    _Batch.made = []
    monkeypatch.setattr(planner, "HipEngine", _Engine)
    monkeypatch.setattr(planner, "HipBatch", _Batch)
    monkeypatch.setattr(planner, "_BATCHES", {})
    monkeypatch.setattr(planner, "_BATCHES_PANDA_RUNTIME", {})
    return planner, make, Objective


KINDS = {
    "weights": (lambda make, Objective: make(objective=Objective(_cfg(panda_cost_weights={"pick_ori": 25.0}))),
                r"command_batch: planner 1 has panda cost weights of its own \(m3_set_panda_cost_weights"),
    "workspace": (lambda make, Objective: make(scene=dict(mu=0.3)),
                  r"command_batch: planner 1 plans in a workspace of its own \(m3_set_panda_scene"),
    "rows": (lambda make, Objective: make(rows=[{}] * 8),
             r"command_batch: planner 1 has a workspace per sample \(set_panda_rollout_scenes"),
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_command_batch_reaches_a_flagged_batch_with_the_keyword_and_refuses_without(planners, kind):
    planner, make, Objective = planners
    build, message = KINDS[kind]
    good, bad = make(), build(make, Objective)
    states = [np.zeros(18, F)] * 2
    for kw in ({}, dict(panda_runtime=False)):
        with pytest.raises(ValueError, match=message):                                   # the existing message, before any call
            planner.command_batch([good, bad], states, **kw)
    assert good._engine.calls == [] and bad._engine.calls == [] and _Batch.made == []
    outs = planner.command_batch([good, bad], states, panda_runtime=True)
    assert outs == [("slot", id(good)), ("slot", id(bad))]
    assert len(_Batch.made) == 1 and _Batch.made[0].panda_runtime is True
    assert _Batch.made[0].commands == [[good._engine, bad._engine]]
    for p in (good, bad):
        assert p._engine.calls == [("stream",), ("noise",), ("objective",), ("bind",)]


def test_the_flagged_batch_is_a_second_cache_entry(planners):
    planner, make, Objective = planners
    a, b = make(), make()
    states = [np.zeros(18, F)] * 2
    planner.command_batch([a, b], states)
    planner.command_batch([a, b], states, panda_runtime=True)
    planner.command_batch([a, b], states)
    planner.command_batch([a, b], states, panda_runtime=True)
    assert [x.panda_runtime for x in _Batch.made] == [False, True]                       # one each, neither re-created
    assert [len(x.commands) for x in _Batch.made] == [2, 2] and not any(x.closed for x in _Batch.made)
    assert planner._BATCHES[0] is _Batch.made[0] and planner._BATCHES_PANDA_RUNTIME[0] is _Batch.made[1]


def test_every_other_refusal_of_command_batch_stays_with_the_keyword(planners):
    planner, make, Objective = planners
    states = [np.zeros(18, F)] * 2
    step = make()
    step._fused = False
    with pytest.raises(ValueError, match="planner 1 runs in step mode"):
        planner.command_batch([make(), step], states, panda_runtime=True)
    sharded = make()
    sharded.world_size = 2
    with pytest.raises(ValueError, match="planner 1 is sharded"):
        planner.command_batch([make(), sharded], states, panda_runtime=True)
    point = make()
    point.env_type, point._rollout_scenes = "point_env", [{}] * 8
    with pytest.raises(ValueError, match="planner 1 has an arena per sample"):            # (point_env: not part of the flag)
        planner.command_batch([make(), point], states, panda_runtime=True)
    other = make()
    other._engine = object()
    with pytest.raises(ValueError, match="planner 1 does not run on the HIP library"):
        planner.command_batch([make(), other], states, panda_runtime=True)
    twice = make()
    with pytest.raises(ValueError, match="listed twice"):
        planner.command_batch([twice, twice], states, panda_runtime=True)
    with pytest.raises(ValueError, match="one state per planner"):
        planner.command_batch([make()], states, panda_runtime=True)
    assert _Batch.made == []
