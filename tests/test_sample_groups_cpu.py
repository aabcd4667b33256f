"""Sample groups (m3_set_sample_groups) without a GPU.

1. The host header csrc/sample_groups.hpp through tests/native/sample_groups_host.cpp (its own main): validation with every
   refusal's code class and text, the table's layout, j per group, the 0-1 proof of the sorting network, the aggregate against
   a binary64 evaluation, permutation invariance -- built plain and under -fsanitize=address,undefined.
2. The committed fixture tests/golden/sample_groups_aggregate.json (costs and expected bits, printed by that program's --emit):
   the program still prints it, its --eval gives the expected bits, and the numpy binary32 emulation groups.aggregate_reference
   / aggregate_one -- the reference of the GPU tests -- gives the same bits.
3. groups.grouped_layout, groups.tile_noise, the `rollout_arena_groups` config key and its ValueErrors, the refusals of the
   batched paths for such a config.
4. The entry points' prototypes in the header and in ctypes.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from m3p2i_aip_amd import _lib as L
from m3p2i_aip_amd import compat, groups

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "sample_groups_aggregate.json")


# ------------------------------------------------------------------ 1. the host program
def _build(tmp, extra=("-O2",)):
    out = str(tmp / "sample_groups_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + list(extra) +
                          [os.path.join(HERE, "native", "sample_groups_host.cpp"), "-o", out])
    return out


def _run(prog, args=(), env=None, stdin=None):
    r = subprocess.run([prog] + list(args), capture_output=True, text=True, timeout=300, env=env, input=stdin)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return r


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("sample_groups"))


def test_the_host_program_walks_validation_table_and_aggregate(host_program):
    r = _run(host_program)
    m = re.fullmatch(r"(\d+) checks, 0 failures\n", r.stdout)
    # 65536 inputs of the 0-1 proof alone, 15 sizes x 300 draws x 3 values of j of the aggregate
    assert m and int(m.group(1)) >= 65536 + 15 * 300 * 3, r.stdout


def test_the_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    prog = _build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    err = _run(prog, env=env).stderr
    assert "AddressSanitizer" not in err and "runtime error" not in err, err[-2000:]


# ------------------------------------------------------------------ 2. the fixture
def _cases():
    return json.load(open(FIXTURE))["cases"]


def test_the_fixture_is_what_the_program_prints(host_program):
    assert json.loads(_run(host_program, ["--emit"]).stdout) == json.load(open(FIXTURE))
    cases = _cases()
    sizes = {len(c["costs"]) for c in cases}
    assert sizes == set(range(2, 17)) and len(cases) >= 15 * 4 * 3
    assert any(c["expected"] == 0x7fc00000 for c in cases) and any(c["expected"] == 0x7f800000 for c in cases)


def test_the_numpy_emulation_and_the_program_agree_bit_for_bit_on_the_fixture(host_program):
    cases = _cases()
    lines = "".join("%d %d %s\n" % (c["j"], len(c["costs"]), " ".join("%08x" % b for b in c["costs"])) for c in cases)
    native = [int(x, 16) for x in _run(host_program, ["--eval"], stdin=lines).stdout.split()]
    assert native == [c["expected"] for c in cases]
    for c in cases:
        costs = np.array(c["costs"], dtype=np.uint32).view(np.float32)
        got = int(np.float32(groups.aggregate_one(costs, c["j"])).view(np.uint32))
        assert got == c["expected"], (c, hex(got))
        # ... whatever the member order
        rev = int(np.float32(groups.aggregate_one(costs[::-1].copy(), c["j"])).view(np.uint32))
        assert rev == c["expected"], (c, hex(rev))


def test_aggregate_reference_by_groups():
    c = np.array([5.0, 1.0, 3.0, 7.0, 2.0, 9.0, 4.0], np.float32)
    g = [-1, 2, 2, -1, 6, 2, 6]
    out = groups.aggregate_reference(c, g, worst=1.0)        # group 2: {1, 3, 9}, group 6: {2, 4}
    mean3 = np.float32(np.float32(np.float32(9) + np.float32(3)) + np.float32(1)) / np.float32(3)
    assert out.tolist() == [5.0, mean3, mean3, 7.0, 3.0, mean3, 3.0] and out.dtype == np.float32
    assert groups.aggregate_reference(c, g, worst=1 / 16).tolist() == [5.0, 9.0, 9.0, 7.0, 4.0, 9.0, 4.0]
    assert groups.aggregate_reference(c, g, worst=0.5).tolist() == [5.0, 6.0, 6.0, 7.0, 4.0, 6.0, 4.0]   # j = 2 | 1
    assert [groups.worst_j(w, m) for w, m in ((1.0, 16), (1 / 16, 16), (1 / 16, 15), (0.25, 4), (0.25, 8), (0.5, 3), (1e-30, 2))] == \
        [16, 1, 1, 1, 2, 2, 1]


# ------------------------------------------------------------------ 3. layout, tiling, config key
def test_grouped_layout_single_mode():
    group_of, model_of = groups.grouped_layout(64, 4, False)
    assert group_of.shape == model_of.shape == (64,)
    ids = sorted(set(group_of[group_of >= 0].tolist()))
    assert ids == list(range(15))                                    # 15 groups, named by their first members 0 .. 14
    for g in ids:
        members = np.nonzero(group_of == g)[0].tolist()
        assert members == [g, g + 15, g + 30, g + 45]
        assert model_of[members].tolist() == [0, 1, 2, 3]
    assert np.nonzero(group_of < 0)[0].tolist() == [60, 61, 62, 63]  # 3 leftovers, K - 1 alone
    assert model_of[60:].tolist() == [-1] * 4


def test_grouped_layout_multi_modal():
    K, M = 64, 4
    group_of, model_of = groups.grouped_layout(K, M, True)
    for k in (0, K // 2, K - 1):
        assert group_of[k] == -1 and model_of[k] == -1
    # the halves: usable 1 .. 31 (31 samples, 7 groups, 3 left over) and 33 .. 62 (30 samples, 7 groups, 2 left over)
    ids = sorted(set(group_of[group_of >= 0].tolist()))
    assert ids == list(range(1, 8)) + list(range(33, 40))
    for g in ids:
        members = np.nonzero(group_of == g)[0]
        assert members.tolist() == [g + 7 * m for m in range(M)] and model_of[members].tolist() == list(range(M))
        assert (members < K // 2).all() or (members >= K // 2).all()
    assert np.nonzero(group_of < 0)[0].tolist() == [0, 29, 30, 31, 32, 61, 62, 63]
    assert (model_of[group_of < 0] == -1).all()
    for bad in (1, 17):
        with pytest.raises(ValueError, match="2 .. 16"):
            groups.grouped_layout(64, bad, False)
    with pytest.raises(ValueError, match="no room"):
        groups.grouped_layout(8, 16, False)


def test_tile_noise():
    K, T, nu = 16, 3, 2
    group_of, _ = groups.grouped_layout(K, 4, False)                 # 3 groups {g, g + 3, g + 6, g + 9}, 12 .. 15 alone
    delta = np.arange(K * T * nu, dtype=np.float32).reshape(K, T, nu)
    tiled = groups.tile_noise(delta, group_of)
    assert tiled is not delta and tiled.dtype == np.float32 and tiled.flags.c_contiguous
    for k in range(K):
        assert np.array_equal(tiled[k], delta[k % 3 if k < 12 else k]), k
    assert groups.first_members([-1, 7, 7, -1, 7]).tolist() == [0, 1, 1, 3, 1]
    import torch
    assert torch.equal(groups.tile_noise(torch.from_numpy(delta), group_of), torch.from_numpy(tiled))
    with pytest.raises(ValueError, match="16 noise rows"):
        groups.tile_noise(delta, group_of[:8])


KEY = "rollout_arena_groups={models: 4, spread: 0.3, seed: 2, fields: [box_m, mu_rb], worst: 0.25}"


def test_rollout_arena_groups_config_key():
    assert compat.make_config("config_point").rollout_arena_groups is None
    cfg = compat.make_config("config_point", ["task=push", "mppi.num_samples=64", KEY])
    assert cfg.rollout_arena_groups == dict(models=4, spread=0.3, seed=2, fields=["box_m", "mu_rb"], worst=0.25)
    assert compat.check_rollout_arena_groups(cfg) == (4, 0.3, 2, ("box_m", "mu_rb"), 0.25)
    group_of, model_of, arenas = compat.rollout_arena_group_layout(cfg)
    assert len(arenas) == 4 and all(set(a) == {"box_m", "box_I", "mu_rb"} for a in arenas)
    assert len({a["box_m"] for a in arenas}) == 4
    g2, m2 = groups.grouped_layout(64, 4, False)
    assert np.array_equal(group_of, g2) and np.array_equal(model_of, m2)
    rows = compat.rollout_point_scenes(cfg)
    assert len(rows) == 64
    for k in range(64):
        assert rows[k] == (arenas[model_of[k]] if model_of[k] >= 0 else {}), k
    assert compat.rollout_point_scenes(cfg, k_offset=32, n=32) == rows[32:]
    for bad, text in (("rollout_arena_groups={spread: 0.3}", "models: M"),
                      ("rollout_arena_groups={models: 4}", "models: M"),
                      ("rollout_arena_groups={models: 4, spread: 0.3, sed: 1}", "sed"),
                      ("rollout_arena_groups={models: 1, spread: 0.3}", "2 .. 16"),
                      ("rollout_arena_groups={models: 17, spread: 0.3}", "2 .. 16"),
                      ("rollout_arena_groups={models: 4, spread: 1.0}", "spread"),
                      ("rollout_arena_groups={models: 4, spread: 0.3, worst: 0.0}", "worst"),
                      ("rollout_arena_groups={models: 4, spread: 0.3, worst: 1.5}", "worst")):
        with pytest.raises(ValueError, match=text):
            compat.make_config("config_point", ["task=push", bad])
    with pytest.raises(ValueError, match="exclusive with rollout_arena_spread"):
        compat.make_config("config_point", ["rollout_arena_spread={spread: 0.2}", KEY])
    with pytest.raises(ValueError, match="point_env only"):
        compat.make_config("config_panda", [KEY])
    with pytest.raises(ValueError, match="noise table"):
        compat.make_config("config_point", ["mppi.sampling_method=random", KEY])


def test_the_batched_paths_refuse_the_config_key():
    from m3p2i_aip_amd import episodes
    eps = [("config_point", ["task=push"], None), ("config_point", ["task=push", "mppi.num_samples=64", KEY], None)]
    for fn in (episodes.run_point_episodes, episodes.build_set):
        for kw in ({}, dict(point_runtime=True), dict(point_priors=True)):
            with pytest.raises(ValueError, match="episode 1 .*rollout_arena_groups"):
                fn(eps, **kw)
    src = open(os.path.join(ROOT, "m3p2i_aip_amd", "planner.py")).read()
    assert re.search(r"command_batch: planner \{i\} has sample groups", src)


# ------------------------------------------------------------------ 4. symbols
def test_the_entry_points_exist_with_their_prototypes():
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    assert "#define M3_ABI_VERSION 4" in hdr
    bound = {s[0]: (s[1], list(s[2])) for s in L.SYMBOLS}
    IP = C.POINTER(C.c_int)
    assert bound["m3_set_sample_groups"] == (C.c_int, [L._H, IP, C.c_int, C.c_float])
    assert bound["m3_sample_groups_set"] == (C.c_int, [L._H])
    assert bound["m3_get_sample_group"] == (C.c_int, [L._H, C.c_int, IP, IP, IP])
    assert bound["m3_sample_group_raw_costs"] == (C.c_int, [L._H, C.POINTER(C.c_void_p)])
    assert bound["m3_aggregate_sample_groups"] == (C.c_int, [L._H])
    assert re.search(r"^int m3_set_sample_groups\(m3_handle\* h, const int\* group_of, int n, float worst_frac\);", hdr, re.M)
    assert re.search(r"^int m3_sample_groups_set\(m3_handle\* h\);", hdr, re.M)
    assert re.search(r"^int m3_get_sample_group\(const m3_handle\* h, int k, int\* group, int\* size, int\* worst_j\);", hdr, re.M)
    assert re.search(r"^int m3_sample_group_raw_costs\(m3_handle\* h, const float\*\* dev\);", hdr, re.M)
    assert re.search(r"^int m3_aggregate_sample_groups\(m3_handle\* h\);", hdr, re.M)
    assert "M3_BUF_COUNT" in hdr and not re.search(r"M3_BUF_\w*GROUP", hdr)      # (no new buffer id)
    lib = L.load()
    # (no handle can be created without a device -- the handle's answers are checked in tests/test_sample_groups_gpu.py)
    assert lib.m3_set_sample_groups(None, None, 0, 1.0) == -1 and lib.m3_sample_groups_set(None) == -1
    assert lib.m3_get_sample_group(None, 0, None, None, None) == -1
    assert lib.m3_sample_group_raw_costs(None, None) == -1 and lib.m3_aggregate_sample_groups(None) == -1
