"""One ledger owns each C object's memory (m3p2i_aip_amd/csrc/owned_blocks.hpp), without a GPU.

1. The sources: in m3p2i_aip_amd/csrc/ the calls that free occur only inside m3_release_block (the ledger's release function
   bound to HIP), the calls that allocate only inside the per-kind helpers own_*; m3_destroy and its three siblings hold no
   per-member lines.  A buffer added the old way fails here.
2. The ledger stand-alone (tests/native/owned_blocks_check.cpp, its own main, bound to malloc / free with a recording release
   function), built plain and with -fsanitize=address,undefined and run directly.
3. Plumbing: the diagnostic m3_owned_blocks_live is declared in the header and bound.
"""
import os
import re
import subprocess

import pytest

from m3p2i_aip_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "m3p2i_aip_amd", "csrc")
NATIVE = os.path.join(HERE, "native")

FREES = ["hipFree", "hipHostFree", "hipEventDestroy", "hipIpcCloseMemHandle", "std::free", "free", "hipFreeAsync"]
ALLOCS = ["hipMalloc", "hipHostMalloc", "hipExtMallocWithFlags", "hipEventCreate", "hipEventCreateWithFlags", "hipIpcOpenMemHandle",
          "std::malloc", "malloc", "calloc", "realloc", "hipMallocAsync", "hipMallocManaged", "hipHostAlloc"]
LEDGER = "owned_blocks.hpp"   # (host only: its own table through std::realloc / std::free, no HIP call -- checked below)


def code_only(text):
    """the text without comments and string literals (lengths of lines are not kept, braces inside them are gone)"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    return re.sub(r"//[^\n]*", " ", text)


def calls(name, text):
    return len(re.findall(r"(?<![\w:.>])" + re.escape(name) + r"\s*\(", text))


def function_bodies(text, pattern):
    """{name: body} of the function definitions whose name matches `pattern`, and the text with those bodies cut out"""
    out, rest, pos = {}, [], 0
    # (a definition: at the left margin, nothing but the return type in front of the name -- a call has a parenthesis there)
    for m in re.finditer(r"^\S[^\n(]*\b(%s)\s*\([^;{}]*\)\s*\{" % pattern, text, re.M):
        if m.start() < pos:
            continue
        depth, i = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(text[i], 0)
            i += 1
        assert m.group(1) not in out, m.group(1)
        out[m.group(1)] = text[m.end():i - 1]
        rest.append(text[pos:m.end()])
        pos = i - 1
    rest.append(text[pos:])
    return out, "".join(rest)


@pytest.fixture(scope="module")
def sources():
    return {f: code_only(open(os.path.join(CSRC, f)).read()) for f in sorted(os.listdir(CSRC))
            if f.endswith((".hip", ".hpp", ".inc", ".h"))}


def test_frees_only_in_the_release_function_and_allocations_only_in_the_helpers(sources):
    api = sources["m3_api.hip"]
    owners, rest = function_bodies(api, r"m3_release_block|own_\w+")
    assert sorted(owners) == ["m3_release_block", "own_device", "own_event", "own_hip", "own_host", "own_ipc", "own_pinned"]
    # the binding releases each kind with its call, once
    rel = owners["m3_release_block"]
    assert [calls(n, rel) for n in ("hipFree", "hipHostFree", "std::free", "hipEventDestroy", "hipIpcCloseMemHandle")] == [1] * 5
    assert not any(calls(n, rel) for n in ALLOCS)
    # the helpers allocate and never free
    for name, body in owners.items():
        if name != "m3_release_block":
            assert not any(calls(n, body) for n in FREES), name
    assert not any(calls(n, owners["own_hip"]) for n in ALLOCS)
    assert calls("hipMalloc", owners["own_device"]) == 1 and calls("hipExtMallocWithFlags", owners["own_device"]) == 1
    assert calls("hipHostMalloc", owners["own_pinned"]) == 1 and calls("std::malloc", owners["own_host"]) == 1
    assert calls("hipEventCreate", owners["own_event"]) == 1 and calls("hipEventCreateWithFlags", owners["own_event"]) == 1
    assert calls("hipIpcOpenMemHandle", owners["own_ipc"]) == 1
    # nothing of either kind anywhere else in csrc/
    everywhere_else = dict(sources, **{"m3_api.hip": rest})
    for f, text in everywhere_else.items():
        names = [n for n in FREES + ALLOCS if calls(n, text)]
        if f == LEDGER:   # its own table of entries: grown through std::realloc, freed once, by the destructor
            assert names == ["std::free"] and calls("std::free", text) == 1 and "std::free(e_)" in text and "hip" not in text.lower()
            continue
        assert names == [], (f, names)
    # ... and every allocation goes into a ledger: each helper ends in own_block
    assert calls("own_block", owners["own_hip"]) == 1
    for name in ("own_device", "own_pinned", "own_host", "own_event", "own_ipc"):
        assert calls("own_hip", owners[name]) == 1, name


def test_the_destroy_functions_have_no_per_member_lines(sources):
    bodies, _ = function_bodies(sources["m3_api.hip"], r"m3_destroy|m3_batch_destroy|m3_episodes_destroy|m3_panda_episodes_destroy")
    assert len(bodies) == 4
    for name, body in bodies.items():
        stmts = [s.strip() for s in body.split(";") if s.strip()]
        assert stmts[0].startswith("if (!") and stmts[0].endswith("return"), (name, stmts)
        assert stmts[-2:] == [stmts[-2], "delete " + stmts[-2].split("->")[0]] and stmts[-2].endswith("->mem.release_all()"), (name, stmts)
        # in between: only what the function synchronises (a stream or the slots' events), nothing per member
        middle = stmts[1:-2]
        assert len(middle) <= 3 and (not middle or "Synchronize(" in middle[-1]), (name, middle)
        assert body.count("->mem.release_all()") == 1 and body.count("delete ") == 1
    assert "Synchronize" not in bodies["m3_destroy"]      # as before: m3_destroy synchronises nothing
    assert "hipEventSynchronize" in bodies["m3_batch_destroy"]
    assert "hipStreamSynchronize" in bodies["m3_episodes_destroy"] and "hipStreamSynchronize" in bodies["m3_panda_episodes_destroy"]


def test_the_lazy_groups_allocate_under_one_guard(sources):
    bodies, _ = function_bodies(sources["m3_api.hip"], r"ensure_sim|refresh_wave_order|upload_scene_rows|m3_enable_timing")
    for name, n_blocks in (("ensure_sim", 2), ("refresh_wave_order", 3), ("upload_scene_rows", 3), ("m3_enable_timing", 1)):
        body = bodies[name]
        g = body.index("BlockGroup g(h->mem)")
        keep = body.index("g.keep = true")
        owned = [m.start() for m in re.finditer(r"\bown_\w+\(h->mem,", body)]
        assert len(owned) == n_blocks and all(g < i < keep for i in owned), name


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_ledger_stand_alone_program(tmp_path, san):
    exe = str(tmp_path / "owned_blocks_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I" + CSRC, os.path.join(NATIVE, "owned_blocks_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)     # (run directly: nothing sanitized is loaded into python)
    assert r.returncode == 0 and "owned_blocks_check: ok" in r.stdout, r.stdout + r.stderr


def test_the_ledger_header_is_host_only():
    text = open(os.path.join(CSRC, LEDGER)).read()
    assert not re.search(r"#include\s*[<\"]hip", text) and "m3_internal" not in text
    assert 60 <= len(text.splitlines()) <= 130


def test_the_diagnostic_is_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    assert re.search(r"/\* Diagnostic(?:(?!\*/).)*\*/\s*long long m3_owned_blocks_live\(void\);", text, re.S)
    assert text.index("m3_point_rollout_plan(int task") < text.index("m3_owned_blocks_live(void)") < text.index("int m3_set_multi_modal(")
    assert ("m3_owned_blocks_live", L.C.c_longlong, []) in L.SYMBOLS
    assert "#define M3_ABI_VERSION 4" in text
