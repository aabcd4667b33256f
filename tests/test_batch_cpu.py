"""The batched command's C-ABI without a GPU: declared, exported and bound; creation fails loudly; null arguments are
refused.  And the residency bound of the batched multi-modal update (update_small.hip:
update_small_batch_blocks_per_cu) re-derived from the built library's code objects."""
import ctypes as C
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["m3_batch_create", "m3_batch_destroy", "m3_batch_last_error", "m3_batch_command", "m3_batch_launches"]


def test_batch_symbols_declared_exported_and_bound():
    from m3p2i_aip_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    bound = {name for name, _, _ in L.SYMBOLS}
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in bound, name
        assert getattr(lib, name)   # exported
    assert "typedef struct m3_batch m3_batch;" in hdr


def test_batch_create_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipBatch
    lib = L.load()
    b = C.c_void_p()
    rc = lib.m3_batch_create(0, 8, C.byref(b))
    assert rc != 0 and not b.value
    assert lib.m3_batch_last_error(None)
    with pytest.raises(L.M3Error):
        HipBatch(8)


def test_batch_null_arguments_are_refused():
    from m3p2i_aip_amd import _lib as L
    lib = L.load()
    assert lib.m3_batch_command(None, None, 1, None) < 0
    assert b"null batch" in lib.m3_batch_last_error(None)
    lib.m3_batch_destroy(None)                 # a no-op
    assert isinstance(lib.m3_batch_last_error(None), bytes)
    assert lib.m3_batch_launches(None, None, None) < 0
    assert lib.m3_batch_create(0, 8, None) < 0
    b = C.c_void_p()
    assert lib.m3_batch_create(0, 0, C.byref(b)) < 0 and not b.value


# blocks per CU that update_small_batch_blocks_per_cu returns, per kb_update_small<MULTI = true, JR, WT> instance
BLOCKS_PER_CU = {(8, 256): 4, (16, 256): 4, (32, 256): 2, (8, 512): 1, (16, 512): 1}


def _blocks_per_cu(k, wt):
    """resident workgroups per CU from the code object: waves per SIMD bounded by VGPRs (arch + acc, granules of 8, 512 per
    lane), SGPRs (granules of 16, + 16, 800 per SIMD) and 8; divided by the workgroup's waves per SIMD; LDS (160 KiB per CU);
    at most 4 workgroups of 256 threads (2 of 512)"""
    v = -(-k["vgpr_count"] // 8) * 8
    s = -(-k["sgpr_count"] // 16) * 16 + 16
    waves = min(8, 512 // v, 800 // s)
    by_lds = 163840 // (k["group_segment_fixed_size"] + 256 * 2 * 4)     # (+ the plan: T <= 256, nu = 2)
    return min(waves // (wt // 256), by_lds, 4 if wt == 256 else 2)


def test_batched_update_residency_bound_matches_the_code_object():
    from m3p2i_aip_amd import _lib as L
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_info
    tmp, cos = codeobj_info.extract(L.LIB_PATH)
    try:
        ks = [k for co in cos for k in codeobj_info.kernels(co)]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    names = dict(zip([k["name"] for k in ks], codeobj_info.demangle([k["name"] for k in ks])))
    seen = set()
    for k in ks:
        m = re.search(r"kb_update_small<true, (\d+), (\d+)>", names[k["name"]])
        if not m:
            continue
        jr, wt = int(m.group(1)), int(m.group(2))
        seen.add((jr, wt))
        assert _blocks_per_cu(k, wt) == BLOCKS_PER_CU[(jr, wt)], (names[k["name"]], k)
    assert seen == set(BLOCKS_PER_CU)
    src = open(os.path.join(ROOT, "m3p2i_aip_amd", "csrc", "update_small.hip")).read()
    body = src[src.index("int update_small_batch_blocks_per_cu"):]
    body = body[:body.index("\n}\n")]
    assert re.findall(r"return (\d+);", body) == [str(BLOCKS_PER_CU[(8, 512)]), str(BLOCKS_PER_CU[(32, 256)]),
                                                  str(BLOCKS_PER_CU[(8, 256)])]
    assert BLOCKS_PER_CU[(8, 512)] == BLOCKS_PER_CU[(16, 512)] and BLOCKS_PER_CU[(8, 256)] == BLOCKS_PER_CU[(16, 256)]
