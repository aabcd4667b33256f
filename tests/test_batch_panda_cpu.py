"""The panda_env half of the batched command without a GPU: the batched kernels are in the built library, and the residency
bound of the batched nu = 9 multi-modal update (update_small.hip: update_small9_batch_blocks_per_cu) is re-derived from the
built library's code objects, as tests/test_batch_cpu.py does for the nu = 2 instances."""
import os
import re
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# blocks per CU that update_small9_batch_blocks_per_cu returns, per kb_update_small9<MULTI = true, JR> instance
BLOCKS_PER_CU = {8: 4, 16: 2}
PLAN_BYTES = 2048 * 4       # the plan staged in dynamic LDS: T * nu <= 2048 floats (the one-launch update's bound)


def _kernels():
    from m3p2i_aip_amd import _lib as L
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_info
    tmp, cos = codeobj_info.extract(L.LIB_PATH)
    try:
        ks = [k for co in cos for k in codeobj_info.kernels(co)]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return ks, codeobj_info.demangle([k["name"] for k in ks])


def _blocks_per_cu(k):
    """resident 256-thread workgroups per CU from the code object: waves per SIMD bounded by VGPRs (arch + acc, granules of 8,
    512 per lane), SGPRs (granules of 16, + 16, 800 per SIMD) and 8; LDS (160 KiB per CU, static + the plan); at most 4"""
    v = -(-k["vgpr_count"] // 8) * 8
    s = -(-k["sgpr_count"] // 16) * 16 + 16
    waves = min(8, 512 // v, 800 // s)
    by_lds = 163840 // (k["group_segment_fixed_size"] + PLAN_BYTES)
    return min(waves, by_lds, 4)


def test_batched_panda_kernels_are_in_the_library():
    ks, names = _kernels()
    have = set(names)
    for forces in ("true", "false"):
        for general in ("true", "false"):
            for lps in (1, 8, 16):
                assert any(n.startswith(f"void m3::kb_rollout_panda<{forces}, {general}, {lps}>(") for n in have), (forces, general, lps)
    assert any(n.startswith("m3::kb_panda_reach_cost(") for n in have)
    for multi in ("true", "false"):
        for jr in (8, 16):
            assert any(n.startswith(f"void m3::kb_update_small9<{multi}, {jr}>(") for n in have), (multi, jr)
    # the batched forms read their arguments from the table: no scratch beyond what the single-handle kernel has
    by = dict(zip(names, ks))
    for n, k in by.items():
        m = re.match(r"void m3::kb_rollout_panda<(\w+), (\w+), (\d+)>\(", n)
        if m:
            twin = [x for x in by if x.startswith(f"void m3::k_rollout_panda<{m.group(1)}, {m.group(2)}, {m.group(3)}>(")]
            assert len(twin) == 1, n
            assert k["private_segment_fixed_size"] <= by[twin[0]]["private_segment_fixed_size"], (n, k, by[twin[0]])


def test_batched_nu9_update_residency_bound_matches_the_code_object():
    ks, names = _kernels()
    seen = set()
    for k, n in zip(ks, names):
        m = re.search(r"kb_update_small9<true, (\d+)>", n)
        if not m:
            continue
        jr = int(m.group(1))
        seen.add(jr)
        assert _blocks_per_cu(k) == BLOCKS_PER_CU[jr], (n, k)
    assert seen == set(BLOCKS_PER_CU)
    src = open(os.path.join(ROOT, "m3p2i_aip_amd", "csrc", "update_small.hip")).read()
    body = src[src.index("int update_small9_batch_blocks_per_cu"):]
    body = body[:body.index("\n}\n")]
    assert re.findall(r"return (\d+);", body) == [str(BLOCKS_PER_CU[16]), str(BLOCKS_PER_CU[8])]
