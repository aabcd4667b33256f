"""m3_batch_command allocates nothing (include/m3p2i_hip.h): all of the batch's device and pinned workspace comes from
m3_batch_create, and a handle's own lazy allocations happen on its first command.  The process runs under the counting
interposer of tests/native/alloc_count_shim.c (as tests/test_no_alloc_in_command_gpu.py does for m3_command); after the
first batched command the counter must not move over further calls -- full lists, subsets, synchronous and asynchronous."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r"""
import ctypes, json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
shim = ctypes.CDLL(%(shim)r)
shim.m3shim_alloc_calls.restype = ctypes.c_long
from m3p2i_aip_amd.engine import HipBatch, HipEngine, make_config
g = torch.Generator().manual_seed(5)

def noise(K, T):
    knots = torch.randn(K, 2, max(T // 4, 2), generator=g)
    return torch.nn.functional.interpolate(knots, size=T, mode="linear", align_corners=True).permute(0, 2, 1).contiguous().numpy()

pk = dict(u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3])
engs = []
for K, T, task, goal, kw in [(2000, 30, "push", (-1.0, -1.0), {}), (200, 15, "navigation", (2.0, -2.0), {}),
                             (4000, 30, "push_pull", (-3.75, -3.75), dict(multi_modal=True)),
                             (2000, 30, "pull", (0.0, 0.0), dict(update_cov=True)),
                             (2000, 30, "push", (-1.0, -1.0), dict(sampling_random=True))] * 4:
    e = HipEngine(make_config(K=K, T=T, nu=2, **pk, **kw))
    if not e.cfg.sampling_random:
        e.set_noise(noise(K, T))
    e.set_objective(task, goal)
    engs.append(e)
batch = HipBatch(len(engs))
batch.command(engs, sync_host=True)      # (every handle's first command: its lazy allocations happen here)
torch.cuda.synchronize()
out = {}
for name, sel, sync in [("all_sync", engs, True), ("all_async", engs, False), ("subset", engs[::3], False),
                        ("reversed", engs[::-1], True), ("one", engs[2:3], False)]:
    before = shim.m3shim_alloc_calls()
    for _ in range(8):
        batch.command(sel, sync_host=sync)
    torch.cuda.synchronize()
    out[name] = shim.m3shim_alloc_calls() - before
assert shim.m3shim_alloc_calls() > 0, "the interposer saw no allocation at all: it is not in front of the HIP runtime"
print("RESULT" + json.dumps(out))
"""


def test_m3_batch_command_allocates_nothing_after_the_first_call(tmp_path):
    shim = str(tmp_path / "liballocshim.so")
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "alloc_count_shim.c"),
                           "-o", shim, "-ldl"])
    env = dict(os.environ, LD_PRELOAD=shim + (":" + os.environ["LD_PRELOAD"] if os.environ.get("LD_PRELOAD") else ""))
    r = subprocess.run([sys.executable, "-c", PROG % dict(root=ROOT, shim=shim)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][6:])
    assert all(c == 0 for c in out.values()), f"allocation calls during m3_batch_command: {out}"
