"""m3_batch_command on panda_env handles allocates nothing (include/m3p2i_hip.h): the batch's workspace -- its ring slots
sized for the larger of the point and panda table entries, and the host scratch of the panda plans -- comes from
m3_batch_create, and a handle's own lazy allocations happen on its first command.  Same interposer and procedure as
tests/test_batch_no_alloc_gpu.py: after the first batched command the counter must not move over further calls -- every kernel
form (one, eight and sixteen lanes per sample, the reach-cost kernel, the general instance, multi-modal reach), full lists,
subsets, synchronous and asynchronous."""
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

pk = dict(u_min=[-2.0] * 7 + [-1.5] * 2, u_max=[2.0] * 7 + [1.5] * 2, noise_sigma_diag=[10.0] * 7 + [0.8] * 2, lambda_=0.05,
          pre_height_diff=0.05, dt=0.01)
engs = []
for K, T, task, grip, lps, kw in [(4000, 20, "pick", 2, 0, {}), (200, 12, "reach", 1, 0, {}), (512, 20, "reach", 1, 1, {}),
                                  (512, 20, "place", 1, 8, {}), (1000, 20, "reach", 1, 0, dict(multi_modal=True)),
                                  (200, 12, "pick", 2, 0, dict(update_cov=True)),
                                  (200, 12, "pick", 2, 0, dict(sampling_random=True))] * 3:
    e = HipEngine(make_config(K=K, T=T, nu=9, env_type="panda_env", **pk, **kw))
    if not e.cfg.sampling_random:
        e.set_noise(torch.randn(K, T, 9, generator=g).numpy())
    e.set_objective(task, [0.2, 0.2, 1.115, 0, 0, 0, 1], gripper_cmd=grip)
    e.set_panda_lanes_per_sample(lps)
    engs.append(e)
batch = HipBatch(len(engs))
batch.command(engs, sync_host=True)      # (every handle's first command: its lazy allocations happen here)
torch.cuda.synchronize()
out = {}
for name, sel, sync in [("all_sync", engs, True), ("all_async", engs, False), ("subset", engs[::3], False),
                        ("reversed", engs[::-1], True), ("one", engs[4:5], False)]:
    before = shim.m3shim_alloc_calls()
    for _ in range(8):
        batch.command(sel, sync_host=sync)
    torch.cuda.synchronize()
    out[name] = shim.m3shim_alloc_calls() - before
assert shim.m3shim_alloc_calls() > 0, "the interposer saw no allocation at all: it is not in front of the HIP runtime"
print("RESULT" + json.dumps(out))
"""


def test_m3_batch_command_on_panda_handles_allocates_nothing_after_the_first_call(tmp_path):
    shim = str(tmp_path / "liballocshim.so")
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "alloc_count_shim.c"),
                           "-o", shim, "-ldl"])
    env = dict(os.environ, LD_PRELOAD=shim + (":" + os.environ["LD_PRELOAD"] if os.environ.get("LD_PRELOAD") else ""))
    r = subprocess.run([sys.executable, "-c", PROG % dict(root=ROOT, shim=shim)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][6:])
    assert all(c == 0 for c in out.values()), f"allocation calls during m3_batch_command: {out}"
