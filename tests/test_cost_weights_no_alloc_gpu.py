"""No HIP allocation in a weighted m3_command after the first, nor in m3_set_point_cost_weights: the LD_PRELOAD counter of
tests/test_no_alloc_in_command_gpu.py (tests/native/alloc_count_shim.c) around both."""
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

def noise(K, T, nu):
    knots = torch.randn(K, nu, max(T // 4, 2), generator=g)
    return torch.nn.functional.interpolate(knots, size=T, mode="linear", align_corners=True).permute(0, 2, 1).contiguous().numpy()

pk = dict(u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3])
out = {}
host = np.zeros((30, 2), np.float32)
for name, mm, task in (("push", False, "push"), ("push_pull", True, "push_pull")):
    K = 4000 if mm else 2000
    e = HipEngine(make_config(K=K, T=30, nu=2, multi_modal=mm, **pk)); e.set_noise(noise(K, 30, 2))
    e.set_objective(task, (-1.0, -1.0))
    e.command(sync_host=True)                 # the handle's first command, unweighted
    torch.cuda.synchronize()
    before = shim.m3shim_alloc_calls()
    e.set_point_cost_weights(dict(push_align=2.5, pull_vel=0.0))
    set_calls = shim.m3shim_alloc_calls() - before
    e.lib.m3_command(e._h, host.ctypes.data)  # the first weighted command (loads no new code object: one library)
    torch.cuda.synchronize()
    before = shim.m3shim_alloc_calls()
    for i in range(6):
        e.set_point_cost_weights(dict(push_align=2.5 + i))
        e.lib.m3_command(e._h, host.ctypes.data)
    torch.cuda.synchronize()
    out[name] = [set_calls, shim.m3shim_alloc_calls() - before]
    e.close()
assert shim.m3shim_alloc_calls() > 0, "the interposer saw no allocation at all: it is not in front of the HIP runtime"
print("RESULT" + json.dumps(out))
"""


def test_weighted_command_and_set_weights_allocate_nothing(tmp_path):
    shim = str(tmp_path / "liballocshim.so")
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "alloc_count_shim.c"),
                           "-o", shim, "-ldl"])
    env = dict(os.environ, LD_PRELOAD=shim + (":" + os.environ["LD_PRELOAD"] if os.environ.get("LD_PRELOAD") else ""))
    r = subprocess.run([sys.executable, "-c", PROG % dict(root=ROOT, shim=shim)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][6:])
    for name, (in_set, in_commands) in out.items():
        assert in_set == 0, f"{name}: m3_set_point_cost_weights made {in_set} allocation calls"
        assert in_commands == 0, f"{name}: {in_commands} allocation calls in weighted m3_commands after the first"
