"""No HIP allocation in m3_set_point_scene, nor in the commands, the batched command and the step of a warmed-up handle with a
custom arena: the LD_PRELOAD counter of tests/test_no_alloc_in_command_gpu.py (tests/native/alloc_count_shim.c) around them, in
the pattern of tests/test_cost_weights_no_alloc_gpu.py."""
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

A = dict(obs_x=-1.0, obs_y=0.5, obs_hx=0.25, obs_hy=0.1, wall=1.5, box_hx=0.3, box_hy=0.15, box_m=9.0, mu_rb=0.4, robot_r=0.25)
pk = dict(u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3])
out = {}
host = np.zeros((30, 2), np.float32)
for name, mm, task in (("push", False, "push"), ("push_pull", True, "push_pull")):
    K = 512 if mm else 256
    e = HipEngine(make_config(K=K, T=30, nu=2, multi_modal=mm, **pk)); e.set_noise(noise(K, 30, 2))
    e.set_objective(task, (1.0, 1.0))
    e.command(sync_host=True)                 # the handle's first command, in the default arena
    torch.cuda.synchronize()
    before = shim.m3shim_alloc_calls()
    e.set_point_scene(A)
    set_calls = shim.m3shim_alloc_calls() - before
    e.lib.m3_command(e._h, host.ctypes.data)  # the first command in the custom arena (loads no new code object: one library)
    torch.cuda.synchronize()
    before = shim.m3shim_alloc_calls()
    for i in range(6):
        e.set_point_scene(A, obs_x=-1.0 + 0.05 * i)
        e.lib.m3_command(e._h, host.ctypes.data)
    torch.cuda.synchronize()
    out[name] = [set_calls, shim.m3shim_alloc_calls() - before]
    e.close()
# batched command: two arenas and a default handle in one call
engs = []
for i in range(3):
    e = HipEngine(make_config(K=256, T=30, nu=2, **pk)); e.set_noise(noise(256, 30, 2)); e.set_objective("push", (1.0, 1.0))
    if i:
        e.set_point_scene(A, wall=1.5 + 0.5 * i)
    engs.append(e)
batch = HipBatch(3)
batch.command(engs); batch.command(engs)
torch.cuda.synchronize()
before = shim.m3shim_alloc_calls()
for i in range(4):
    engs[1].set_point_scene(A, mu_rb=0.3 + 0.05 * i)
    batch.command(engs)
torch.cuda.synchronize()
out["batch"] = [0, shim.m3shim_alloc_calls() - before]
batch.close()
for e in engs:
    e.close()
# step mode: a sim_only handle with bound views
n = 64
s = HipEngine(make_config(K=n, K_local=n, T=1, nu=2, sim_only=True, filter_u=False))
dof = torch.zeros(n, 4, device="cuda:0"); root = torch.zeros(n, 11, 13, device="cuda:0"); root[..., 6] = 1.0
root[:, 6, 0:2] = torch.tensor([0.45, 0.0]); root[:, 5, 0:2] = torch.tensor([1.0, 1.0])
rb = torch.zeros(n, 13, 13, device="cuda:0"); ncf = torch.zeros(n, 13, 3, device="cuda:0")
s.sim_bind_views(dof, root, rb, ncf); s.sim_pull_state()
u = torch.ones(n, 2, device="cuda:0")
s.set_point_scene(A)
s._ck(s.lib.m3_sim_step_with_target(s._h, u.data_ptr()))
torch.cuda.synchronize()
before = shim.m3shim_alloc_calls()
for i in range(4):
    s.set_point_scene(A, mu_rb=0.3 + 0.05 * i)
    s._ck(s.lib.m3_sim_step_with_target(s._h, u.data_ptr()))
torch.cuda.synchronize()
out["step"] = [0, shim.m3shim_alloc_calls() - before]
assert float(dof[:, 0].abs().max()) > 0.0, "the step did not move the robot"
s.close()
assert shim.m3shim_alloc_calls() > 0, "the interposer saw no allocation at all: it is not in front of the HIP runtime"
print("RESULT" + json.dumps(out))
"""


def test_set_point_scene_commands_batch_and_step_allocate_nothing(tmp_path):
    shim = str(tmp_path / "liballocshim.so")
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "alloc_count_shim.c"),
                           "-o", shim, "-ldl"])
    env = dict(os.environ, LD_PRELOAD=shim + (":" + os.environ["LD_PRELOAD"] if os.environ.get("LD_PRELOAD") else ""))
    r = subprocess.run([sys.executable, "-c", PROG % dict(root=ROOT, shim=shim)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][6:])
    assert set(out) == {"push", "push_pull", "batch", "step"}
    for name, (in_set, in_calls) in out.items():
        assert in_set == 0, f"{name}: m3_set_point_scene made {in_set} allocation calls"
        assert in_calls == 0, f"{name}: {in_calls} allocation calls in set + command / batched command / step after the first"
