"""m3_panda_episodes_observe / m3_panda_episodes_act allocate nothing (include/m3p2i_hip.h): the set's planning views,
status words, trace and pinned host copy come from m3_panda_episodes_create, the planners' own lazy allocations happen at
their first commands.  The process runs under the counting interposer of tests/native/alloc_count_shim.c (as
tests/test_episodes_no_alloc_gpu.py); the counter is read around the two library calls of every tick after the first
batched one -- the host's task planners in between are torch's and numpy's business, not the library's."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r"""
import ctypes, json, sys
import numpy as np
import torch
sys.path.insert(0, %(root)r)
shim = ctypes.CDLL(%(shim)r)
shim.m3shim_alloc_calls.restype = ctypes.c_long
from m3p2i_aip_amd.episodes import build_panda_set
ov = ["mppi.num_samples=200", "mppi.horizon=12"]
eps = [("config_panda", ov, dict(cube=(0.0, 0.0) if e == 0 else tuple(np.random.default_rng([77, e]).uniform(-0.02, 0.02, 2).tolist())))
       for e in range(4)]
es = build_panda_set(eps, max_ticks=150, settle_ticks=3, trace=True)
es.start()
es.tick()                                     # (the first batched command of every planner)
torch.cuda.synchronize()
calls = {"observe": 0, "act": 0}
eng = es.eps
observe, act = eng.observe, eng.act

def counted(name, fn):
    def call(*a, **k):
        before = shim.m3shim_alloc_calls()
        r = fn(*a, **k)
        calls[name] += shim.m3shim_alloc_calls() - before
        return r
    return call

eng.observe, eng.act = counted("observe", observe), counted("act", act)
n = 0
while es.active and n < 120:
    es.tick()
    n += 1
torch.cuda.synchronize()
assert shim.m3shim_alloc_calls() > 0, "the interposer saw no allocation at all: it is not in front of the HIP runtime"
out = dict(ticks=n, calls=calls)
es.close()
print("RESULT" + json.dumps(out))
"""


def test_observe_and_act_allocate_nothing_after_the_first_batched_tick(tmp_path):
    shim = str(tmp_path / "liballocshim.so")
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "alloc_count_shim.c"),
                           "-o", shim, "-ldl"])
    env = dict(os.environ, LD_PRELOAD=shim + (":" + os.environ["LD_PRELOAD"] if os.environ.get("LD_PRELOAD") else ""))
    r = subprocess.run([sys.executable, "-c", PROG % dict(root=ROOT, shim=shim)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][6:])
    assert out["ticks"] >= 50 and out["calls"] == {"observe": 0, "act": 0}, f"allocation calls inside observe / act: {out}"
