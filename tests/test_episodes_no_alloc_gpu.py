"""m3_episodes_tick allocates nothing (include/m3p2i_hip.h): all of the set's memory comes from m3_episodes_create, and the
planners' own lazy allocations happen at their first commands.  The process runs under the counting interposer of
tests/native/alloc_count_shim.c (as tests/test_batch_no_alloc_gpu.py); after the first batched tick the counter must not
move."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r"""
import ctypes, json, sys
import torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tools)r)
shim = ctypes.CDLL(%(shim)r)
shim.m3shim_alloc_calls.restype = ctypes.c_long
import band_stats as bs
from m3p2i_aip_amd.episodes import build_set
eps = [("config_point", bs.overrides(sc, size), bs.jitter_of(sc, e))
       for sc, size, e in [("case2_halton_push_coll", "default", 1), ("case2_halton_pull_coll", "default", 2),
                           ("corner1_hybrid", "default", 3), ("corner2_push", "baseline", 1), ("corner1_push", "default", 0)]]
es = build_set(eps, max_ticks=120)
es.start()
es.tick()                                     # (the first batched command of every planner)
torch.cuda.synchronize()
before = shim.m3shim_alloc_calls()
n = 0
while es.running and n < 100:
    es.tick()
    n += 1
torch.cuda.synchronize()
out = dict(ticks=n, calls=shim.m3shim_alloc_calls() - before)
assert shim.m3shim_alloc_calls() > 0, "the interposer saw no allocation at all: it is not in front of the HIP runtime"
es.close()
print("RESULT" + json.dumps(out))
"""


def test_m3_episodes_tick_allocates_nothing_after_the_first_tick(tmp_path):
    shim = str(tmp_path / "liballocshim.so")
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "alloc_count_shim.c"),
                           "-o", shim, "-ldl"])
    env = dict(os.environ, LD_PRELOAD=shim + (":" + os.environ["LD_PRELOAD"] if os.environ.get("LD_PRELOAD") else ""))
    r = subprocess.run([sys.executable, "-c", PROG % dict(root=ROOT, tools=os.path.join(ROOT, "tools"), shim=shim)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][6:])
    assert out["ticks"] >= 50 and out["calls"] == 0, f"allocation calls during m3_episodes_tick: {out}"
