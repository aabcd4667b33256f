"""Build libm3p2i_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python -m m3p2i_aip_amd.build [--force]

-ffp-contract=off / no fast-math: the dynamics are specified as a fixed sequence of IEEE
binary32 operations so that the CPU oracle can check them bit-for-bit.  Every source is its own
translation unit (no relocatable device code): they are compiled in parallel and linked into one .so.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "lib", "libm3p2i_hip.so")
OBJ = os.path.join(HERE, "_obj")   # object files (git- and gpurun-ignored)
SOURCES = ["rollout_point.hip", "rollout_point_task0.hip", "rollout_point_task1.hip", "rollout_point_task2.hip",
           "rollout_point_task3.hip", "rollout_point_scene.hip", "rollout_point_scene_rows.hip",
           "rollout_point_rollout_scenes.hip", "rollout_point_priors.hip", "rollout_point_priors_batch.hip", "prior_controllers.hip",
           "rollout_panda.hip", "rollout_panda_scene.hip", "rollout_panda_weights.hip", "rollout_panda_rows.hip",
           "rollout_panda_priors.hip", "rollout_panda_batch_rt.hip", "rollout_panda_episodes_rt.hip",
           "update.hip", "update_small.hip", "update_sharded.hip", "sampler.hip", "p2p.hip", "sample_groups.hip", "m3_api.hip"]
CFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall",
          "-Wno-unused-function"]
# per-source flags, measured on the bench configs (tools/time_variants_cfg.sh; later flags win; none of them changes
# floating-point semantics): the point rollout kernels are ~2 % faster at -O2 than at -O3, the panda rollout
# faster without the SLP vectoriser (the point kernels ~2 % slower without it -- measured again with the predicated rows of the
# lean substep instances, profiles/lean_rows: +2.4 % without it) and at -O2
PER_SOURCE = {
    "rollout_point.hip": ["-O2"], "rollout_point_task0.hip": ["-O2"], "rollout_point_task1.hip": ["-O2"],
    "rollout_point_task2.hip": ["-O2"], "rollout_point_task3.hip": ["-O2"], "rollout_point_scene.hip": ["-O2"],
    "rollout_point_scene_rows.hip": ["-O2"], "rollout_point_rollout_scenes.hip": ["-O2"],
    "rollout_point_priors.hip": ["-O2"], "rollout_point_priors_batch.hip": ["-O2"],   # (its twin's: the same bodies)
    "rollout_panda.hip": ["-fno-slp-vectorize", "-O2"],   # (round 4, world spec v2: -O2 -1.5 % reach / -4.5 % pick; with SLP +18 % / +11 %)
    "rollout_panda_scene.hip": ["-fno-slp-vectorize", "-O2"],   # (rollout_panda.hip's: the same bodies)
    "rollout_panda_weights.hip": ["-fno-slp-vectorize", "-O2"],   # (likewise)
    "rollout_panda_rows.hip": ["-fno-slp-vectorize", "-O2"],   # (likewise)
    "rollout_panda_priors.hip": ["-fno-slp-vectorize", "-O2"],   # (likewise)
    "rollout_panda_batch_rt.hip": ["-fno-slp-vectorize", "-O2"],   # (likewise)
    "rollout_panda_episodes_rt.hip": ["-fno-slp-vectorize", "-O2"],   # (likewise: k_panda_episodes_pre / _post live in rollout_panda.hip)
}


def source_hash(extra_flags=()):
    """Identity of a build that survives a rebuild: sha256 over the kernel sources, the public headers and every compiler flag
    (the .so's own bytes differ from one link to the next).  Compiled into the library (m3_build_id) -- the key of the committed
    PMC profiles that bench.py's roofline_valu reads."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(os.listdir(CSRC)) + [os.path.join("..", "..", "include", h) for h in ("m3p2i_hip.h", "m3p2i_hip_ext.h")]
    for f in files:
        path = os.path.join(CSRC, f)
        if os.path.isfile(path):
            h.update(f.encode()); h.update(open(path, "rb").read())
    h.update(repr((CFLAGS, sorted(PER_SOURCE.items()), list(extra_flags))).encode())
    return h.hexdigest()[:16]


def _stale():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    deps += [os.path.join(os.path.dirname(HERE), "include", h) for h in ("m3p2i_hip.h", "m3p2i_hip_ext.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False, extra_flags=(), out=OUT):
    if not force and out == OUT and not _stale():
        return OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    build_id = source_hash(extra_flags)
    objdir = OBJ if out == OUT else os.path.join(OBJ, os.path.basename(out) + ".d")
    os.makedirs(objdir, exist_ok=True)

    def compile_one(src):
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        ident = ['-DM3_BUILD_ID="%s"' % build_id] if src == "m3_api.hip" else []
        cmd = [hipcc] + CFLAGS + PER_SOURCE.get(src, []) + list(extra_flags) + ident + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        return obj

    with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 4)) as pool:
        objs = list(pool.map(compile_one, SOURCES))
    link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", out]
    if verbose:
        print(" ".join(link), flush=True)
    subprocess.check_call(link)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
