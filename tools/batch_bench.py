"""Batched command (m3_batch_command) vs the best a caller can do without it: n independent planners, each with its own
jittered world (point_env: tools/band_stats.py's jitter_of; panda_env: cubeA's start displaced by up to 2 cm as
band_stats.panda_episodes does, then the product's own closed loop, tools/closed_loop.py, run into the scene measured),
commanded
  batched        ONE m3_batch_command per iteration (one rollout + one update launch per group; multi-modal groups in
                 residency chunks)
  back_to_back   n m3_command calls per iteration on the same stream, no host synchronisation in between
Both are timed with HIP events around `--iters` iterations after `--warmup` (ms per iteration, median of `--repeats`).
Each configuration runs in a child process of its own under a time limit; the parent prints ONE JSON line.

    python tools/batch_bench.py [--only c2_push] [--json out.json] [--iters 50] [--warmup 10] [--repeats 5]

The `*_rt` configurations (panda_env, a batch created with M3_BATCH_PANDA_RUNTIME; not part of the default list, name them with
--only) measure, per n and in one process on the same worlds, three kinds of handles: `literal` (the default workspace and
weights: kb_rollout_panda), `weighted` (tuned weights on the default workspace: kb_rollout_panda_w) and `per_sample` (a spread
of 0.3 over the workspaces as tools/panda_rollout_scenes_bench.py: kb_rollout_panda_v) -- each batched and back to back, with
the ratios of the non-literal kinds' batched time to the literal one's.  Two controls do the literal handles' work, bit for
bit, on the other kernels: `weighted_same_work` (the weighted instance forced at the default weights) and
`per_sample_same_work` (K rows of the default workspace) -- what the kernels cost, apart from what the tuned handles meet.

The `*_sv` configurations (point_env, a batch created with M3_BATCH_SECTION_POINT_ROLLOUT_SCENES; not part of the default list
either) measure n planners with an arena per sample: `per_sample` (scenes.spread_point_scenes rows, spread 0.3, a seed per
planner: kb_rollout_point_sv*), batched against n back-to-back m3_command calls of the same handles, beside `scene` (the
single-arena run-time-scene group of the same n, K, T: the run-time-scene instance forced on at the default arena) and the
control `per_sample_same_work` (K rows of the default arena: the `scene` handles' work bit for bit, plus the 38 row loads per
lane).

The `*_pr` configurations (point_env, a batch created with M3_BATCH_SECTION_POINT_PRIORS and _POINT_ROLLOUT_SCENES; not part of
the default list either; n = 1, 4, 16, 64) measure n planners with prior samples: `priors` (a push_behind controller on the
device, four sequences per planner: kb_prior_controllers + kb_rollout_point_pr*), batched against n back-to-back m3_command calls
of the same handles -- the only path such handles had --, beside `per_sample_same_work` (K rows of the default arena, no priors:
the kernels the prior build twins) of the same run.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

# name -> (scenario of band_stats whose jitter the worlds take, task, goal, K, T, multi_modal, the n to measure)
CONFIGS = {
    "c2_push": ("corner1_push", "push", (-3.75, -3.75), 2000, 30, False, (1, 4, 16, 64)),
    "shipped_push": ("case2_halton_push_coll", "push", (-3.0, 3.0), 200, 15, False, (1, 16, 64)),
    "c3_push_pull": ("corner1_hybrid", "push_pull", (-3.75, -3.75), 4000, 30, True, (1, 4, 16)),
}
# panda_env: name -> (task, the closed-loop phase the scene is taken from + ticks into it, K, T, the n to measure)
PANDA_CONFIGS = {
    "c4_reach": ("reach", ("reach", 40), 4000, 20, (1, 4, 16)),
    "c4_pick": ("pick", ("pick", 12), 4000, 20, (1, 4, 16)),
    "shipped_pick": ("pick", ("pick", 6), 200, 12, (1, 16, 64)),
}


# the same with run-time entries: name -> the PANDA_CONFIGS entry whose worlds it takes
PANDA_RT_CONFIGS = {"shipped_pick_rt": "shipped_pick", "c4_reach_rt": "c4_reach", "c4_pick_rt": "c4_pick"}
RT_WEIGHTS = dict(reach_dist=20.0, reach_tilt=5.0, pick_goal=7.5, pick_ori=25.0, collision=500.0, shelf_force=3.0, place_grip=3.0)
RT_SPREAD = 0.3
# point_env planners with an arena per sample: name -> the CONFIGS entry whose worlds it takes
POINT_SV_CONFIGS = {"c2_push_sv": "c2_push", "shipped_push_sv": "shipped_push"}
# point_env planners with prior samples from a controller on the device: name -> the CONFIGS entry whose worlds it takes
POINT_PR_CONFIGS = {"c2_push_pr": "c2_push", "shipped_push_pr": "shipped_push"}
POINT_PR_NS = (1, 4, 16, 64)


def panda_world_of(task_phase, K, T, episode, device):
    """57 floats (q9 qd9 | cubeA | cubeB | dyn-obs) and the goal: the world the closed loop (planner K, T) of an episode whose
    cubeA starts displaced (tools/band_stats.py: panda_episodes; episode 0 the reference scene) is in `ticks` ticks into
    `phase`"""
    import closed_loop
    from m3p2i_aip_amd import scenes
    rng = np.random.default_rng([77, episode])
    cube = (0.0, 0.0) if episode == 0 else tuple(rng.uniform(-0.02, 0.02, 2).tolist())
    phase, ticks = task_phase
    res = closed_loop.run("config_panda", [f"mppi.num_samples={K}", f"mppi.horizon={T}", f"mppi.device={device}"], ticks=400,
                          until_task=phase, extra_ticks=ticks, jitter=dict(cube=cube))
    cap = res.get("captured")
    if cap is None or cap["task"] != phase:
        raise RuntimeError(f"episode {episode}: no {phase} scene: {res.get('timeline')}")
    dof, root = np.asarray(cap["dof_state"], np.float32).reshape(-1), np.asarray(cap["root_state"], np.float32)
    w = np.zeros(57, np.float32)
    w[0:9], w[9:18] = dof[0::2], dof[1::2]
    for o, name in ((18, "cubeA"), (31, "cubeB"), (44, "dyn-obs")):
        w[o:o + 13] = root[scenes.actor_index("panda_env", name)]
    return w, cap["goal"]


def world_of(scenario, episode):
    """the reference's initial scene (robot at the origin, box (0, 2), dyn-obs (-2, 2) walking in -y) with the episode's
    jitter: robot / box displaced, the dyn-obs `dyn_phase` ticks into its walk (0.01 m per tick, isaacgym_wrapper.py)"""
    from band_stats import jitter_of
    j = jitter_of(scenario, episode)
    w = np.zeros(18, np.float32)
    w[0:2] = j["robot"]
    bx, by = j["box_start"] if j["box_start"] is not None else (0.0, 2.0)
    w[4:7] = (bx + j["box"][0], by + j["box"][1], 1.0)
    w[11:14] = (-2.0, 2.0 - 0.01 * j["dyn_phase"], 1.0)
    return w


def measure(name, iters, warmup, repeats):
    import torch
    from m3p2i_aip_amd import sampling
    from m3p2i_aip_amd.engine import HipBatch, HipEngine, make_config
    engs = []
    kinds = None
    if name in PANDA_RT_CONFIGS:
        kinds = ("literal", "weighted", "per_sample", "weighted_same_work", "per_sample_same_work")
        name_worlds = PANDA_RT_CONFIGS[name]
    elif name in POINT_SV_CONFIGS:
        kinds = ("scene", "per_sample", "per_sample_same_work")
        name_worlds = POINT_SV_CONFIGS[name]
    elif name in POINT_PR_CONFIGS:
        kinds = ("per_sample_same_work", "priors")
        name_worlds = POINT_PR_CONFIGS[name]
    else:
        name_worlds = name
    if name_worlds in PANDA_CONFIGS:
        task, phase, K, T, ns = PANDA_CONFIGS[name_worlds]
        mm = False
        n_max = max(ns)
        pk = dict(u_min=[-2.0] * 7 + [-1.5] * 2, u_max=[2.0] * 7 + [1.5] * 2, noise_sigma_diag=[10.0] * 7 + [0.8] * 2,
                  lambda_=0.05, pre_height_diff=0.05, dt=0.01)
        knots = sampling.halton_knots(K, T, 9, 4, 2, 0, K, scramble="none")
        worlds = [panda_world_of(phase, K, T, e_i, "cuda:0") for e_i in range(n_max)]
        by_kind = {}
        for kind in kinds or ("literal",):
            for w, goal in worlds:
                e = HipEngine(make_config(K=K, T=T, nu=9, env_type="panda_env", **pk))
                e.set_noise_knots(knots, 2, 0.5)
                e.set_objective(task, goal, gripper_cmd=1 if task == "reach" else 2)
                e.set_world_panda_raw(w)
                if kind == "weighted":
                    e.set_panda_cost_weights(RT_WEIGHTS)
                elif kind == "per_sample":
                    from m3p2i_aip_amd.scenes import spread_panda_scenes
                    e.set_panda_rollout_scenes(spread_panda_scenes(K, RT_SPREAD, seed=1, nominal_rows=(0, K // 2, K - 1)))
                elif kind == "weighted_same_work":
                    e.set_panda_weighted_cost_instance(1)
                elif kind == "per_sample_same_work":
                    e.set_panda_rollout_scenes([None] * K)
                by_kind.setdefault(kind, []).append(e)
        engs = by_kind["literal"]
    else:
        scenario, task, goal, K, T, mm, ns = CONFIGS[name_worlds]
        if name in POINT_PR_CONFIGS:
            ns = POINT_PR_NS
        pk = dict(u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3], lambda_=0.5)
        n_max = max(ns)
        knots = sampling.halton_knots(K, T, 2, 4, 2, 0, K, scramble="none")
        by_kind = {}
        for kind in kinds or (None,):
            for e_i in range(n_max):
                e = HipEngine(make_config(K=K, T=T, nu=2, multi_modal=mm, **pk))
                e.set_noise_knots(knots, 2, 0.5)
                e.relabel_samples()
                e.set_objective(task, goal)
                e.set_world_point_raw(world_of(scenario, e_i))
                if kind == "scene":
                    e.set_point_scene_instance(1)
                elif kind == "per_sample":
                    from m3p2i_aip_amd.scenes import spread_point_scenes
                    e.set_point_rollout_scenes(spread_point_scenes(K, RT_SPREAD, seed=1 + e_i, nominal_rows=(0, K // 2, K - 1)))
                elif kind == "per_sample_same_work":
                    e.set_point_rollout_scenes([None] * K)
                elif kind == "priors":
                    e.set_prior_controller("push_behind", 4)
                by_kind.setdefault(kind, []).append(e)
        engs = by_kind[kinds[0] if kinds else None]
    lib = engs[0].lib
    if name in POINT_PR_CONFIGS:
        batch = HipBatch(n_max, point_runtime=True, point_priors=True)
    elif name in POINT_SV_CONFIGS:
        batch = HipBatch(n_max, point_runtime=True)
    else:
        batch = HipBatch(n_max, panda_runtime=True) if kinds else HipBatch(n_max)
    stream = torch.cuda.current_stream()

    def timed(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(iters):
                fn()
            e1.record(stream)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / iters)
        return float(np.median(out)), out

    rows = []
    for n, kind in [(n, kind) for n in ns for kind in (kinds or (None,))]:
        sel = (by_kind[kind] if kind else engs)[:n]
        arr = (C.c_void_p * n)(*[e._h.value for e in sel])

        def batched():
            rc = lib.m3_batch_command(batch._b, arr, n, None)
            if rc != 0:
                raise RuntimeError(lib.m3_batch_last_error(batch._b).decode())

        def back_to_back():
            for e in sel:
                if lib.m3_command(e._h, None) != 0:
                    raise RuntimeError(lib.m3_last_error(e._h).decode())

        t0 = time.perf_counter()
        b_ms, b_all = timed(batched)
        r_launch, u_launch = batch.launches()
        s_ms, s_all = timed(back_to_back)
        rows.append(dict(n=n, **({"kind": kind} if kind else {}), batched_ms=round(b_ms, 4), back_to_back_ms=round(s_ms, 4),
                         speedup=round(s_ms / b_ms, 3), rollout_launches=r_launch, update_launches=u_launch,
                         panda_lanes_per_sample=sorted({e.panda_lanes_per_sample_used() for e in sel}) if name_worlds in PANDA_CONFIGS else None,
                         batched_repeats_ms=[round(x, 4) for x in b_all], back_to_back_repeats_ms=[round(x, 4) for x in s_all],
                         wall_s=round(time.perf_counter() - t0, 2)))
    if kinds:   # each other kind's batched time over the first kind's batch (literal / scene) of the same worlds and n
        lit = {r["n"]: r["batched_ms"] for r in rows if r["kind"] == kinds[0]}
        for r in rows:
            r["batched_over_" + kinds[0]] = round(r["batched_ms"] / lit[r["n"]], 3)
        engs = [e for es in by_kind.values() for e in es]
    batch.close()
    for e in engs:
        e.close()
    return dict(config=name, K=K, T=T, task=task, multi_modal=mm, rows=rows)


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="comma-separated configuration names")
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)     # (child process: one configuration)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=400.0, help="seconds per configuration")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if a.one:
        print("RESULT" + json.dumps(measure(a.one, a.iters, a.warmup, a.repeats)), flush=True)
        return 0
    from m3p2i_aip_amd import _lib as L
    names = a.only.split(",") if a.only else list(CONFIGS) + list(PANDA_CONFIGS)
    res = dict(tool="batch_bench", build_id=L.load().m3_build_id().decode(), iters=a.iters, warmup=a.warmup,
               repeats=a.repeats, configs=[])
    rc = 0
    for name in names:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--iters", str(a.iters), "--warmup", str(a.warmup),
               "--repeats", str(a.repeats)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            res["configs"].append(dict(config=name, error="time limit"))
            rc = 1
            break      # (a configuration that hung: nothing more on the GPU)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
        if p.returncode != 0 or not lines:
            res["configs"].append(dict(config=name, error="exit %d" % p.returncode, stderr=p.stderr[-2000:]))
            rc = 1
            break
        res["configs"].append(json.loads(lines[-1][6:]))
    line = json.dumps(res)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
