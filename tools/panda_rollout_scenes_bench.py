"""What one workspace per sample of the fused panda_env rollout (m3_set_panda_rollout_scenes) costs at C4's size: m3_command at
K = 4000 x T = 20 of
  reach   in the configured initial scene (gripper open), and
  pick    with cubeA held (gripper closing),
each on three handles:
  twin      the weighted family forced at the DEFAULT weights (m3_set_panda_weighted_cost_instance 1) in the default workspace:
            k_rollout_panda_w, the kernels the per-sample family is built from -- the yardstick
  rows      the per-sample family with K DEFAULT rows: the same arithmetic on the same values (the same results, byte for
            byte), 22 words of the scene read from the table per sample -- what the family itself costs
  spread    the per-sample family with a spread of workspaces (scenes.spread_panda_scenes, --spread, the fields cube_m, mu,
            obs_m; samples 0, K / 2 and K - 1 nominal): other models, so the samples meet other contacts and the update picks
            other plans -- not a like-for-like row
HIP events around `--iters` commands, ms per command, median / min / max of `--repeats`; the three handles alternate inside
every repeat in one process and each timed window follows its own warm-up directly (the method of
tools/panda_cost_weights_bench.py).  One JSON line with the ratios to `twin` and each handle's own window-to-window spread
((max - min) / median).  `--only NAME` runs one handle alone (for a kernel trace in a run of its own).

    python tools/panda_rollout_scenes_bench.py [--json out.json] [--iters 200] [--warmup 10] [--repeats 7] [--spread 0.3] [--only rows]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, T = 4000, 20
GOAL = (0.2, 0.2, 1.115, 0.0, 0.0, 0.0, 1.0)
VARIANTS = ("twin", "rows", "spread")
TASKS = (("reach", 1), ("pick", 2))


def world(P, task):
    """the 57 floats the handle starts from: reach -- the configured initial scene; pick -- cubeA held"""
    from tests.panda_worlds import grasp_world
    if task == "reach":
        return P.raw57(P.init_world(1)[0])
    return P.raw57(grasp_world(P, P.default_scene()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--spread", type=float, default=0.3)
    ap.add_argument("--only", choices=VARIANTS)
    a = ap.parse_args()
    import torch
    import oracle
    oracle.load()
    import oracle.panda as P
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipEngine, make_config
    from m3p2i_aip_amd.scenes import spread_panda_scenes
    names = [a.only] if a.only else list(VARIANTS)
    delta = np.random.default_rng(3).standard_normal((K, T, 9)).astype(np.float32)
    spread_rows = spread_panda_scenes(K, a.spread, seed=1, nominal_rows=(0, K // 2, K - 1))
    rows = {}
    for task, grip in TASKS:
        engines = {}
        for name in names:
            e = HipEngine(make_config(K=K, T=T, nu=9, env_type="panda_env", u_min=[-2.0] * 7 + [-1.5] * 2,
                                      u_max=[2.0] * 7 + [1.5] * 2, noise_sigma_diag=[10.0] * 7 + [0.8] * 2, lambda_=0.05,
                                      pre_height_diff=0.05, dt=0.01))
            e.set_noise(delta)
            e.set_objective(task, GOAL, gripper_cmd=grip)
            if name == "twin":
                e.set_panda_weighted_cost_instance(1)
            if name == "rows":
                e.set_panda_rollout_scenes([None] * K)
            if name == "spread":
                e.set_panda_rollout_scenes(spread_rows)
            e.set_world_panda_raw(world(P, task))
            engines[name] = e
        samples = {name: [] for name in names}
        for _ in range(a.repeats):           # the handles alternate inside every repeat; warm-up directly before each window
            for name in names:
                e = engines[name]
                e.reset()                    # (the rows survive it)
                for _ in range(a.warmup):
                    e.command()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    e.command()
                e1.record()
                e1.synchronize()
                samples[name].append(e0.elapsed_time(e1) / a.iters)
        launch = {}
        for name, e in engines.items():
            launch[name] = dict(rollout_scenes=int(e.panda_rollout_scenes_set()), weighted=int(e.panda_weighted_cost_instance_used()),
                                lanes_per_sample=e.panda_lanes_per_sample_used())
            e.close()
        ms = {n: dict(median=float(np.median(s)), min=float(min(s)), max=float(max(s))) for n, s in samples.items()}
        row = dict(ms_per_command=ms, launch=launch, spread={n: (m["max"] - m["min"]) / m["median"] for n, m in ms.items()})
        if "twin" in ms:
            row["ratio_to_twin"] = {n: ms[n]["median"] / ms["twin"]["median"] for n in ms}
        rows[task] = row
    out = dict(tool="panda_rollout_scenes_bench", build_id=L.load().m3_build_id().decode(), device=torch.cuda.get_device_name(0),
               K=K, T=T, iters=a.iters, warmup=a.warmup, repeats=a.repeats, workspace_spread=a.spread,
               spread_fields=["cube_m", "mu", "obs_m"], rows=rows)
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
