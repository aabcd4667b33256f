"""What the run-time point_env arena (m3_set_point_scene) costs: m3_command at C2 (push, K = 2000, T = 30) on
  per_task        the default handle: the push instance (what bench.py's headline runs)
  general         the same handle with the weighted instance forced on (m3_set_weighted_cost_instance 1): the parent's general,
                  weighted instance -- the yardstick of the two below
  scene_default   the run-time-scene build forced on at the default values (m3_set_point_scene_instance 1)
  scene_custom    a custom arena (the obstacle moved next to the start, a smaller room): the build by the automatic choice
HIP events around `--iters` commands after `--warmup`, ms per command, median / min / max of `--repeats`, the variants
alternating inside every repeat; one JSON line with the ratios to `general`.

    python tools/point_scene_bench.py [--json out.json] [--iters 50] [--warmup 10] [--repeats 7]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, T = 2000, 30
WORLD = np.array([0.1, 1.5, 0, 0, 0.0, 2.0, 1, 0, 0, 0, 0, -2.0, 2.0, 1, 0, 0, 0, 0], np.float32)
CUSTOM = dict(obs_x=-1.0, obs_y=0.5, wall=2.95)


def noise(torch):
    g = torch.Generator().manual_seed(3)
    knots = torch.randn(K, 2, T // 4, generator=g)
    return torch.nn.functional.interpolate(knots, size=T, mode="linear", align_corners=True).permute(0, 2, 1).contiguous().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    import torch
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipEngine, make_config
    variants = [("per_task", {}), ("general", dict(weighted=1)), ("scene_default", dict(force=1)), ("scene_custom", dict(scene=CUSTOM))]
    delta = noise(torch)
    engines = {}
    for name, v in variants:
        e = HipEngine(make_config(K=K, T=T, nu=2, u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3]))
        e.set_noise(delta)
        e.set_objective("push", (-3.75, -3.75))
        e.set_world_point_raw(WORLD)
        if v.get("weighted") is not None:
            e.set_weighted_cost_instance(v["weighted"])
        if v.get("scene"):
            e.set_point_scene(v["scene"])
        if v.get("force") is not None:
            e.set_point_scene_instance(v["force"])
        engines[name] = e
    samples = {name: [] for name, _ in variants}
    for _ in range(a.repeats):          # the variants interleaved inside every repeat
        for name, _ in variants:
            e = engines[name]
            e.reset()
            for _ in range(a.warmup):
                e.command()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                e.command()
            e1.record()
            e1.synchronize()
            samples[name].append(e0.elapsed_time(e1) / a.iters)
    ms = {n: dict(median=float(np.median(s)), min=float(min(s)), max=float(max(s))) for n, s in samples.items()}
    out = dict(tool="point_scene_bench", build_id=L.load().m3_build_id().decode(), device=torch.cuda.get_device_name(0),
               K=K, T=T, task="push", iters=a.iters, warmup=a.warmup, repeats=a.repeats, custom_scene=CUSTOM, ms_per_command=ms,
               ratio_to_general={n: ms[n]["median"] / ms["general"]["median"] for n in ms})
    for e in engines.values():
        e.close()
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
