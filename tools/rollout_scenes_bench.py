"""What one arena PER SAMPLE of the fused point_env rollout (m3_set_point_rollout_scenes) costs, and what it buys.

Timing mode (the default): m3_command of push at K = 2000 x T = 30 and K = 10000 x T = 30 on
  default      the default handle: the push instance (what bench.py's headline runs)
  one_scene    one non-default arena (m3_set_point_scene): the run-time-scene build of the general instance -- the yardstick
  per_sample   K arenas spread around that arena (m3_set_point_rollout_scenes): the same build, each lane's 38 arena words
               loaded from the handle's table
HIP events around `--iters` commands after `--warmup` commands of every variant, ms per command, median / min / max of
`--repeats`, the variants alternating inside every repeat in one process; one JSON line with the ratios to `one_scene`.
`--only NAME` runs the commands of one variant alone (for a kernel trace in a run of its own: the three variants launch
kernels with different names, so the rollout kernel's time is read per name).

    python tools/rollout_scenes_bench.py [--json out.json] [--iters 400] [--warmup 20] [--repeats 7] [--only per_sample]

Episode mode: `--episodes n` serial closed-loop push episodes (tools/closed_loop.run) whose REAL world draws its
`world_point_scene` (box mass, box ground friction, robot-box friction) from `--world-spread`, each run twice on the same
seeds: with the nominal planner, and with `rollout_arena_spread={spread: --planner-spread}`.  Successes, task time and final
error per arm as JSON: evidence, not an assertion.

    python tools/rollout_scenes_bench.py --episodes 20 [--world-spread 0.5] [--planner-spread 0.5] [--ticks 600] [--json out.json]

`--batched` (with --episodes): both arms in lockstep, one set of 2 n episodes (m3p2i_aip_amd.episodes.run_point_episodes with
point_runtime=True: m3_episodes_create_ex, a batch with the per-sample section) -- the episodes of the serial mode, bit for bit.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

T = 30
SIZES = (2000, 10000)
WORLD = np.array([0.1, 1.5, 0, 0, 0.0, 2.0, 1, 0, 0, 0, 0, -2.0, 2.0, 1, 0, 0, 0, 0], np.float32)
CUSTOM = dict(obs_x=-1.0, obs_y=0.5, wall=2.95)
SPREAD = 0.3
VARIANTS = ("default", "one_scene", "per_sample")


def noise(torch, K):
    g = torch.Generator().manual_seed(3)
    knots = torch.randn(K, 2, T // 4, generator=g)
    return torch.nn.functional.interpolate(knots, size=T, mode="linear", align_corners=True).permute(0, 2, 1).contiguous().numpy()


def timing(a):
    import torch
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipEngine, make_config
    from m3p2i_aip_amd.scenes import spread_point_scenes
    names = [a.only] if a.only else list(VARIANTS)
    sizes = {}
    for K in SIZES:
        delta = noise(torch, K)
        engines = {}
        for name in names:
            e = HipEngine(make_config(K=K, T=T, nu=2, u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3]))
            e.set_noise(delta)
            e.set_objective("push", (-3.75, -3.75))
            e.set_world_point_raw(WORLD)
            if name == "one_scene":
                e.set_point_scene(CUSTOM)
            if name == "per_sample":
                e.set_point_rollout_scenes(spread_point_scenes(K, SPREAD, seed=1, base=CUSTOM, nominal_rows=(0, K // 2, K - 1)))
            engines[name] = e
        plan = {}
        for name, e in engines.items():      # warm-up of every variant before any window
            for _ in range(a.warmup):
                e.command()
        torch.cuda.synchronize()
        samples = {name: [] for name in names}
        for _ in range(a.repeats):           # the variants alternate inside every repeat
            for name in names:
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
        for name, e in engines.items():
            plan[name] = dict(rows_set=e.point_rollout_scenes_set(), form=int(e.lib.m3_point_rollout_form_used(e._h)))
            e.close()
        ms = {n: dict(median=float(np.median(s)), min=float(min(s)), max=float(max(s))) for n, s in samples.items()}
        size = dict(K=K, T=T, ms_per_command=ms, launch=plan)
        if "one_scene" in ms:
            size["ratio_to_one_scene"] = {n: ms[n]["median"] / ms["one_scene"]["median"] for n in ms}
        sizes[str(K)] = size
    return dict(tool="rollout_scenes_bench", mode="timing", build_id=L.load().m3_build_id().decode(),
                device=torch.cuda.get_device_name(0), task="push", iters=a.iters, warmup=a.warmup, repeats=a.repeats,
                base_scene=CUSTOM, spread=SPREAD, sizes=sizes)


def world_arena(episode, spread):
    """the real world of an episode: factors in [1 - spread, 1 + spread] on box_m (box_I with it), box_mu_g and mu_rb, from the
    episode's own stream (as tools/band_stats.world_arena_of draws them)"""
    from m3p2i_aip_amd._lib import POINT_SCENE_DEFAULTS as D
    fm, fg, fr = (float(f) for f in np.random.default_rng([7, episode]).uniform(1.0 - spread, 1.0 + spread, 3))
    return dict(box_m=D["box_m"] * fm, box_I=D["box_I"] * fm, box_mu_g=D["box_mu_g"] * fg, mu_rb=D["mu_rb"] * fr)


def episodes(a):
    import band_stats as bs
    import closed_loop
    import torch
    from m3p2i_aip_amd import _lib as L
    sc = "case2_halton_push_coll"
    arms = {"nominal": [], "randomised": ["rollout_arena_spread={spread: %r, seed: 1}" % a.planner_spread]}
    rows = {name: [] for name in arms}
    arenas = [world_arena(e, a.world_spread) for e in range(a.episodes)]
    worlds = ["world_point_scene={" + ", ".join(f"{k}: {v!r}" for k, v in arena.items()) + "}" for arena in arenas]
    if a.batched:      # both arms in lockstep: one set of 2 * episodes episodes (m3p2i_aip_amd.episodes, point_runtime=True)
        from m3p2i_aip_amd.episodes import run_point_episodes
        order = [(name, e) for e in range(a.episodes) for name in arms]
        reps = run_point_episodes([("config_point", bs.overrides(sc, "default") + [worlds[e]] + arms[name], bs.jitter_of(sc, 1 + e))
                                   for name, e in order], max_ticks=a.ticks, point_runtime=True)
        for (name, e), r in zip(order, reps):
            rows[name].append(dict(episode=e, success=bool(r["success"]), sim_time_s=r["sim_time_s"], final_pos_error=r["final_pos_error"],
                                   command_ms_p50=r["tick_ms_p50"], world=arenas[e]))
    for e in range(0 if a.batched else a.episodes):
        arena, world = arenas[e], worlds[e]
        for name, extra in arms.items():                # the same seeds (jitter, world) for both arms
            r = closed_loop.run("config_point", bs.overrides(sc, "default") + [world] + extra, ticks=a.ticks, jitter=bs.jitter_of(sc, 1 + e))
            rows[name].append(dict(episode=e, success=bool(r["success"]), sim_time_s=r["sim_time_s"], final_pos_error=r["final_pos_error"],
                                   command_ms_p50=r["command_ms_p50"], world=arena))
    summary = {}
    for name, rs in rows.items():
        ok = [r for r in rs if r["success"]]
        summary[name] = dict(n=len(rs), successes=len(ok),
                             task_time_s_median_of_successes=float(np.median([r["sim_time_s"] for r in ok])) if ok else None,
                             final_pos_error_median=float(np.median([r["final_pos_error"] for r in rs])),
                             final_pos_error_max=float(max(r["final_pos_error"] for r in rs)),
                             command_ms_p50_median=float(np.median([r["command_ms_p50"] for r in rs])))
    return dict(tool="rollout_scenes_bench", mode="episodes", build_id=L.load().m3_build_id().decode(),
                device=torch.cuda.get_device_name(0), scenario=sc, ticks=a.ticks, world_spread=a.world_spread, batched=bool(a.batched),
                planner_spread=a.planner_spread, summary=summary, episodes=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=VARIANTS)
    ap.add_argument("--episodes", type=int, default=0)
    ap.add_argument("--world-spread", type=float, default=0.5)
    ap.add_argument("--planner-spread", type=float, default=0.5)
    ap.add_argument("--ticks", type=int, default=600)
    ap.add_argument("--batched", action="store_true",
                    help="--episodes: both arms in lockstep (one set; command_ms_p50 is then the set's tick time)")
    a = ap.parse_args()
    out = episodes(a) if a.episodes else timing(a)
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
