"""What sample groups (m3_set_sample_groups) cost and what they buy.

Part 1, the cost: push, K = 2000, T = 30, an arena per sample (the M = 4 arenas of groups.grouped_layout, the noise tiled), ms
  per m3_command on ONE handle, the arms interleaved in one process: `without` (no groups: the kernels of a handle that never
  had any) and `groups` (M = 4, worst_frac 1).  Also the aggregate kernel's own time: the rollout phase of m3_timing with and
  without groups, and `--agg-launches` back-to-back launches of m3_aggregate_sample_groups alone.  `--without-only` runs the
  first arm alone and touches none of the feature's entry points: the same file, copied into a checkout of the parent commit,
  measures the parent.  Bar: `groups` at most 5 % above the parent's `without`.
Part 2, the benefit: the closed-loop push episodes of tools/rollout_scenes_bench.py (the real world's box mass, ground friction
  and robot-box friction drawn from --world-spread, the same seeds for every arm), run serially: the nominal planner,
  `rollout_arena_spread`, and `rollout_arena_groups` at M = 4 and 8 with worst 1.0 and 0.25.  Successes, task time and final
  error as they come: evidence, not an assertion.

    python tools/sample_groups_bench.py --part 1 [--rounds 7] [--commands 200] [--without-only] [--out cost.json]
    python tools/sample_groups_bench.py --part 2 [--episodes 20] [--ticks 600] [--arms nominal,spread,...] [--out benefit.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

K, T, M = 2000, 30, 4
WORLD = np.array([0.1, 1.5, 0, 0, 0.0, 2.0, 1, 0, 0, 0, 0, -2.0, 2.0, 1, 0, 0, 0, 0], np.float32)


def _layout(K, M):
    """groups.grouped_layout and groups.first_members restated for a single-mode planner, so that --without-only runs in a
    checkout that has no groups module: (group_of, model_of, src)"""
    G = (K - 1) // M
    group_of, model_of, src = np.full(K, -1, np.int64), np.full(K, -1, np.int64), np.arange(K)
    for g in range(G):
        for m in range(M):
            group_of[g + m * G], model_of[g + m * G], src[g + m * G] = g, m, g
    return group_of, model_of, src


def cost(a):
    import torch
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipEngine, make_config
    from m3p2i_aip_amd.scenes import spread_point_scenes
    group_of, model_of, src = _layout(K, M)
    if not a.without_only:
        from m3p2i_aip_amd import groups
        g2, m2 = groups.grouped_layout(K, M, False)
        assert np.array_equal(g2, group_of) and np.array_equal(m2, model_of) and np.array_equal(groups.first_members(g2), src)
    gen = torch.Generator().manual_seed(3)
    knots = torch.randn(K, 2, T // 4, generator=gen)
    delta = torch.nn.functional.interpolate(knots, size=T, mode="linear", align_corners=True).permute(0, 2, 1).contiguous().numpy()
    arenas = spread_point_scenes(M, 0.3, seed=1)
    eng = HipEngine(make_config(K=K, T=T, nu=2, u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3]))
    eng.set_objective("push", (-3.75, -3.75))
    eng.set_noise(np.ascontiguousarray(delta[src]))
    eng.set_point_rollout_scenes([arenas[m] if m >= 0 else None for m in model_of.tolist()])
    eng.set_world_point_raw(WORLD)
    arms = ["without"] if a.without_only else ["without", "groups"]
    ms = {n: [] for n in arms}
    phase = {n: [] for n in arms}
    try:
        for r in range(a.rounds + 1):            # (round 0 warms every arm up and is dropped)
            for name in arms:
                if not a.without_only:
                    eng.set_sample_groups(group_of if name == "groups" else None, 1.0)
                eng.reset()
                eng.enable_timing(False)
                for _ in range(20):
                    eng.command()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.commands):
                    eng.command()
                e1.record()
                torch.cuda.synchronize()
                eng.enable_timing(True)          # (the phases of one command: the rollout phase ends behind the aggregation)
                ph = []
                for _ in range(20):
                    eng.command()
                    ph.append(eng.timing().rollout_ms)
                if r:
                    ms[name].append(e0.elapsed_time(e1) / a.commands)
                    phase[name].append(float(np.median(ph)))
        out = {n: dict(ms_median=float(np.median(v)), ms_min=float(np.min(v)), ms_max=float(np.max(v)), rounds=len(v),
                       rollout_phase_ms_median=float(np.median(phase[n]))) for n, v in ms.items()}
        res = dict(tool="sample_groups_bench", part="cost", K=K, T=T, M=M, task="push", commands_per_block=a.commands,
                   device=torch.cuda.get_device_name(0), build_id=L.load().m3_build_id().decode(), arms=out)
        if not a.without_only:
            out["groups"]["vs_without"] = out["groups"]["ms_median"] / out["without"]["ms_median"]
            eng.set_sample_groups(group_of, 1.0)
            eng.enable_timing(False)
            eng.command()
            lone = []
            for _ in range(a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.agg_launches):
                    eng.aggregate_sample_groups()
                e1.record()
                torch.cuda.synchronize()
                lone.append(e0.elapsed_time(e1) / a.agg_launches * 1000.0)
            res["aggregate_kernel"] = dict(
                us_per_launch_back_to_back_median=float(np.median(lone)), launches_per_block=a.agg_launches,
                rollout_phase_delta_us=1000.0 * (out["groups"]["rollout_phase_ms_median"] - out["without"]["rollout_phase_ms_median"]),
                groups=int(eng.sample_groups_set()))
    finally:
        eng.close()
    return res


def benefit(a):
    import closed_loop
    import band_stats as bs
    import torch
    from m3p2i_aip_amd import _lib as L
    from rollout_scenes_bench import world_arena
    sc = "case2_halton_push_coll"
    s = a.planner_spread
    arms = {"nominal": [], "spread": ["rollout_arena_spread={spread: %r, seed: 1}" % s]}
    for m in (4, 8):
        for w in (1.0, 0.25):
            arms["groups_M%d_worst%g" % (m, w)] = ["rollout_arena_groups={models: %d, spread: %r, seed: 1, worst: %r}" % (m, s, w)]
    if a.arms:
        arms = {n: arms[n] for n in a.arms.split(",")}
    arenas = [world_arena(e, a.world_spread) for e in range(a.episodes)]
    worlds = ["world_point_scene={" + ", ".join(f"{k}: {v!r}" for k, v in arena.items()) + "}" for arena in arenas]
    res = dict(tool="sample_groups_bench", part="benefit", build_id=L.load().m3_build_id().decode(),
               device=torch.cuda.get_device_name(0), scenario=sc, size="default (K = 200, T = 15)", ticks=a.ticks,
               world_spread=a.world_spread, planner_spread=s, episodes_per_arm=a.episodes, summary={}, episodes={})
    for name, extra in arms.items():             # (serial; every arm on the same seeds: jitter and world per episode)
        rows = []
        for e in range(a.episodes):
            r = closed_loop.run("config_point", bs.overrides(sc, "default") + [worlds[e]] + extra, ticks=a.ticks, jitter=bs.jitter_of(sc, 1 + e))
            rows.append(dict(episode=e, success=bool(r["success"]), sim_time_s=r["sim_time_s"], final_pos_error=r["final_pos_error"],
                             command_ms_p50=r["command_ms_p50"]))
        ok = [r for r in rows if r["success"]]
        res["episodes"][name] = rows
        res["summary"][name] = dict(n=len(rows), successes=len(ok),
                                    task_time_s_median_of_successes=float(np.median([r["sim_time_s"] for r in ok])) if ok else None,
                                    final_pos_error_median=float(np.median([r["final_pos_error"] for r in rows])),
                                    final_pos_error_max=float(max(r["final_pos_error"] for r in rows)),
                                    command_ms_p50_median=float(np.median([r["command_ms_p50"] for r in rows])))
        print(json.dumps({name: res["summary"][name]}), flush=True)
        if a.out:                                # (kept arm by arm: a run that is cut short leaves what it finished)
            _write(a.out, res)
    return res


def _write(path, res):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("1", "2"), required=True)
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--commands", type=int, default=200)
    ap.add_argument("--agg-launches", type=int, default=2000)
    ap.add_argument("--without-only", action="store_true")
    ap.add_argument("--episodes", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=600)
    ap.add_argument("--world-spread", type=float, default=0.5)
    ap.add_argument("--planner-spread", type=float, default=0.5)
    ap.add_argument("--arms", help="part 2: a comma-separated subset of the arms")
    a = ap.parse_args()
    res = cost(a) if a.part == "1" else benefit(a)
    print(json.dumps(res if a.part == "1" else res["summary"], indent=1))
    if a.out:
        _write(a.out, res)


if __name__ == "__main__":
    main()
