"""Batched closed-loop episodes: tick time of m3_episodes_tick for N = 1, 8, 64, 480 episodes, and wall time
of the 8-scenario band (tools/band_stats.py) per size, batched against serial, planner construction shown separately.

    python tools/episode_bench.py [--json out.json] [--n 60] [--serial-n 4] [--ticks 100]

The serial band time is measured on --serial-n episodes per scenario and scaled to --n (the serial loop's cost is linear
in the number of episodes); construction of the serial runs is timed by building their planners alone.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def tick_times(n, ticks):
    """n case2_halton_push_coll episodes at BASELINE size (K = 2000, T = 30): ms per tick over `ticks` ticks."""
    import band_stats as bs
    from m3p2i_aip_amd.episodes import build_set
    eps = [("config_point", bs.overrides("case2_halton_push_coll", "baseline"), bs.jitter_of("case2_halton_push_coll", e % 60))
           for e in range(n)]
    es = build_set(eps, max_ticks=ticks + 1)
    try:
        es.start()
        for _ in range(ticks):
            if not es.running:
                break
            es.tick()
        lat = np.array(es.lat[3:]) * 1e3
        return dict(n=n, K=2000, T=30, build_s=es.build_s, ticks=len(es.lat), tick_ms_p50=float(np.percentile(lat, 50)),
                    tick_ms_p99=float(np.percentile(lat, 99)), tick_ms_mean=float(lat.mean()))
    finally:
        es.close()


def serial_band(size, n):
    import band_stats as bs
    import closed_loop
    from m3p2i_aip_amd import compat
    t0 = time.perf_counter()
    for sc in bs.SCENARIOS:
        for e in range(n):
            closed_loop.run("config_point", bs.overrides(sc, size), ticks=800, jitter=bs.jitter_of(sc, e))
    wall = time.perf_counter() - t0
    compat.install(force_standins=True)
    t0 = time.perf_counter()
    for sc in bs.SCENARIOS:          # construction alone: one Tamp per episode, as closed_loop.run builds it
        for e in range(n):
            t = closed_loop.Tamp(compat.make_config("config_point", bs.overrides(sc, size)))
            t.close()
    build = time.perf_counter() - t0
    return dict(episodes=8 * n, wall_s=wall, build_s=build, loop_s=wall - build)


def batched_band(size, n):
    import band_stats as bs
    from m3p2i_aip_amd.episodes import run_point_episodes
    eps = [("config_point", bs.overrides(sc, size), bs.jitter_of(sc, e)) for sc in bs.SCENARIOS for e in range(n)]
    t0 = time.perf_counter()
    reps = run_point_episodes(eps, max_ticks=800)
    wall = time.perf_counter() - t0
    return dict(episodes=len(eps), wall_s=wall, build_s=reps[0]["build_s"], loop_s=reps[0]["loop_s"],
                tick_ms_p50=reps[0]["tick_ms_p50"], tick_ms_p99=reps[0]["tick_ms_p99"],
                successes=int(sum(r["success"] for r in reps)))


def main(argv):
    out, n, serial_n, ticks = None, 60, 4, 100
    it = iter(argv)
    for a in it:
        if a == "--json":
            out = next(it)
        elif a == "--n":
            n = int(next(it))
        elif a == "--serial-n":
            serial_n = int(next(it))
        elif a == "--ticks":
            ticks = int(next(it))
    res = dict(tick=[], band={})
    for k in (1, 8, 64, 480):
        r = tick_times(k, ticks)
        res["tick"].append(r)
        print(json.dumps(r), flush=True)
    for size in ("default", "baseline"):
        b = batched_band(size, n)
        s = serial_band(size, serial_n)
        scale = n / serial_n
        s_scaled = dict(episodes=8 * n, wall_s=s["wall_s"] * scale, build_s=s["build_s"] * scale, loop_s=s["loop_s"] * scale,
                        measured_on=s)
        res["band"][size] = dict(batched=b, serial=s_scaled, loop_speedup=s_scaled["loop_s"] / b["loop_s"],
                                 wall_speedup=s_scaled["wall_s"] / b["wall_s"])
        print(size, json.dumps(res["band"][size]), flush=True)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
