"""Batched panda_env episodes: the lockstep tick of m3_panda_episodes_* for N = 1, 8, 16, 60 reactive
pick-and-place episodes at the shipped size (K = 200, T = 12) and at C4 (K = 4000, T = 20) -- p50 ms per tick over ticks
1.., split into observe / host task planners / act, construction and tick 0 separately -- against the serial loop of
tools/closed_loop.run on --serial-n of the same episodes, scaled to N (its cost is linear in the number of episodes).

    python tools/panda_episode_bench.py [--json out.json] [--ticks 150] [--serial-n 4] [--sizes shipped,c4] [--ns 1,8,16,60]
                                        [--runtime]

--runtime: per N three sets in ONE process, their ticks interleaved (set A's tick t, set B's, set C's, then tick t + 1) so that
clock and thermal drift fall on all three alike: `plain` (m3_panda_episodes_create), `default_rt` (the run-time set,
M3_PANDA_EPISODES_RUNTIME, every workspace and weight the default: identical work on the rows kernels and the batch's run-time
table) and `mixed_rt` (the run-time set, the episodes in a 5-cycle of workspaces, weights and spreads: MIXED below).  The
row that matters is default_rt against plain (`rt_over_plain`).

The serial loop and every kernel it launches are the parent's (this feature adds beside them), so the serial side measured
here is the parent commit's.  Serial construction is timed by building the planner side alone, as tools/episode_bench.py.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = {"shipped": ["mppi.num_samples=200", "mppi.horizon=12"], "c4": ["mppi.num_samples=4000", "mppi.horizon=20"]}


def jitter(e):
    rng = np.random.default_rng([77, e % 60])          # band_stats.panda_episodes
    return dict(cube=(0.0, 0.0) if e % 60 == 0 else tuple(rng.uniform(-0.02, 0.02, 2).tolist()))


def batched(size, n, ticks):
    from m3p2i_aip_amd.episodes import build_panda_set
    es = build_panda_set([("config_panda", SIZES[size], jitter(e)) for e in range(n)], max_ticks=ticks + 1)
    try:
        es.start()
        while es.active and len(es.lat) < ticks:
            es.tick()
        lat, sp = np.array(es.lat[3:]) * 1e3, np.array(es.split[3:]) * 1e3
        p = np.percentile(sp, 50, axis=0)
        return dict(size=size, n=n, build_s=es.build_s, tick0_s=es.first_s, ticks=len(es.lat),
                    tick_ms_p50=float(np.percentile(lat, 50)), tick_ms_p99=float(np.percentile(lat, 99)),
                    observe_ms_p50=float(p[0]), host_ms_p50=float(p[1]), act_ms_p50=float(p[2]),
                    host_share=float(p[1] / max(np.percentile(lat, 50), 1e-9)))
    finally:
        es.close()


# the 5-cycle of a mixed_rt set: the reference's episode, a planner workspace, a heavier real cube, a tuned weight, a heavier
# real cube planned for over a spread of models
MIXED = [[], ["panda_scene={table: [0, 0, 0.99, 0.6, 0.6, 0.025], mu: 0.5}"], ["world_panda_scene={cube_m: 0.2}"],
         ["panda_cost_weights={pick_ori: 25.0}"],
         ["world_panda_scene={cube_m: 0.2}", "rollout_workspace_spread={spread: 0.3, seed: 1}"]]


def batched_runtime(size, n, ticks):
    """the three sets of --runtime, interleaved tick by tick; one row each"""
    from m3p2i_aip_amd.episodes import build_panda_set
    plain_eps = [("config_panda", SIZES[size], jitter(e)) for e in range(n)]
    mixed_eps = [("config_panda", SIZES[size] + MIXED[e % 5], jitter(e)) for e in range(n)]
    sets = {}
    try:
        sets["plain"] = build_panda_set(plain_eps, max_ticks=ticks + 1)
        sets["default_rt"] = build_panda_set(plain_eps, max_ticks=ticks + 1, panda_runtime=True)
        sets["mixed_rt"] = build_panda_set(mixed_eps, max_ticks=ticks + 1, panda_runtime=True)
        for es in sets.values():
            es.start()
        # `act` does not synchronise: alone, a set pays for its command and post kernel in its NEXT observe.  Interleaved on one
        # stream the next observe is another set's, so every tick here ends with a synchronisation of its own and the wait is
        # booked to the set that launched the work (wait_ms); a tick is observe + host + act + wait
        import torch
        wait = {kind: [] for kind in sets}
        while all(es.active and len(es.lat) < ticks for es in sets.values()):
            for kind, es in sets.items():
                es.tick()
                t = time.perf_counter()
                torch.cuda.synchronize()
                wait[kind].append(time.perf_counter() - t)
        rows = []
        for kind, es in sets.items():
            wt = np.array(wait[kind][3:]) * 1e3
            lat, sp = np.array(es.lat[3:]) * 1e3 + wt, np.array(es.split[3:]) * 1e3
            p = np.percentile(sp, 50, axis=0)
            rows.append(dict(size=size, n=n, kind=kind, build_s=es.build_s, tick0_s=es.first_s, ticks=len(es.lat),
                             tick_ms_p50=float(np.percentile(lat, 50)), tick_ms_p99=float(np.percentile(lat, 99)),
                             observe_ms_p50=float(p[0]), host_ms_p50=float(p[1]), act_ms_p50=float(p[2]),
                             wait_ms_p50=float(np.percentile(wt, 50))))
        for r in rows[1:]:
            r["rt_over_plain"] = {k: r[k] / max(rows[0][k], 1e-9) for k in ("tick_ms_p50", "observe_ms_p50", "act_ms_p50", "wait_ms_p50")}
        return rows
    finally:
        for es in sets.values():
            es.close()


def serial(size, n, ticks):
    import closed_loop
    from m3p2i_aip_amd import compat
    walls, per_tick = [], []
    for e in range(n):
        t0 = time.perf_counter()
        r = closed_loop.run("config_panda", SIZES[size], ticks=ticks + 1, jitter=jitter(e))
        walls.append(time.perf_counter() - t0)
        per_tick.append((r["ticks"], r["command_ms_p50"]))
    compat.install(force_standins=True)
    t0 = time.perf_counter()
    for e in range(n):
        t = closed_loop.Tamp(compat.make_config("config_panda", SIZES[size]))
        t.close()
    build = (time.perf_counter() - t0) / n
    ticks_run = float(np.mean([t for t, _ in per_tick]))
    loop = float(np.mean(walls)) - build                       # tick 0 (the probe) included
    return dict(size=size, episodes=n, build_s_per_episode=build, loop_s_per_episode=loop, ticks=ticks_run,
                tick_ms_per_episode=loop / ticks_run * 1e3, command_ms_p50=float(np.mean([c for _, c in per_tick])))


def main(argv):
    out, ticks, serial_n, sizes, ns, runtime = None, 150, 4, ["shipped", "c4"], [1, 8, 16, 60], False
    it = iter(argv)
    for a in it:
        if a == "--runtime":
            runtime = True
        elif a == "--json":
            out = next(it)
        elif a == "--ticks":
            ticks = int(next(it))
        elif a == "--serial-n":
            serial_n = int(next(it))
        elif a == "--sizes":
            sizes = next(it).split(",")
        elif a == "--ns":
            ns = [int(x) for x in next(it).split(",")]
    from m3p2i_aip_amd import _lib as L
    res = dict(tool="panda_episode_bench", build_id=L.load().m3_build_id().decode(), ticks=ticks, sizes={})
    for size in sizes:
        s = serial(size, serial_n, ticks)
        print("serial", json.dumps(s), flush=True)
        rows = []
        for n in ns:
            for b in batched_runtime(size, n, ticks) if runtime else [batched(size, n, ticks)]:
                b["serial_tick_ms_scaled"] = s["tick_ms_per_episode"] * n
                b["tick_speedup"] = b["serial_tick_ms_scaled"] / b["tick_ms_p50"]
                rows.append(b)
                print("batched", json.dumps(b), flush=True)
        res["sizes"][size] = dict(serial=s, batched=rows)
        if out:      # (written as it grows: a long run cut short keeps what it measured)
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
