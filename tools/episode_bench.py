"""Batched closed-loop episodes: tick time of m3_episodes_tick for N = 1, 8, 64, 480 episodes, and wall time
of the 8-scenario band (tools/band_stats.py) per size, batched against serial, planner construction shown separately.

    python tools/episode_bench.py [--json out.json] [--n 60] [--serial-n 4] [--ticks 100]
    python tools/episode_bench.py --arena-rows [--json out.json] [--rows 64] [--repeats 5] [--ticks 8]
    python tools/episode_bench.py --rollout-arenas [--json out.json] [--rows 64] [--repeats 5] [--ticks 8]

--arena-rows: what an arena per world row costs (m3_set_point_scene_rows, k_episodes_post_sv).  Three sets of --rows case2 push
episodes at BASELINE size whose planners all plan in the reference's arena (the batched command is the same work in all three):
`single` -- one custom arena on the world handle (m3_set_point_scene: k_episodes_post_s, the kernel of the parent commit),
`rows_same` -- the same arena as --rows identical rows, `rows_distinct` -- --rows different arenas.  The variants alternate
inside each of --repeats repeats of --ticks ticks; p50 ms per m3_episodes_tick of each and the ratios to `single`.

--rollout-arenas: what an arena per SAMPLE of every planner costs in lockstep (m3_episodes_create_ex with
M3_EPISODES_ROLLOUT_SCENES, kb_rollout_point_sv*).  Two sets of --rows case2 push episodes at BASELINE size in the
nominal world, both built with point_runtime=True: `nominal` -- every planner in the reference's arena (the batched push
instance), `rollout_arenas` -- every planner with `rollout_arena_spread={spread: 0.3, seed: 1 + e}` (one per-sample group).  The
two alternate inside each of --repeats repeats of --ticks ticks; p50 ms per m3_episodes_tick of each and the ratio.

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


def arena_rows_times(n=64, repeats=5, ticks=8):
    import band_stats as bs
    from m3p2i_aip_amd._lib import POINT_SCENE_DEFAULTS as D
    from m3p2i_aip_amd.episodes import build_set
    sc = "case2_halton_push_coll"

    def arena(f):      # the box heavier / lighter by the factor f, its frictions moved with it
        return dict(box_m=D["box_m"] * f, box_I=D["box_I"] * f, box_mu_g=D["box_mu_g"] * (2.0 - f), mu_rb=D["mu_rb"] * f)

    def world(a):
        return "world_point_scene={" + ", ".join(f"{k}: {v!r}" for k, v in a.items()) + "}"

    one = arena(1.125)
    distinct = [arena(0.8 + 0.4 * e / max(n - 1, 1)) for e in range(n)]
    plans = dict(single=[one] * n, rows_same=[one] * n, rows_distinct=distinct)
    sets = {}
    try:
        for name, arenas in plans.items():
            eps = [("config_point", bs.overrides(sc, "baseline") + [world(arenas[e])], bs.jitter_of(sc, e % 60)) for e in range(n)]
            es = sets[name] = build_set(eps, max_ticks=repeats * ticks + 4)
            if name == "rows_same":      # (episodes that agree build the single-arena world: give it the rows by hand)
                es.real._engine.set_point_scene_rows(arenas)
            assert es.real._engine.point_scene_rows_set() == (name != "single")
            es.start()
            for _ in range(3):           # warm-up ticks, not counted
                es.tick()
            es.lat.clear()
        for _ in range(repeats):         # the variants interleaved inside every repeat
            for es in sets.values():
                for _ in range(ticks):
                    if es.running:
                        es.tick()
        out = dict(n=n, K=2000, T=30, repeats=repeats, ticks_per_repeat=ticks, tick_ms_p50={}, tick_ms_min={}, ticks={})
        for name, es in sets.items():
            lat = np.array(es.lat) * 1e3
            out["tick_ms_p50"][name] = float(np.percentile(lat, 50))
            out["tick_ms_min"][name] = float(lat.min())
            out["ticks"][name] = len(lat)
        out["ratio_to_single"] = {k: v / out["tick_ms_p50"]["single"] for k, v in out["tick_ms_p50"].items()}
        return out
    finally:
        for es in sets.values():
            es.close()


def _two_sets_times(plans, base, n, repeats, ticks, spread, check):
    """two lockstep sets of n episodes of one scenario, `plans`: name -> (extra overrides of episode e, build_set's switches),
    interleaved inside every repeat; the second set's tick p50 over the first's is `ratio_to_<first>`"""
    import band_stats as bs
    from m3p2i_aip_amd.episodes import build_set
    sc = "case2_halton_push_coll"
    sets = {}
    try:
        for name, (extra, kw) in plans.items():
            eps = [("config_point", bs.overrides(sc, "baseline") + extra(e), bs.jitter_of(sc, e % 60)) for e in range(n)]
            es = sets[name] = build_set(eps, max_ticks=repeats * ticks + 4, **kw)
            es.start()
            assert all(check(s.motion_planner._engine) == (name != base) for s in es.sides)
            for _ in range(3):           # warm-up ticks, not counted
                es.tick()
            es.lat.clear()
        for _ in range(repeats):         # the two sets interleaved inside every repeat
            for es in sets.values():
                for _ in range(ticks):
                    if es.running:
                        es.tick()
        out = dict(n=n, K=2000, T=30, spread=spread, repeats=repeats, ticks_per_repeat=ticks, tick_ms_p50={}, tick_ms_min={}, ticks={},
                   rollout_launches={k: es.batch.launches()[0] for k, es in sets.items()})
        for name, es in sets.items():
            lat = np.array(es.lat) * 1e3
            out["tick_ms_p50"][name] = float(np.percentile(lat, 50))
            out["tick_ms_min"][name] = float(lat.min())
            out["ticks"][name] = len(lat)
        other = [k for k in plans if k != base][0]
        out["ratio_to_" + base] = out["tick_ms_p50"][other] / out["tick_ms_p50"][base]
        return out
    finally:
        for es in sets.values():
            es.close()


def rollout_arenas_times(n=64, repeats=5, ticks=8, spread=0.3):
    arenas = lambda e: ["rollout_arena_spread={spread: %r, seed: %d}" % (spread, 1 + e)]
    return _two_sets_times(dict(nominal=(lambda e: [], dict(point_runtime=True)), rollout_arenas=(arenas, dict(point_runtime=True))),
                           "nominal", n, repeats, ticks, spread, lambda eng: eng.point_rollout_scenes_set())


def priors_times(n=64, repeats=5, ticks=8, spread=0.3):
    """The lockstep tick with controller planners (`prior_samples={controller: push_behind, n: 4, device: true}`: one
    kb_prior_controllers launch and one kb_rollout_point_pr* group per tick) beside the `rollout arenas` set (an arena per sample of
    every planner: the kernels the prior build twins)."""
    arenas = lambda e: ["rollout_arena_spread={spread: %r, seed: %d}" % (spread, 1 + e)]
    priors = lambda e: ["prior_samples={controller: push_behind, n: 4, device: true}"]
    return _two_sets_times(dict(rollout_arenas=(arenas, dict(point_runtime=True)), priors=(priors, dict(point_priors=True))),
                           "rollout_arenas", n, repeats, ticks, spread, lambda eng: eng.prior_controller() is not None)


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
    if "--arena-rows" in argv:
        opt = dict(zip(argv, argv[1:]))
        res = dict(arena_rows=arena_rows_times(int(opt.get("--rows", 64)), int(opt.get("--repeats", 5)), int(opt.get("--ticks", 8))))
        print(json.dumps(res), flush=True)
        if opt.get("--json"):
            os.makedirs(os.path.dirname(opt["--json"]) or ".", exist_ok=True)
            json.dump(res, open(opt["--json"], "w"), indent=1)
        return
    for switch, key, fn in (("--rollout-arenas", "rollout_arenas", rollout_arenas_times), ("--priors", "priors", priors_times)):
        if switch in argv:
            from m3p2i_aip_amd import _lib as L
            opt = dict(zip(argv, argv[1:]))
            res = {"build_id": L.load().m3_build_id().decode(),
                   key: fn(int(opt.get("--rows", 64)), int(opt.get("--repeats", 5)), int(opt.get("--ticks", 8)))}
            print(json.dumps(res), flush=True)
            if opt.get("--json"):
                os.makedirs(os.path.dirname(opt["--json"]) or ".", exist_ok=True)
                json.dump(res, open(opt["--json"], "w"), indent=1)
            return
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
