"""N closed-loop episodes per scenario of the reference's recorded experiments, with the start jittered
(deterministic seeds): statistics of what the reference logged per run (plot/plot_point.py:26-34) -- final
block-to-goal error, task time, dyn-obs collisions -- next to the logged statistics (tests/golden/behaviour_band.json).

    python tools/band_stats.py [--n 20] [--json out.json] [--size baseline|default] [--avoid] [--batched]
                               [--world-arena-spread S] [--runtime] [--priors] [key=value ...] [scenario ...]

--batched: all episodes of all named scenarios in lockstep, one library call per tick (m3p2i_aip_amd/episodes.py,
DESIGN.md §7c): the same per-episode results as the serial runs, bit for bit.  The `panda` rows likewise, the n episodes
of each row in lockstep (two library calls per tick with the host's task planners in between, §7d).

--runtime (with --batched, the `panda` rows): the run-time set of the lockstep panda episodes (run_panda_episodes(...,
panda_runtime=True)), which takes `panda_scene=...`, `world_panda_scene=...`, `panda_cost_weights=...` and
`rollout_workspace_spread=...` given as key=value arguments -- e.g. --batched --runtime 'world_panda_scene={cube_m: 0.2}'
'rollout_workspace_spread={spread: 0.3, seed: 1}' panda: does a planner that plans over a spread of models succeed more often
in a world whose cube is heavier than its model's?  The serial `panda` rows take the same keys.

--priors (with --batched): the lockstep set created for planners with prior samples (run_point_episodes(..., point_priors=True)),
which takes 'prior_samples={controller: push_behind, n: 4, device: true}' given as a key=value argument: every planner hears that
controller, computed on the device from its episode's row of the world every tick.

--world-arena-spread S (with --batched): a randomised band -- each episode's REAL world gets its own box mass, box ground
friction and robot-box friction, the nominal value times a factor drawn from [1 - S, 1 + S] (world_arena_of; the config key
`world_point_scene`); the planners keep the nominal arena.  0 (default): the runs as without the option, byte for byte.

--size default: the reference's shipped planner size, K=200 samples, T=15 (config/mppi/point.yaml) -- the size the
logged runs were most plausibly made with (it is not recorded); baseline (default here): K, T of the BASELINE configs.

The reference's runs differ from each other through PhysX's own non-determinism, its unseeded per-shape torsion
friction (isaacgym_wrapper.py:318) and the asynchronous RPC loop; this build is deterministic, so the spread is
produced by what plausibly varied there: the phase of the dyn-obs walk at the moment the task starts (0..99 ticks of
its 100-tick period) and +-5 cm on the start positions of box and robot.
tests/test_behaviour_band_gpu.py asserts on the output of `episodes()`.
"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SCENARIOS = {
    # scenario of the log -> overrides of config_point (reactive_tamp.py:11-16 command lines); K, T of BASELINE configs
    "case2_halton_push_coll": ["task=push", "goal=[-3,3]", "mppi.num_samples=2000", "mppi.horizon=30"],
    "case2_halton_pull_coll": ["task=pull", "goal=[-3,3]", "mppi.num_samples=2000", "mppi.horizon=30"],
    "corner1_push": ["task=push", "goal=[-3.75,-3.75]", "mppi.num_samples=2000", "mppi.horizon=30"],
    "corner1_pull": ["task=pull", "goal=[-3.75,-3.75]", "mppi.num_samples=2000", "mppi.horizon=30"],
    "corner1_hybrid": ["task=push_pull", "multi_modal=True", "goal=[-3.75,-3.75]", "mppi.num_samples=4000", "mppi.horizon=30"],
    # corner2_*: the box STARTS in the far corner (BOX_START below) and has to go to the opposite one
    "corner2_push": ["task=push", "goal=[-3.75,-3.75]", "mppi.num_samples=2000", "mppi.horizon=30"],
    "corner2_pull": ["task=pull", "goal=[-3.75,-3.75]", "mppi.num_samples=2000", "mppi.horizon=30"],
    "corner2_hybrid": ["task=push_pull", "multi_modal=True", "goal=[-3.75,-3.75]", "mppi.num_samples=4000", "mppi.horizon=30"],
}

# Where the box starts when it is not the scene's default (0, 2).  The logs hold final states only; corner2_push.npy tells the
# start: 6 of its 20 runs end with the box at (3.70, 3.70) -- 10.54 m from the goal, never moved --, 11 with it pushed down the
# wall into the next corner (3.70, -3.72), 3 succeed.  The box is 0.4 m wide and the walls' faces are at +-3.95 minus a
# contact offset: flush in the corner its centre is at 3.70.
BOX_START = {"corner2_push": (3.70, 3.70), "corner2_pull": (3.70, 3.70), "corner2_hybrid": (3.70, 3.70)}


SETTLE_TICKS = 0       # the final error is taken AT the success tick.  (The reference's logs were written after the run;
                       # with closed_loop.run(settle_ticks=20) -- 1 s of the zero action the planner side returns once the
                       # task is done -- this build's box coasts on: it is pushed 2-3x faster than in the logged runs and
                       # ends flush in the corner / up to 0.2 m past a free-standing goal: DESIGN.md section 2.)


def jitter_of(scenario, episode):
    """Deterministic per (scenario, episode); episode 0 is the unjittered reference scene."""
    start = BOX_START.get(scenario)
    if episode == 0:
        return dict(dyn_phase=0, box=(0.0, 0.0), robot=(0.0, 0.0), box_start=start)
    # (the scenario's index in the list of round 5 for the five scenarios of round 5: their episodes keep their jitter)
    order = sorted(k for k in SCENARIOS if not k.startswith("corner2")) + sorted(k for k in SCENARIOS if k.startswith("corner2"))
    rng = np.random.default_rng([order.index(scenario), episode])
    j = dict(dyn_phase=int(rng.integers(0, 100)), box=tuple(rng.uniform(-0.05, 0.05, 2).tolist()),
             robot=tuple(rng.uniform(-0.05, 0.05, 2).tolist()), box_start=start)
    if start is not None:      # a box flush in a corner can only be displaced INTO the arena
        j["box"] = tuple(float(-abs(d) * np.sign(c)) for d, c in zip(j["box"], start))
    return j


def world_arena_of(scenario, episode, spread):
    """--world-arena-spread: the `world_point_scene` overrides of an episode, or None (spread 0, and episode 0: the nominal
    world).  Factors in [1 - spread, 1 + spread] for box_m, box_mu_g and mu_rb from the episode's jitter seed (its own stream:
    the jitter's draws are what they were); box_I scales with box_m."""
    if not spread or episode == 0:
        return None
    if not 0.0 < spread < 1.0:
        raise ValueError("--world-arena-spread: a share in [0, 1)")
    from m3p2i_aip_amd._lib import POINT_SCENE_DEFAULTS as D
    order = sorted(k for k in SCENARIOS if not k.startswith("corner2")) + sorted(k for k in SCENARIOS if k.startswith("corner2"))
    rng = np.random.default_rng([order.index(scenario), episode, 1])
    fm, fg, fr = (float(f) for f in rng.uniform(1.0 - spread, 1.0 + spread, 3))
    return dict(box_m=D["box_m"] * fm, box_I=D["box_I"] * fm, box_mu_g=D["box_mu_g"] * fg, mu_rb=D["mu_rb"] * fr)


def batched_episode_list(pairs, n=20, world_arena_spread=0.0, extra=()):
    """What band_batched runs: [(scenario, size, episode, jitter)] and the [(config name, overrides, jitter)] of
    run_point_episodes, in the same order.  extra: overrides of every episode (POINT_RUNTIME_KEYS)."""
    items = [(sc, size, e, jitter_of(sc, e)) for sc, size in pairs for e in range(n)]
    eps = []
    for sc, size, e, j in items:
        ov = overrides(sc, size) + list(extra)
        arena = world_arena_of(sc, e, world_arena_spread)
        if arena:
            ov.append("world_point_scene={" + ", ".join(f"{k}: {v!r}" for k, v in arena.items()) + "}")
        eps.append(("config_point", ov, j))
    return items, eps


def fisher_one_sided(a, b, c, d, alternative="less"):
    """One-sided Fisher exact test of the 2x2 table [[a, b], [c, d]] (rows: this build, the logged runs; columns: event,
    no event): the probability, with all margins fixed, of a top-left count <= a ("less") or >= a ("greater")."""
    r1, c1, n = a + b, a + c, a + b + c + d
    lo, hi = max(0, r1 + c1 - n), min(r1, c1)
    tot = math.comb(n, r1)
    xs = range(lo, a + 1) if alternative == "less" else range(a, hi + 1)
    return sum(math.comb(c1, x) * math.comb(n - c1, r1 - x) for x in xs) / tot


def stats(x):
    x = np.asarray(x, np.float64)
    return {"mean": float(x.mean()), "std": float(x.std()), "min": float(x.min()), "max": float(x.max()), "n": int(x.size)}


AVOID = False      # --avoid: the extension `avoid_dyn_obs=True` (push / pull with get_motion_cost; cost_functions.Objective)


def overrides(scenario, size="baseline"):
    ov = list(SCENARIOS[scenario]) + (["avoid_dyn_obs=True"] if AVOID else [])
    if size == "default":      # config/mppi/point.yaml: 200 samples, horizon 15 (400 / 15 multi-modal: 200 per mode)
        mm = "multi_modal=True" in ov
        ov = [o for o in ov if not o.startswith("mppi.")] + [f"mppi.num_samples={400 if mm else 200}", "mppi.horizon=15"]
    return ov


def episodes(scenario, n=20, max_sim_time_s=40.0, size="baseline"):
    import closed_loop
    runs = []
    for e in range(n):
        j = jitter_of(scenario, e)
        r = closed_loop.run("config_point", overrides(scenario, size), ticks=int(max_sim_time_s / 0.05), jitter=j,
                            settle_ticks=SETTLE_TICKS)
        runs.append(dict(episode=e, jitter=j, success=r["success"], final_pos_error_m=r["final_pos_error"],
                         task_time_s=r["sim_time_s"], dyn_obs_collision_ticks=r["dyn_obs_collision_ticks"],
                         command_ms_p50=r["command_ms_p50"]))
    ok = [r for r in runs if r["success"]]
    return dict(scenario=scenario, n=n, size=size, overrides=overrides(scenario, size), successes=len(ok),
                final_pos_error_m=stats([r["final_pos_error_m"] for r in ok]) if ok else None,
                task_time_s=stats([r["task_time_s"] for r in ok]) if ok else None,
                dyn_obs_collided_episodes=int(sum(r["dyn_obs_collision_ticks"] > 0 for r in runs)),
                dyn_obs_collision_ticks=stats([r["dyn_obs_collision_ticks"] for r in runs]),
                command_ms_p50=stats([r["command_ms_p50"] for r in runs]), runs=runs)


def _summary(scenario, n, size, runs):
    ok = [r for r in runs if r["success"]]
    return dict(scenario=scenario, n=n, size=size, overrides=overrides(scenario, size), successes=len(ok),
                final_pos_error_m=stats([r["final_pos_error_m"] for r in ok]) if ok else None,
                task_time_s=stats([r["task_time_s"] for r in ok]) if ok else None,
                dyn_obs_collided_episodes=int(sum(r["dyn_obs_collision_ticks"] > 0 for r in runs)),
                dyn_obs_collision_ticks=stats([r["dyn_obs_collision_ticks"] for r in runs]),
                command_ms_p50=stats([r["command_ms_p50"] for r in runs]), runs=runs)


def band_batched(pairs, n=20, max_sim_time_s=40.0, world_arena_spread=0.0, extra=(), runtime=False, priors=False):
    """episodes() of every (scenario, size) in `pairs` at once: all n * len(pairs) episodes in lockstep
    (m3p2i_aip_amd.episodes.run_point_episodes).  Returns {(scenario, size): the dict episodes() returns}; each run's
    command_ms_p50 is the set's tick time.  runtime: the set created for planners with an arena per sample (point_runtime=True),
    which takes `rollout_arena_spread` among the `extra` overrides of every episode.  priors: the set created for planners with
    prior samples (point_priors=True), which takes `prior_samples={controller: ..., n: 4, device: true}` among them."""
    from m3p2i_aip_amd.episodes import run_point_episodes
    items, eps = batched_episode_list(pairs, n, world_arena_spread, extra)
    reps = run_point_episodes(eps, max_ticks=int(max_sim_time_s / 0.05), point_runtime=bool(runtime), point_priors=bool(priors))
    out = {}
    for (sc, size, e, j), r in zip(items, reps):
        out.setdefault((sc, size), []).append(dict(episode=e, jitter=j, success=r["success"], final_pos_error_m=r["final_pos_error"],
                                                   task_time_s=r["sim_time_s"], dyn_obs_collision_ticks=r["dyn_obs_collision_ticks"],
                                                   command_ms_p50=r["tick_ms_p50"]))
    return {k: _summary(k[0], n, k[1], runs) for k, runs in out.items()}


def episodes_batched(scenario, n=20, max_sim_time_s=40.0, size="baseline"):
    """episodes() with the n episodes in lockstep: the same dict, the same per-episode results (SETTLE_TICKS = 0)."""
    if SETTLE_TICKS:
        raise ValueError("episodes_batched: the batched runner takes the final error at the success tick (SETTLE_TICKS = 0)")
    return band_batched([(scenario, size)], n, max_sim_time_s)[(scenario, size)]


# config keys `panda` takes as overrides on the command line (e.g. 'world_panda_scene={cube_m: 0.2}'); batched: with --runtime
PANDA_RUNTIME_KEYS = ("panda_scene", "world_panda_scene", "panda_cost_weights", "rollout_workspace_spread")
# config keys the point scenarios take as overrides on the command line ('rollout_arena_spread={spread: 0.3, seed: 1}': an arena
# per sample of every planner); with --batched --runtime only (the lockstep set created for such planners)
POINT_RUNTIME_KEYS = ("rollout_arena_spread",)
# 'prior_samples={controller: push_behind, n: 4, device: true}': prior samples from a controller on the device for every planner;
# with --batched --priors only (the lockstep set created for such planners)
POINT_PRIORS_KEYS = ("prior_samples",)


def panda_episodes(n=20, overrides=("mppi.num_samples=4000", "mppi.horizon=20"), ticks=600):
    """Panda reactive pick-and-place (config_panda), cubeA's start jittered by +-2 cm (episode 0: the reference scene)."""
    import closed_loop
    runs = []
    for e in range(n):
        rng = np.random.default_rng([77, e])
        j = dict(cube=(0.0, 0.0) if e == 0 else tuple(rng.uniform(-0.02, 0.02, 2).tolist()))
        r = closed_loop.run("config_panda", list(overrides), ticks=ticks, jitter=j, settle_ticks=SETTLE_TICKS)
        runs.append(dict(episode=e, jitter=j, success=r["success"], ticks=r["ticks"], timeline=r["timeline"],
                         cube_to_goal_xy=r["cube_to_goal_xy"], cube_height_above_goal=r["cube_height_above_goal"]))
    ok = [r for r in runs if r["success"]]
    return dict(n=n, overrides=list(overrides), successes=len(ok),
                final_xy_error_m=stats([r["cube_to_goal_xy"] for r in ok]) if ok else None,
                ticks_to_success=stats([r["ticks"] for r in ok]) if ok else None, runs=runs)


def panda_episodes_batched(n=20, overrides=("mppi.num_samples=4000", "mppi.horizon=20"), ticks=600, runtime=False):
    """panda_episodes() with the n episodes in lockstep (m3p2i_aip_amd.episodes.run_panda_episodes): the same
    dict, the same per-episode results bit for bit.  runtime: the run-time set (panda_runtime=True), which takes `panda_scene`,
    `world_panda_scene`, `panda_cost_weights` and `rollout_workspace_spread` among the overrides."""
    from m3p2i_aip_amd.episodes import run_panda_episodes
    jit = []
    for e in range(n):
        rng = np.random.default_rng([77, e])
        jit.append(dict(cube=(0.0, 0.0) if e == 0 else tuple(rng.uniform(-0.02, 0.02, 2).tolist())))
    reps = run_panda_episodes([("config_panda", list(overrides), j) for j in jit], max_ticks=ticks, settle_ticks=SETTLE_TICKS,
                              panda_runtime=bool(runtime))
    runs = [dict(episode=e, jitter=j, success=r["success"], ticks=r["ticks"], timeline=r["timeline"],
                 cube_to_goal_xy=r["cube_to_goal_xy"], cube_height_above_goal=r["cube_height_above_goal"])
            for e, (j, r) in enumerate(zip(jit, reps))]
    ok = [r for r in runs if r["success"]]
    return dict(n=n, overrides=list(overrides), successes=len(ok),
                final_xy_error_m=stats([r["cube_to_goal_xy"] for r in ok]) if ok else None,
                ticks_to_success=stats([r["ticks"] for r in ok]) if ok else None, runs=runs)


def main(argv):
    n, out, names, size, batched, spread, runtime, extra, point_extra = 20, None, [], "baseline", False, 0.0, False, [], []
    priors, prior_extra = False, []
    it = iter(argv)
    for a in it:
        if a == "--batched":
            batched = True
        elif a == "--runtime":
            runtime = True
        elif a == "--priors":
            priors = True
        elif a.split("=", 1)[0] in POINT_PRIORS_KEYS and "=" in a:
            prior_extra.append(a)
        elif a.split("=", 1)[0] in PANDA_RUNTIME_KEYS and "=" in a:
            extra.append(a)
        elif a.split("=", 1)[0] in POINT_RUNTIME_KEYS and "=" in a:
            point_extra.append(a)
        elif a == "--n":
            n = int(next(it))
        elif a == "--json":
            out = next(it)
        elif a == "--size":
            size = next(it)
        elif a == "--world-arena-spread":
            spread = float(next(it))
        elif a == "--avoid":
            global AVOID
            AVOID = True
        else:
            names.append(a)
    if spread and not batched:
        raise SystemExit("--world-arena-spread: with --batched (the serial runs keep the nominal world)")
    if runtime and not batched:
        raise SystemExit("--runtime: with --batched (the run-time sets of the lockstep episodes)")
    if point_extra and not (batched and runtime):
        raise SystemExit(f"{point_extra[0].split('=', 1)[0]}: with --batched --runtime only (the serial runs: tools/rollout_scenes_bench.py)")
    if (priors or prior_extra) and not (batched and priors):
        raise SystemExit("--priors / prior_samples=...: with --batched --priors only (the serial runs: tools/prior_samples_bench.py)")
    if extra and batched and not runtime:
        raise SystemExit(f"{extra[0].split('=', 1)[0]}: with --batched, the run-time set only (--runtime)")
    allband = json.load(open(os.path.join(ROOT, "tests", "golden", "behaviour_band.json")))
    band = allband["point"]
    res = {}
    if "panda" in names:
        names.remove("panda")
        for tag, ov in (("panda_pick", ["mppi.num_samples=4000", "mppi.horizon=20"]),
                        ("panda_pick_faure", ["mppi.num_samples=4000", "mppi.horizon=20", "mppi.halton_scramble=faure"]),
                        ("panda_pick_default_size", ["mppi.num_samples=200", "mppi.horizon=12"]),
                        ("panda_pick_default_size_faure", ["mppi.num_samples=200", "mppi.horizon=12", "mppi.halton_scramble=faure"])):
            ov = ov + extra
            r = panda_episodes_batched(n, ov, runtime=runtime) if batched else panda_episodes(n, ov)
            r["logged"] = allband["panda"]["reactive_pick"]["final_xy_error_m"]
            res[tag] = r
            e = r["final_xy_error_m"]
            print(f"{tag}: {r['successes']}/{n} ok; xy err " + (f"{e['mean']:.4f}+-{e['std']:.4f}" if e else "-") +
                  f" (logged {r['logged']['mean']:.4f}+-{r['logged']['std']:.4f}); ticks " +
                  (f"{r['ticks_to_success']['mean']:.0f}+-{r['ticks_to_success']['std']:.0f}" if e else "-"), flush=True)
        if not names:
            if out:
                json.dump(res, open(out, "w"), indent=1)
            return
    pre = band_batched([(sc, size) for sc in names or list(SCENARIOS)], n, world_arena_spread=spread, extra=point_extra + prior_extra,
                       runtime=runtime, priors=priors) if batched else {}
    for sc in names or list(SCENARIOS):
        r = pre[(sc, size)] if batched else episodes(sc, n, size=size)
        r["logged"] = {k: band[sc][k] for k in ("final_pos_error_m", "task_time_s", "dyn_obs_collisions")}
        res[sc] = r
        lg = r["logged"]
        print(f"{sc} [{size}]: {r['successes']}/{n} ok; err {r['final_pos_error_m']['mean']:.3f}+-{r['final_pos_error_m']['std']:.3f} "
              f"(logged {lg['final_pos_error_m']['mean']:.3f}+-{lg['final_pos_error_m']['std']:.3f}); "
              f"time {r['task_time_s']['mean']:.2f}+-{r['task_time_s']['std']:.2f} s (median {np.median([q['task_time_s'] for q in r['runs']]):.2f}) "
              f"(logged {lg['task_time_s']['mean']:.2f}+-{lg['task_time_s']['std']:.2f}); "
              f"dyn-obs collided in {r['dyn_obs_collided_episodes']}/{n} episodes "
              f"(logged {lg['dyn_obs_collisions']['mean'] * lg['dyn_obs_collisions']['n']:.0f}/{lg['dyn_obs_collisions']['n']})", flush=True)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
