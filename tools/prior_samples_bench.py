"""What prior samples (m3_set_prior_samples) cost and what they buy.

Part 1, the cost: push, K = 2000, T = 30, ms per command on ONE handle, the arms interleaved in one process:
  (a) the untouched handle, (b) the same handle with m3_set_point_scene_instance(h, 1) -- the build the prior kernels twin --,
  (c) n = 1, 8, 64 and 256 priors.  Bar: (c) at most 5 % above (b).
Part 2, the benefit: closed loop (tools/closed_loop.run) at the reference's shipped size (K = 200, T = 15) and at K = 32, push and
  navigation, jittered episodes in three arms interleaved on the same seeds -- no priors, `prior_samples={controller: ..., n: 4}`
  (the numpy controller, uploaded every tick) and the same key with `device: true` (the controller kernel, set once): success count,
  task time, final error, the host's ms per command.  Condition: the device arm's host ms per command below the host arm's.

Part 3 (not part of `all`): the rows of part 2 at N = 60 per row in lockstep, no priors against the device controller.

    python tools/prior_samples_bench.py [--part 1|2|3|all] [--rounds 7] [--commands 200] [--episodes 20] [--ticks 400]
                                        [--out profiles/prior_samples_bench.json]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd import priors  # noqa: E402
from m3p2i_aip_amd.engine import HipEngine, make_config  # noqa: E402


def _noise(K, T, seed):
    g = torch.Generator().manual_seed(seed)
    knots = torch.randn(K, 2, max(T // 4, 2), generator=g)
    return torch.nn.functional.interpolate(knots, size=T, mode="linear", align_corners=True).permute(0, 2, 1).contiguous().numpy()


def cost(rounds, commands, warmup=20):
    K, T = 2000, 30
    eng = HipEngine(make_config(K=K, T=T, nu=2, u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3]))
    eng.set_objective("push", (-1.0, -1.0))
    eng.set_noise(_noise(K, T, 1))
    world = np.zeros(18, np.float32)
    world[0:2] = (0.2, 0.5); world[4:7] = (0.1, 2.0, 1.0); world[11:14] = (-2.0, 2.0, 1.0)
    robot, box, goal = world[0:2], world[4:6], (-1.0, -1.0)
    arms = [("untouched", -1, 0), ("scene_instance_1", 1, 0)] + [(f"priors_{n}", -1, n) for n in (1, 8, 64, 256)]
    ms = {name: [] for name, _, _ in arms}
    plans = {}
    try:
        for r in range(rounds + 1):           # (round 0 warms every arm's kernel up and is dropped)
            for name, inst, n in arms:
                eng.set_point_scene_instance(inst)
                if n:
                    speeds = [1.0 - 0.9 * j / max(n - 1, 1) for j in range(n)]
                    eng.set_prior_samples(priors.push_behind(robot, box, goal, T, 0.05, [3.0, 3.0], speeds), list(range(n)))
                else:
                    eng.set_prior_samples(None)
                eng.reset()
                eng.set_world_point_raw(world)
                for _ in range(warmup):
                    eng.command()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(commands):
                    eng.command()
                e1.record()
                torch.cuda.synchronize()
                plans[name] = dict(priors_used=eng.prior_samples_used(), form=eng.point_rollout_form_used())
                if r:
                    ms[name].append(e0.elapsed_time(e1) / commands)
    finally:
        eng.close()
    out = {name: dict(ms_median=float(np.median(v)), ms_min=float(np.min(v)), ms_max=float(np.max(v)), rounds=len(v), **plans[name])
           for name, v in ms.items()}
    b = out["scene_instance_1"]["ms_median"]
    for name in out:
        out[name]["vs_scene_instance_1"] = out[name]["ms_median"] / b
    out["bar"] = dict(text="every priors_n at most 5 % above scene_instance_1",
                      met=all(out[f"priors_{n}"]["vs_scene_instance_1"] <= 1.05 for n in (1, 8, 64, 256)))
    return dict(K=K, T=T, task="push", commands_per_block=commands, device=torch.cuda.get_device_name(0), build_id=_build_id(), arms=out)


def _build_id():
    try:
        lib = L.load()
        lib.m3_build_id.restype = __import__("ctypes").c_char_p
        return lib.m3_build_id().decode()
    except Exception:
        return None


def _jitters(n):
    """the n jittered starts every row runs on (seeded: the first draws are the same for every n)"""
    rng = np.random.default_rng(0)
    return [dict(dyn_phase=int(rng.integers(0, 100)), box=tuple(rng.uniform(-0.05, 0.05, 2).tolist()),
                 robot=tuple(rng.uniform(-0.05, 0.05, 2).tolist())) for _ in range(n)]


ARMS = ("none", "host", "device")   # no priors | the numpy controller, uploaded every tick | the controller kernel (device: true)


def benefit(episodes, ticks):
    """Per row (K, task) the three arms INTERLEAVED episode by episode, on the same jitter seeds."""
    import closed_loop
    jit = _jitters(episodes)
    rows = []
    for K, T in ((200, 15), (32, 15)):
        for task, controller in (("push", "push_behind"), ("navigation", "go_to")):
            base = [f"task={task}", f"mppi.num_samples={K}", f"mppi.horizon={T}", f"mppi.u_per_command={T}"]
            key = {"none": [], "host": ["prior_samples={controller: %s, n: 4}" % controller],
                   "device": ["prior_samples={controller: %s, n: 4, device: true}" % controller]}
            res = {arm: [] for arm in ARMS}
            for j in jit:
                for arm in ARMS:
                    res[arm].append(closed_loop.run("config_point", base + key[arm], ticks=ticks, jitter=j))
            for arm in ARMS:
                ok = [r for r in res[arm] if r["success"]]
                rows.append(dict(K=K, T=T, task=task, priors=None if arm == "none" else controller, arm=arm, episodes=episodes,
                                 successes=len(ok), max_ticks=ticks,
                                 task_time_s_median=float(np.median([r["sim_time_s"] for r in ok])) if ok else None,
                                 final_pos_error_median=float(np.median([r["final_pos_error"] for r in res[arm]])),
                                 command_ms_p50_median=float(np.median([r["command_ms_p50"] for r in res[arm]]))))
                print(json.dumps(rows[-1]), flush=True)
            h, d, n0 = (rows[-3 + ARMS.index(a)]["command_ms_p50_median"] for a in ("host", "device", "none"))
            rows.append(dict(K=K, T=T, task=task, condition="device arm's host ms per command below the host-controller arm's",
                             met=bool(d < h), device_ms=d, host_ms=h, none_ms=n0, device_minus_none_ms=d - n0))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def lockstep_rows(n=60, ticks=400):
    """Part 3: the rows of part 2 with N = n episodes per row in LOCKSTEP (m3p2i_aip_amd.episodes.run_point_episodes with
    point_priors=True), no priors against the device controller, on the first n draws of part 2's jitter seed."""
    from m3p2i_aip_amd.episodes import run_point_episodes
    jit = _jitters(n)
    rows = []
    for K, T in ((200, 15), (32, 15)):
        for task, controller in (("push", "push_behind"), ("navigation", "go_to")):
            base = [f"task={task}", f"mppi.num_samples={K}", f"mppi.horizon={T}", f"mppi.u_per_command={T}"]
            for arm, extra in (("none", []), ("device", ["prior_samples={controller: %s, n: 4, device: true}" % controller])):
                reps = run_point_episodes([("config_point", base + extra, j) for j in jit], max_ticks=ticks, point_priors=True)
                ok = [r for r in reps if r["success"]]
                rows.append(dict(K=K, T=T, task=task, arm=arm, controller=controller if extra else None, episodes=n, successes=len(ok),
                                 max_ticks=ticks, jitter_seed="default_rng(0), the first %d draws" % n,
                                 task_time_s_median=float(np.median([r["sim_time_s"] for r in ok])) if ok else None,
                                 task_time_s_mean=float(np.mean([r["sim_time_s"] for r in ok])) if ok else None,
                                 final_pos_error_median=float(np.median([r["final_pos_error"] for r in reps])),
                                 tick_ms_p50=reps[0]["tick_ms_p50"]))
                print(json.dumps(rows[-1]), flush=True)
    return rows


def main(argv):
    opt = dict(part="all", rounds=7, commands=200, episodes=20, ticks=400, out=os.path.join(ROOT, "profiles", "prior_samples_bench.json"))
    for i in range(0, len(argv) - 1, 2):
        key = argv[i].lstrip("-")
        opt[key] = type(opt[key])(argv[i + 1])
    res = {}
    if os.path.exists(opt["out"]):
        res = json.load(open(opt["out"]))
    if opt["part"] in ("1", "all"):
        res["cost"] = cost(opt["rounds"], opt["commands"])
        print(json.dumps(res["cost"], indent=1), flush=True)
    if opt["part"] in ("2", "all"):
        res["benefit"] = benefit(opt["episodes"], opt["ticks"])
        res["benefit_build_id"], res["benefit_device"] = _build_id(), torch.cuda.get_device_name(0)
    if opt["part"] == "3":
        res["lockstep_rows"] = lockstep_rows(60, opt["ticks"])
        res["lockstep_rows_build_id"] = _build_id()
    os.makedirs(os.path.dirname(opt["out"]), exist_ok=True)
    json.dump(res, open(opt["out"], "w"), indent=1)
    print("wrote", opt["out"])


if __name__ == "__main__":
    main(sys.argv[1:])
