"""What panda_env prior samples (m3_set_panda_prior_samples) cost and what they buy.

Part 1, the cost: K = 4000, T = 20, reach (the configured initial scene, gripper open) and pick (cubeA held, gripper closing), ms
per m3_command, one handle per arm, the arms interleaved in one process, `--rounds` rounds of `--commands` commands per arm after
a dropped warm-up round, median and range:
  (a) untouched  the handle as created: the literal kernels,
  (b) twin       both run-time instances forced on (m3_set_panda_scene_instance 1 + m3_set_panda_weighted_cost_instance 1):
                 k_rollout_panda_w, the construction the prior kernels are built from -- the yardstick,
  (c) priors_n   n = 1, 8, 64, 256 prior samples (priors.joint_go_to at n speed factors, samples 0 .. n - 1): k_rollout_panda_pr.
Bar: every (c) at most 5 % above (b), for pick and for reach.  Reported without a bar: (c) against (a), n = 256 against n = 1.
Part 2, the benefit: closed loop (tools/closed_loop.run) on config_panda at K = 200 and K = 32, `--episodes` jittered episodes per
row, the arms interleaved on the same seeds -- no priors, `panda_prior_samples={controller: hold, n: 4}` and a joint_go_to row
(towards the joints that put the finger tips 5 cm above cubeA's configured place): successes, task time, the host's ms per
command.  Reported as measured, with the episode count; no bar.

    python tools/panda_prior_samples_bench.py [--part 1|2|all] [--rounds 7] [--commands 200] [--episodes 3] [--ticks 600]
                                              [--out profiles/panda_prior_samples_bench.json]
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

K, T = 4000, 20
GOAL = (0.2, 0.2, 1.115, 0.0, 0.0, 0.0, 1.0)
UMIN, UMAX, SIG = [-2.0] * 7 + [-1.5] * 2, [2.0] * 7 + [1.5] * 2, [10.0] * 7 + [0.8] * 2
NS = (1, 8, 64, 256)


def _build_id():
    return L.load().m3_build_id().decode()


def _oracle():
    import oracle
    oracle.load()
    import oracle.panda as P
    return P


def cost(rounds, commands, warmup=10):
    from tests.panda_prior_samples_fixture import joints_that_reach
    from tests.panda_worlds import grasp_world
    P = _oracle()
    delta = np.random.default_rng(3).standard_normal((K, T, 9)).astype(np.float32)
    arms = [("untouched", 0), ("twin", 0)] + [(f"priors_{n}", n) for n in NS]
    rows = {}
    for task, grip in (("reach", 1), ("pick", 2)):
        w0 = P.init_world(1)[0] if task == "reach" else grasp_world(P, P.default_scene())
        q_target = joints_that_reach(P, w0[:9], GOAL[:3])
        engines = {}
        for name, n in arms:
            e = HipEngine(make_config(K=K, T=T, nu=9, env_type="panda_env", u_min=UMIN, u_max=UMAX, noise_sigma_diag=SIG, lambda_=0.05,
                                      pre_height_diff=0.05, dt=0.01))
            e.set_noise(delta)
            e.set_objective(task, GOAL, gripper_cmd=grip)
            if name == "twin":
                e.set_panda_scene_instance(1)
                e.set_panda_weighted_cost_instance(1)
            if n:
                speeds = [1.0 - 0.9 * j / max(n - 1, 1) for j in range(n)]
                e.set_panda_prior_samples(priors.joint_go_to(w0[:9], q_target, T, 0.01, UMAX, speeds), list(range(n)))
            e.set_world_panda_raw(P.raw57(w0))
            engines[name] = e
        ms = {name: [] for name, _ in arms}
        try:
            for r in range(rounds + 1):           # (round 0 warms every arm's kernel up and is dropped)
                for name, _ in arms:
                    e = engines[name]
                    e.reset()                     # (the priors survive it)
                    for _ in range(warmup):
                        e.command()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(commands):
                        e.command()
                    e1.record()
                    e1.synchronize()
                    if r:
                        ms[name].append(e0.elapsed_time(e1) / commands)
            launch = {name: dict(priors_used=e.panda_prior_samples_used(), scene=int(e.panda_scene_instance_used()),
                                 weighted=int(e.panda_weighted_cost_instance_used()), lanes_per_sample=e.panda_lanes_per_sample_used())
                      for name, e in engines.items()}
        finally:
            for e in engines.values():
                e.close()
        out = {name: dict(ms_median=float(np.median(v)), ms_min=float(np.min(v)), ms_max=float(np.max(v)), rounds=len(v), **launch[name])
               for name, v in ms.items()}
        for name in out:
            out[name]["vs_twin"] = out[name]["ms_median"] / out["twin"]["ms_median"]
            out[name]["vs_untouched"] = out[name]["ms_median"] / out["untouched"]["ms_median"]
        out["priors_256_vs_priors_1"] = out["priors_256"]["ms_median"] / out["priors_1"]["ms_median"]
        out["bar"] = dict(text="every priors_n at most 5 % above twin", met=all(out[f"priors_{n}"]["vs_twin"] <= 1.05 for n in NS))
        rows[task] = out
    return dict(K=K, T=T, commands_per_block=commands, device=torch.cuda.get_device_name(0), build_id=_build_id(), tasks=rows)


ARMS = ("none", "hold", "joint_go_to")


def benefit(episodes, ticks):
    """Per K the three arms INTERLEAVED episode by episode, on the same jitter seeds."""
    import closed_loop
    from tests.panda_prior_samples_fixture import joints_that_reach
    P = _oracle()
    w0 = P.init_world(1)[0]
    above = np.asarray(w0[P.W_CUBEA:P.W_CUBEA + 3], np.float64) + (0.0, 0.0, 0.05)
    q = [round(float(x), 4) for x in joints_that_reach(P, w0[:9], above)]
    rng = np.random.default_rng(0)
    jit = [dict(cube=tuple(rng.uniform(-0.03, 0.03, 2).tolist())) for _ in range(episodes)]
    key = {"none": [], "hold": ["panda_prior_samples={controller: hold, n: 4}"],
           "joint_go_to": ["panda_prior_samples={controller: joint_go_to, n: 4, q: %s}" % q]}
    rows = []
    for Ks in (200, 32):
        base = [f"mppi.num_samples={Ks}"]
        res = {arm: [] for arm in ARMS}
        for j in jit:
            for arm in ARMS:
                res[arm].append(closed_loop.run("config_panda", base + key[arm], ticks=ticks, jitter=j))
        for arm in ARMS:
            ok = [r for r in res[arm] if r["success"]]
            rows.append(dict(K=Ks, arm=arm, key=key[arm], episodes=episodes, successes=len(ok), max_ticks=ticks,
                             task_time_s_median=float(np.median([r["sim_time_s"] for r in ok])) if ok else None,
                             command_ms_p50_median=float(np.median([r["command_ms_p50"] for r in res[arm]]))))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main(argv):
    opt = dict(part="all", rounds=7, commands=200, episodes=3, ticks=600, out=os.path.join(ROOT, "profiles", "panda_prior_samples_bench.json"))
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
    os.makedirs(os.path.dirname(opt["out"]), exist_ok=True)
    json.dump(res, open(opt["out"], "w"), indent=1)
    print("wrote", opt["out"])


if __name__ == "__main__":
    main(sys.argv[1:])
