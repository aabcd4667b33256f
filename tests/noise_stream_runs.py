"""The runs tests/test_noise_stream_gpu.py repeats to pin determinism (a helper, not a test): a configuration by name, six
commands on a fresh handle, every buffer of every call.  `python -m tests.noise_stream_runs NAME OUT.npz` is the same run
in a fresh process."""
import sys

import numpy as np

from tests.noise_stream_ref import NAVR_MU, NAVR_SIG, PANDA_DIAG

N_COMMANDS = 6
TORCH_SEED = 1234          # C1 draws its initial plan from torch's global generator (mppi.py:129-134; planner.py)
# the order a difference is reported in: the stream, then what the rollout wrote, then what the update wrote
BUFFERS = ("NOISE", "ACTIONS", "STATES", "COST_HORIZON", "TRAJ_COST", "WEIGHTS", "MEAN", "action")
CONFIGS = ("c1", "navr", "panda_simple")


def _snapshot(eng, L, action):
    out = {n: eng.buffer(getattr(L, "BUF_" + n)).cpu().numpy().copy() for n in BUFFERS[1:-1]}
    out["action"] = np.array(action.cpu().numpy() if hasattr(action, "cpu") else action, copy=True)
    return out


def run(name, torch_seed=TORCH_SEED):
    """-> (initial plan, [per command: {buffer name: array}])"""
    import torch
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipEngine, make_config
    calls = []
    if name == "c1":           # BASELINE C1, built exactly as bench.py builds it
        import bench
        env, task, goal, multi_modal, K, T = bench.CONFIGS["c1"]
        torch.manual_seed(torch_seed)
        pl, sim, obj, cfg = bench.build_tamp(env, task, goal, multi_modal, K, 0, 1, T, "cuda:0", simple="c1" in bench.SIMPLE_MODE)
        eng = pl._engine
        state = sim._dof_state[0]
        plan0 = eng.buffer(L.BUF_MEAN).cpu().numpy().copy()
        for _ in range(N_COMMANDS):
            noise = eng.sample_noise().cpu().numpy().copy()
            action = pl.command(state)
            torch.cuda.synchronize()
            calls.append(dict(NOISE=noise, **_snapshot(eng, L, action)))
        return plan0, calls
    if name == "navr":         # halton-spline + random, the opt_navr distribution
        eng = HipEngine(make_config(K=1000, T=20, nu=2, sampling_random=True, u_min=[-3, -3], u_max=[3, 3],
                                    noise_mu=NAVR_MU, noise_sigma=NAVR_SIG, lambda_=0.5, seed=7))
        eng.set_objective("navigation", (-3.0, 3.0))
    elif name == "panda_simple":
        eng = HipEngine(make_config(K=256, T=12, nu=9, env_type="panda_env", mode_simple=True, sampling_random=True,
                                    u_per_command=12, u_min=[-2.0] * 7 + [-1.5] * 2, u_max=[2.0] * 7 + [1.5] * 2,
                                    noise_sigma_diag=PANDA_DIAG, lambda_=0.05, pre_height_diff=0.05, dt=0.01,
                                    seed=7))
        eng.set_objective("reach", [0.2, 0.2, 1.115, 0.0, 0.0, 0.0, 1.0], gripper_cmd=1)
    else:
        raise KeyError(name)
    plan0 = eng.buffer(L.BUF_MEAN).cpu().numpy().copy()
    for _ in range(N_COMMANDS):
        noise = eng.sample_noise().cpu().numpy().copy()
        action = eng.command(sync_host=True)
        calls.append(dict(NOISE=noise, **_snapshot(eng, L, action)))
    eng.close()
    return plan0, calls


def first_difference(a, b):
    """(call, buffer) of the first buffer, in BUFFERS order within the earliest call, whose bytes differ -- or None."""
    for c, (x, y) in enumerate(zip(a, b)):
        for n in BUFFERS:
            if x[n].shape != y[n].shape or x[n].tobytes() != y[n].tobytes():
                return c, n
    return None


def save(path, plan0, calls):
    np.savez(path, plan0=plan0, **{"c%d_%s" % (c, n): v for c, d in enumerate(calls) for n, v in d.items()})


def load(path):
    z = np.load(path)
    return z["plan0"], [{n: z["c%d_%s" % (c, n)] for n in BUFFERS} for c in range(N_COMMANDS)]


if __name__ == "__main__":
    save(sys.argv[2], *run(sys.argv[1]))
