"""Probe workspaces of m3_set_panda_scene (include/m3p2i_hip.h), each with the world, task and gripper command it is tested
in, and what the CPU and GPU tests of the feature share: the oracle's scene of a probe, the oracle's rollout in it (computed
once per case and kept), and the SHARE of a probe -- the fraction of samples whose cost_horizon row differs between the
probe scene and the default scene on the oracle alone.  A test of a probe first asserts that share: a scene that changes
nothing would pass every comparison with the oracle while testing nothing.

The shares below were measured on the CPU oracle with delta = default_rng(1).standard_normal((64, 20, 9)), the goal
(0.2, 0.2, 1.115, 0, 0, 0, 1) and the worlds of random_panda_worlds(P, default scene, 42, default_rng(900)):

    field alone          value         world, task, gripper                      share
    table[2]             0.99          world 41, reach, 2                        1.00
    table[3]             0.25          world 36, reach, 2                        1.00
    shelf[0]             0.42          world 22, reach, 1                        0.92
    shelf[5]             0.12          init_world(cube_on_shelf=True), reach, 1  1.00   (0.16 gives 0)
    cube_m               0.4           world 40, pick, 2                         1.00
    obs_m                0.2           world 41, reach, 2                        1.00
    obs_half[0], [2]     0.16, 0.02    world 41, reach, 2                        1.00
    mu                   0.3           world 41, reach, 2                        1.00
    base[0], [2]         -0.40, 1.10   world 41, reach, 2                        1.00

COMBINED (all of them at once, table[3] = 0.45) over the 42 worlds with the task cycling FUZZ_TASKS[i % 4]: 31 worlds with a
share >= 0.8, 34 with >= 0.5, share 0 in worlds 1, 10, 37 and 38; every result finite."""
import functools

import numpy as np

GOAL = (0.2, 0.2, 1.115, 0.0, 0.0, 0.0, 1.0)
K, T = 64, 20
K_RAGGED = 61
STEP_ENVS, STEP_STEPS = 65, 25
FUZZ_TASKS = [("reach", 1), ("pick", 2), ("place", 1), ("reach", 2)]
UMIN = [-2.0] * 7 + [-1.5] * 2
UMAX = [2.0] * 7 + [1.5] * 2
SIG = [10.0] * 7 + [0.8] * 2

DEFAULTS = dict(base=(-0.45, 0.0, 1.125), table=(0.0, 0.0, 1.0, 0.6, 0.6, 0.025), shelf=(0.5, 0.0, 1.175, 0.1, 0.1, 0.15),
                obs_half=(0.1, 0.1, 0.01), obs_m=0.8, cube_m=0.125, mu=1.0)

# name -> (field overrides, world (index into the fuzz batch, or "shelf"), task, gripper command, the masses alone)
PROBES = {
    "table_z": (dict(table=(0.0, 0.0, 0.99, 0.6, 0.6, 0.025)), 41, "reach", 2, False),
    "table_hx": (dict(table=(0.0, 0.0, 1.0, 0.25, 0.6, 0.025)), 36, "reach", 2, False),
    "shelf_x": (dict(shelf=(0.42, 0.0, 1.175, 0.1, 0.1, 0.15)), 22, "reach", 1, False),
    "shelf_hz": (dict(shelf=(0.5, 0.0, 1.175, 0.1, 0.1, 0.12)), "shelf", "reach", 1, False),
    "cube_m": (dict(cube_m=0.4), 40, "pick", 2, True),
    "obs_m": (dict(obs_m=0.2), 41, "reach", 2, True),
    "obs_half": (dict(obs_half=(0.16, 0.1, 0.02)), 41, "reach", 2, False),
    "mu": (dict(mu=0.3), 41, "reach", 2, False),
    "base": (dict(base=(-0.40, 0.0, 1.10)), 41, "reach", 2, False),
}
COMBINED = dict(base=(-0.40, 0.0, 1.10), table=(0.0, 0.0, 0.99, 0.45, 0.6, 0.025), shelf=(0.42, 0.0, 1.175, 0.1, 0.1, 0.12),
                obs_half=(0.16, 0.1, 0.02), obs_m=0.2, cube_m=0.4, mu=0.3)
SCENES = {**{n: p[0] for n, p in PROBES.items()}, "COMBINED": COMBINED}


def full(fields):
    """all fields of a scene: the overrides over the defaults"""
    return {**DEFAULTS, **(fields or {})}


def flat21(fields):
    """the 21 floats of m3_panda_scene, in field order"""
    f = full(fields)
    return np.array(list(f["base"]) + list(f["table"]) + list(f["shelf"]) + list(f["obs_half"]) + [f["obs_m"], f["cube_m"], f["mu"]],
                    np.float32)


def oracle_scene(P, fields=None):
    """the oracle's scene (m3o_panda_scene) of a workspace"""
    sc = P.default_scene()
    f = full(fields)
    for name in ("base", "table", "shelf", "obs_half"):
        for i, v in enumerate(f[name]):
            getattr(sc, name)[i] = v
    sc.obs_m, sc.cube_m, sc.mu = f["obs_m"], f["cube_m"], f["mu"]
    return sc


@functools.lru_cache(maxsize=1)
def fuzz_worlds():
    import oracle.panda as P
    from tests.test_device_dynamics_on_host import random_panda_worlds
    w = random_panda_worlds(P, P.default_scene(), 42, np.random.default_rng(900))
    w.setflags(write=False)
    return w


def world_of(spec):
    import oracle.panda as P
    if spec == "shelf":
        return P.init_world(1, cube_on_shelf=True)[0].copy()
    return fuzz_worlds()[int(spec)].copy().astype(np.float32)


@functools.lru_cache(maxsize=4)
def delta_of(k):
    d = np.random.default_rng(1).standard_normal((k, T, 9)).astype(np.float32)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def oracle_rollout(scene_name, world_spec, task, grip, k=K):
    """the first command of an OraclePandaPlanner in the named scene (None: the default): actions, states, cost_h, J.
    Computed once per case; the arrays are read-only."""
    import oracle.panda as P
    cfg = P.make_cfg(k, T, multi_modal=False, task=task, goal=np.array(GOAL, np.float32), gripper_cmd=grip)
    opl = P.OraclePandaPlanner(cfg, delta_of(k), oracle_scene(P, SCENES[scene_name] if scene_name else None))
    opl.command(world_of(world_spec))
    out = {n: np.array(opl.last[n]) for n in ("actions", "states", "cost_h", "J")}
    for a in out.values():
        a.setflags(write=False)
    return out


def share(scene_name, world_spec, task, grip, k=K):
    """the fraction of samples whose cost_h row in the named scene differs from the default scene's (the oracle alone)"""
    a = oracle_rollout(scene_name, world_spec, task, grip, k)["cost_h"]
    b = oracle_rollout(None, world_spec, task, grip, k)["cost_h"]
    assert np.isfinite(a).all() and np.isfinite(b).all()
    return float((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).mean())


@functools.lru_cache(maxsize=1)
def combined_fuzz_shares():
    """COMBINED's share in each of the 42 fuzz worlds under its task of FUZZ_TASKS"""
    return tuple(share("COMBINED", i, *FUZZ_TASKS[i % 4]) for i in range(42))


def qualifying_fuzz_worlds():
    """the fuzz worlds in which COMBINED shows (share >= 0.5); the tests need at least 30 of the 42"""
    return [i for i, s in enumerate(combined_fuzz_shares()) if s >= 0.5]
