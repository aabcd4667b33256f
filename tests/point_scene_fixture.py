"""Shared inputs of the run-time point scene tests (tests/test_point_scene_cpu.py, tests/test_point_scene_gpu.py): the custom
arena, the three start worlds and the actions; the oracle's results on them, computed once per process and never modified."""
import functools

import numpy as np

from m3p2i_aip_amd import _lib as L

F = np.float32
FIELDS = list(L.POINT_SCENE_DEFAULTS)
# the default arena with a moved, smaller obstacle, a smaller room, an oblong heavier box with other frictions, a larger robot
CUSTOM = dict(obs_x=-1.0, obs_y=0.5, obs_hx=0.25, obs_hy=0.1, wall=1.5, box_hx=0.3, box_hy=0.15, box_m=9.0,
              box_I=9.0 * (0.6 ** 2 + 0.3 ** 2) / 12.0, mu_rb=0.4, box_mu_g=0.6, robot_r=0.25)
# a second custom arena (batch test: two scenes in one launch)
CUSTOM_B = dict(obs_x=0.6, obs_y=0.9, obs_hx=0.1, obs_hy=0.3, wall=2.0, dyn_hx=0.15, dyn_hy=0.3, dyn_m=9.0,
                dyn_I=9.0 * (0.3 ** 2 + 0.6 ** 2) / 12.0, mu_rd=0.3, mu_ro=0.2, robot_m=8.0)
K, T, GOAL = 64, 8, (1.0, 1.0)
WORLD_NAMES = ["at_obstacle", "at_walls", "at_box"]


def scene_dict(overrides=None):
    return {**L.POINT_SCENE_DEFAULTS, **(overrides or {})}


def scene_array(overrides=None):
    d = scene_dict(overrides)
    return np.array([d[n] for n in FIELDS], F)


def oracle_scene(O, overrides=None, dt=0.05, substeps=2, iters=6):
    sc = O.default_scene()
    for n, v in (overrides or {}).items():
        setattr(sc, n, float(v))
    sc.dt, sc.substeps, sc.iters = dt, substeps, iters
    return sc


def start_worlds(O):
    """the three start worlds: the robot at the moved obstacle; robot, box and dyn-obs at the (smaller room's) walls; the
    robot at the box"""
    w = O.init_world(3)
    w[0, 0:2] = (-0.6, 0.5)
    w[1, 0:2] = (1.2, -1.2); w[1, O.W_B:O.W_B + 2] = (1.1, 1.0); w[1, O.W_D:O.W_D + 2] = (-1.1, -1.1)
    w[2, 0:2] = (0.0, 0.0); w[2, O.W_B:O.W_B + 2] = (0.45, 0.0); w[2, O.W_D:O.W_D + 2] = (3.0, 3.0)
    return w.astype(F)


def actions(k=K, t=T):
    return (np.random.default_rng(1).standard_normal((k, t, 2)) * 1.5).astype(F)


@functools.lru_cache(maxsize=None)
def oracle_rollout(task, world, custom, k=K):
    """oracle.point_rollout of start world `world` under the custom (True) / default (False) arena: dict of read-only arrays.
    The actions are the scaled controls themselves (u_scale 1, no clamping in reach: |a| < 3 is not guaranteed, so the cfg's
    bounds are wide)."""
    import oracle as O
    mm = task == "push_pull"
    cfg = O.make_cfg(k, T, task=task, goal=GOAL, multi_modal=mm, u_min=[-100.0] * 2, u_max=[100.0] * 2)
    sc = oracle_scene(O, CUSTOM if custom else None)
    out = O.point_rollout(cfg, sc, start_worlds(O)[world], actions(k))
    for a in out.values():
        a.setflags(write=False)
    return out


def changed_share(task, world, k=K):
    """share of the samples whose robot states differ between the two arenas, on the oracle alone"""
    a, b = oracle_rollout(task, world, True, k)["states"], oracle_rollout(task, world, False, k)["states"]
    return float((a.view(np.uint32) != b.view(np.uint32)).reshape(len(a), -1).any(1).mean())
