"""The reference of the per-sample panda_env workspaces (m3_set_panda_rollout_scenes): a STITCHED rollout
built from oracle calls only -- the oracle has one scene per call, so a rollout whose samples live in different workspaces is
put together from

  * `oracle.panda.rollout`'s assembled `actions` (the scaled controls; they do not depend on the scene),
  * `step_batch` per group of samples with equal scenes,
  * `observe` of every sample in its own row's scene,
  * `make_obs` with the `cube0` / `cube_q_half0` columns taken from rows 0 and K / 2 (quirk Q8 under per-sample workspaces: the
    cube of sample 0 as simulated in scenes[0], the orientation of sample K / 2 in scenes[K / 2]),
  * `cost_obs` (or tests/panda_cost_ref.py for tuned weights) and the rollout's own discount recurrence, in binary32.

tests/test_panda_scene_rows_cpu.py pins it: with all rows equal it reproduces `oracle.panda.rollout` bit for bit.  It also holds
the 5-cycles of workspaces the GPU cases use (row i = cycle[i % 5]; 5 is coprime to every samples-per-wavefront count of the
three kernel forms with and without shadow slots -- 3, 4, 8, 62, 63, 64 -- so a kernel that indexed the table by slot, lane or
wavefront cannot pass) and the guard that each pair of scenes of a cycle shows."""
import functools
import itertools

import numpy as np

from tests import panda_scene_fixture as X

F = np.float32
# name -> world, task, gripper command, the cycle's scenes (names of tests/panda_scene_fixture.py; None: the default workspace)
CYCLES = {
    "reach": (41, "reach", 2, (None, "table_z", "mu", "base", "obs_half")),
    "pick": (40, "pick", 2, (None, "cube_m", "mu", "table_z", "COMBINED")),
}


def fields_of(name):
    return None if name is None else X.SCENES[name]


def cycle_rows(cycle, n, offset=0):
    """the field overrides of rows offset .. offset + n - 1: row i = cycle[i % 5]"""
    names = CYCLES[cycle][3]
    return [fields_of(names[(offset + i) % len(names)]) for i in range(n)]


def groups_of(rows):
    """[(field overrides, indices)]: the rows with the same 21 floats"""
    by = {}
    for i, r in enumerate(rows):
        by.setdefault(X.flat21(r).tobytes(), (r, []))[1].append(i)
    return [(r, np.array(idx)) for r, idx in by.values()]


def stitched_rollout(P, cfg, task, rows, world0, act, k0=0, cost=None, keep_obs=False, scaled=False):
    """The rollout of samples k0 .. k0 + len(rows) - 1 with sample i in the workspace rows[i].  act: the assembled actions of
    those samples [n, T, 9] (scaled: the rollout's own `actions` output instead -- the controls as the steps receive them).
    cost: None = oracle.panda.cost_obs, else f(obs [n, 30], k [n]) -> [n] float32.  Returns states, actions, cost_h, J as
    oracle.panda.rollout does (and obs [T, n, 30] if asked)."""
    n, K, T = len(rows), cfg.K, cfg.T
    assert act.shape == (n, T, 9)
    # (scaled by u_scale; the null action of sample K - 1)
    u = np.array(act, F) if scaled else P.rollout(cfg, P.default_scene(), world0, act, k0, k0 + n)["actions"]
    groups = [(X.oracle_scene(P, r), idx) for r, idx in groups_of(rows)]
    scene_of = [None] * n
    for sc, idx in groups:
        for i in idx:
            scene_of[i] = sc
    w = np.tile(np.asarray(world0, F).reshape(-1)[:P.WORLD_FLOATS], (n, 1)).astype(F)
    for i in range(n):
        row = np.ascontiguousarray(w[i])
        P.infer_state(scene_of[i], row)
        w[i] = row
    env0 = task == "reach" and k0 == 0 and n == K and K >= 2          # (quirk Q8 exactly where oracle.panda.rollout applies it)
    states, cost_h = np.zeros((n, T, 4), F), np.zeros((n, T), F)
    J, g = np.zeros(n, F), F(1.0)
    all_obs = []
    for t in range(T):
        for sc, idx in groups:
            sub = np.ascontiguousarray(w[idx])
            P.step_batch(sc, sub, np.ascontiguousarray(u[idx, t]))
            w[idx] = sub
        states[:, t] = w[:, [0, 9, 1, 10]]
        obs = np.stack([P.observe(scene_of[i], w[i]) for i in range(n)])
        cube0, qh = obs[:, 10:13], obs[:, 13:17]
        if env0:
            cube0 = np.tile(obs[0, 10:13], (n, 1))
            qh = np.tile(obs[0, 13:17], (n, 1))
            if cfg.multi_modal:
                qh[K // 2:] = obs[K // 2, 13:17]
        o = P.make_obs(obs[:, 0:3], obs[:, 3:7], obs[:, 7:10], obs[:, 10:13], obs[:, 13:17], cube0, qh, obs[:, 24:26], obs[:, 26:28],
                       obs[:, 28:30])
        c = P.cost_obs(cfg, o, k0) if cost is None else np.asarray(cost(o, k0 + np.arange(n)), F)
        cost_h[:, t] = c
        gc = (g * c).astype(F)
        J = (J + gc).astype(F)
        g = F(g * F(cfg.gamma))
        if keep_obs:
            all_obs.append(o)
    out = dict(states=states, actions=u.copy(), cost_h=cost_h, J=J)
    if keep_obs:
        out["obs"] = np.stack(all_obs)
    return out


def stitched_planner(P, cfg, delta, task, rows, cost=None):
    """an OraclePandaPlanner whose rollout is the stitched one: command() warm-starts from the stitched costs"""

    class Stitched(P.OraclePandaPlanner):
        def _rollout(self, world0, act):
            r = stitched_rollout(P, self.cfg, task, rows, world0, act, cost=cost)
            s = np.zeros(self.cfg.K, F)
            for t in range(self.cfg.T):
                s = (s + r["cost_h"][:, t]).astype(F)
            r["S"] = s
            return r

    return Stitched(cfg, delta, P.default_scene())


@functools.lru_cache(maxsize=None)
def cycle_reference(cycle, k=X.K, multi_modal=False, weights=None):
    """the first command of the stitched planner on a cycle: actions, states, cost_h, J; computed once per case, the arrays
    read-only.  weights: None, or a tuple of (name, value) pairs of tests/panda_cost_ref.py"""
    import oracle.panda as P
    world, task, grip, _ = CYCLES[cycle]
    cfg = P.make_cfg(k, X.T, multi_modal=multi_modal, task=task, goal=np.array(X.GOAL, F), gripper_cmd=grip)
    cost = None
    if weights is not None:
        from tests import panda_cost_ref as R
        w = R.weights(**dict(weights))
        cost = lambda o, kk: R.cost_of_obs(task, o, goal=np.array(X.GOAL, F), w=w, multi_modal=multi_modal, half_K=k // 2, k=kk)  # noqa: E731
    pl = stitched_planner(P, cfg, X.delta_of(k), task, cycle_rows(cycle, k), cost)
    pl.command(X.world_of(world))
    out = {n: np.array(pl.last[n]) for n in ("actions", "states", "cost_h", "J")}
    for a in out.values():
        a.setflags(write=False)
    return out


def pair_shares(cycle, k=X.K):
    """{(scene a, scene b): the fraction of samples whose cost_h row differs between the two scenes on the oracle alone} for
    every pair of scenes of the cycle"""
    world, task, grip, names = CYCLES[cycle]
    out = {}
    for a, b in itertools.combinations(names, 2):
        ca = X.oracle_rollout(a, world, task, grip, k)["cost_h"]
        cb = X.oracle_rollout(b, world, task, grip, k)["cost_h"]
        assert np.isfinite(ca).all() and np.isfinite(cb).all()
        out[(a, b)] = float((ca.view(np.uint32) != cb.view(np.uint32)).any(axis=1).mean())
    return out
