"""Shared pieces of the panda_env prior-sample tests (tests/test_panda_prior_samples_cpu.py, tests/test_panda_prior_samples_gpu.py;
DESIGN.md section 7l): which samples are priors for a given K, their fixed-seed sequences, the oracle planner that overwrites
those samples' assembled actions before it rolls out, and the guards that the priors matter.  Sizes, worlds and workspaces:
tests/panda_scene_fixture.py; the workspace per sample: tests/panda_rollout_scenes_ref.py.

Index set: every i with i % 5 == 0 that the library does not refuse, plus K - 2.  5 is coprime to every samples-per-wavefront
count of the three kernel forms with and without shadow slots (3, 4, 8, 62, 63, 64), so first and last slots of wavefronts are
hit in every form and a kernel that indexed the slot map by slot, lane or wavefront cannot pass; sample 0 is a prior (the reach
command's shadow slot re-simulates it).  Multi-modal: 0 and K / 2 are the best-trajectory samples (refused), K / 2 - 1 and
K / 2 + 1 are added -- the last sample of mode 1 and the first free one of mode 2."""
import numpy as np

from tests import panda_rollout_scenes_ref as R
from tests import panda_scene_fixture as X

F = np.float32
# world, task, gripper command of the two cases (the probes of tests/panda_scene_fixture.py)
CASES = {"reach": (41, "reach", 2), "pick": (40, "pick", 2)}


def prior_indices(K, mm=False):
    refused = {K - 1} | ({0, K // 2} if mm else set())
    idx = [i for i in range(0, K, 5) if i not in refused]
    for k in ([K // 2 - 1, K // 2 + 1] if mm else []) + [K - 2]:
        if k not in idx:
            idx.append(k)
    return idx


def prior_seqs(n, T=X.T, seed=11):
    """fixed-seed sequences [n, T, 9]; scaled so that more than a tenth of the components lie outside [u_min, u_max]: the clamp
    is exercised (a standard normal times 1.8 against limits of 2 and 1.5: about three in ten)"""
    s = (np.random.default_rng(seed).standard_normal((n, T, 9)) * 1.8).astype(F)
    outside = (s < np.array(X.UMIN, F)) | (s > np.array(X.UMAX, F))
    assert outside.mean() > 0.1 and outside.any(axis=(1, 2)).all()
    return s


def clip(cfg, seqs):
    """the kernel's clamp: fmaxf(fminf(p, u_max), u_min)"""
    lo = np.array([cfg.u_min[j] for j in range(cfg.nu)], F)
    hi = np.array([cfg.u_max[j] for j in range(cfg.nu)], F)
    return np.maximum(np.minimum(np.asarray(seqs, F), hi), lo).astype(F)


def make_panda_prior_planner(P, cfg, delta, idx, seqs, rows=None, task=None, cost=None, **kw):
    """oracle.panda.OraclePandaPlanner (rows: the stitched per-sample-workspace planner of tests/panda_rollout_scenes_ref.py,
    which needs the task's name) whose sample idx[j] rolls out clip(seqs[j]): _rollout overwrites those rows of the assembled
    actions, re-applies the gripper command's override to their columns 7 and 8 (the oracle applies it inside
    assemble_actions, i.e. ahead of this overwrite; the kernel applies it behind its select), then calls the base.  `idx` /
    `seqs` may be replaced between commands (set_priors).  The oracle itself is not edited."""
    base = P.OraclePandaPlanner if rows is None else type(R.stitched_planner(P, cfg, delta, task, rows, cost))

    class _Priors(base):
        def set_priors(self, idx, seqs):
            self.prior_idx = [int(k) for k in idx]
            self.prior_seqs = np.asarray(seqs, F).reshape(len(self.prior_idx), self.cfg.T, self.cfg.nu).copy()

        def _rollout(self, world0, act):
            for j, k in enumerate(self.prior_idx):
                act[k] = clip(self.cfg, self.prior_seqs[j])
                if self.cfg.gripper_cmd != 0:
                    act[k, :, 7:] = 1.5 if self.cfg.gripper_cmd == 1 else -1.5
            return super()._rollout(world0, act)

    p = _Priors(cfg, delta, **kw) if rows is None else _Priors(cfg, delta, P.default_scene(), **kw)
    p.set_priors(idx, seqs)
    return p


def make_cfg(P, case, K, mm=False, grip=None, **kw):
    _, task, g = CASES[case]
    return P.make_cfg(K, X.T, multi_modal=mm, task=task, goal=np.array(X.GOAL, F), gripper_cmd=g if grip is None else grip, **kw)


def joints_that_reach(P, q0, point, iters=30):
    """seven arm joint positions whose finger-tip midpoint (the oracle's forward kinematics, default workspace) lies at
    `point`: damped Gauss-Newton steps of at most 0.1 rad per joint from q0, in float64"""
    sc = P.default_scene()

    def tip(q):
        pos = P.fk(sc, q)["pos"]
        return 0.5 * (np.asarray(pos[9], np.float64) + np.asarray(pos[10], np.float64))

    q = np.asarray(q0, np.float64)[:9].copy()
    point = np.asarray(point, np.float64)
    for _ in range(iters):
        e = tip(q) - point
        jac = np.zeros((3, 7))
        for j in range(7):
            dq = q.copy()
            dq[j] += 1e-4
            jac[:, j] = (tip(dq) - tip(q)) / 1e-4
        q[:7] += np.clip(-np.linalg.solve(jac.T @ jac + 1e-3 * np.eye(7), jac.T @ e), -0.1, 0.1)
    return q[:7]


def assert_priors_matter(P, case, mm, K, label, rows=None):
    """On the oracle alone: every prior sample's `states` row differs bitwise both from what the planner without priors gives
    that sample and from what the NEIGHBOURING prior's sequence would give it -- a dropped select or an off-by-one slot is
    visible.  The share that must differ is all of them."""
    world, task, _ = CASES[case]
    idx = prior_indices(K, mm)
    seqs = prior_seqs(len(idx))
    got = []
    for variant in ("own", "none", "next"):
        s = {"own": seqs, "none": seqs[:0], "next": np.roll(seqs, -1, axis=0)}[variant]
        p = make_panda_prior_planner(P, make_cfg(P, case, K, mm), X.delta_of(K), idx if variant != "none" else [], s, rows=rows, task=task)
        p.command(X.world_of(world))
        assert np.isfinite(p.last["cost_h"]).all() and np.isfinite(p.last["states"]).all()
        got.append(p.last["states"].view(np.uint32)[idx].reshape(len(idx), -1).copy())
    vs_none, vs_next = (got[0] != got[1]).any(1), (got[0] != got[2]).any(1)
    print(f"{label}: prior samples {idx}: differ from the run without priors {int(vs_none.sum())}/{len(idx)}, from the "
          f"neighbouring prior's sequence {int(vs_next.sum())}/{len(idx)}")
    assert vs_none.all() and vs_next.all(), (label, idx, vs_none, vs_next)
