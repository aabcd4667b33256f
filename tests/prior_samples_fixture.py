"""Shared pieces of the prior-sample tests (tests/test_prior_samples_cpu.py, tests/test_prior_samples_gpu.py): which samples
are priors for a given K, their fixed-seed sequences, the oracle planner that overwrites those samples' actions before it rolls
out, and the guard that the priors matter.  Inputs: tests/point_scene_fixture.py; the per-sample arenas:
tests/rollout_scenes_fixture.py."""
import numpy as np

from tests import point_scene_fixture as X
from tests import rollout_scenes_fixture as R

F = np.float32
U_LIM = 3.0   # the planners of these tests run with u_min = -3, u_max = 3 (oracle.make_cfg's defaults, the engines' PK)


def prior_indices(K, mm=False):
    """the first and last lane of a wavefront and the first lane of the next (0 is a best-trajectory sample in multi-modal
    mode: 1 then), K - 2 (K - 1 is the zero-noise sample), and in multi-modal mode the two neighbours of K / 2"""
    idx = [1 if mm else 0]
    idx += [k for k in (63, 64) if k < K - 2 and not (mm and k == K // 2)]
    idx.append(K - 2)
    if mm:
        idx += [K // 2 - 1, K // 2 + 1]
    out = []
    for k in idx:
        if k not in out:
            out.append(k)
    return out


def prior_seqs(n, T=X.T, seed=7):
    """fixed-seed sequences [n, T, 2], about a quarter of the components outside [-3, 3]: the clamp is exercised"""
    s = (np.random.default_rng(seed).standard_normal((n, T, 2)) * 2.6).astype(F)
    assert (np.abs(s) > U_LIM).mean() > 0.1
    return s


def clip(cfg, seqs):
    """the kernel's clamp: fmaxf(fminf(p, u_max), u_min)"""
    lo = np.array([cfg.u_min[j] for j in range(cfg.nu)], F)
    hi = np.array([cfg.u_max[j] for j in range(cfg.nu)], F)
    return np.maximum(np.minimum(np.asarray(seqs, F), hi), lo).astype(F)


def make_prior_planner(O, cfg, delta, idx, seqs, rows=None, **kw):
    """oracle.OraclePointPlanner (rows: the stitched per-sample-arena planner) whose sample idx[j] rolls out clip(seqs[j]):
    _rollout overwrites those rows of the assembled actions, then calls the base.  `idx` / `seqs` may be replaced between
    commands (set_priors).  (The base classes live in the oracle package, which the suite imports lazily.)"""
    base = O.OraclePointPlanner if rows is None else type(R.make_stitched(O, cfg, delta, rows))

    class _Priors(base):
        def set_priors(self, idx, seqs):
            self.prior_idx = [int(k) for k in idx]
            self.prior_seqs = np.asarray(seqs, F).reshape(len(self.prior_idx), self.cfg.T, self.cfg.nu).copy()

        def _rollout(self, world0, act):
            for j, k in enumerate(self.prior_idx):
                act[k] = clip(self.cfg, self.prior_seqs[j])
            return super()._rollout(world0, act)

    p = _Priors(cfg, delta, **kw) if rows is None else _Priors(cfg, delta, rows, **kw)
    p.set_priors(idx, seqs)
    return p


def assert_priors_matter(O, task, mm, K, w0, label, T=X.T, rows=None, idx=None, seqs=None, **cfg_kw):
    """On the oracle alone: every prior sample's robot states differ both from what the planner without priors gives that
    sample and from what the NEIGHBOURING prior's sequence would give it -- an off-by-one slot or a dropped select is visible.
    The share that must differ is all of them."""
    cfg_kw = cfg_kw or dict(filter_u=False)
    idx = prior_indices(K, mm) if idx is None else list(idx)
    seqs = prior_seqs(len(idx), T) if seqs is None else seqs
    assert len(idx) >= 2
    mk = lambda: O.make_cfg(K, T, 2, task=task, goal=X.GOAL, multi_modal=mm, **cfg_kw)
    got = []
    for variant in ("own", "none", "next"):
        s = {"own": seqs, "none": seqs[:0], "next": np.roll(seqs, -1, axis=0)}[variant]
        p = make_prior_planner(O, mk(), X.actions(K, T), idx if variant != "none" else [], s, rows=rows)
        p.command(w0)
        assert np.isfinite(p.last["cost_h"]).all()
        got.append(p.last["states"].view(np.uint32)[idx].reshape(len(idx), -1).copy())
    vs_none, vs_next = (got[0] != got[1]).any(1), (got[0] != got[2]).any(1)
    print(f"{label}: prior samples {idx}: differ from the run without priors {int(vs_none.sum())}/{len(idx)}, from the "
          f"neighbouring prior's sequence {int(vs_next.sum())}/{len(idx)}")
    assert vs_none.all() and vs_next.all(), (label, idx, vs_none, vs_next)
