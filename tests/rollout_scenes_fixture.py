"""Shared pieces of the per-sample-arena tests (tests/test_point_rollout_scenes_cpu.py, tests/test_point_rollout_scenes_gpu.py):
the rows, the oracle planner that rolls each sample out in its own arena, and the guard that the rows matter.  Inputs:
tests/point_scene_fixture.py."""
import numpy as np

from tests import point_scene_fixture as X

F = np.float32
CYCLE = (None, X.CUSTOM, X.CUSTOM_B)   # rows cycle with period three: default, CUSTOM, CUSTOM_B


def cycle_rows(K, shift=0):
    """row i: CYCLE[(i + shift) % 3], as field overrides (None: the reference's arena)"""
    return [CYCLE[(i + shift) % 3] for i in range(K)]


def make_stitched(O, cfg, delta, rows, **kw):
    """oracle.OraclePointPlanner whose sample k rolls out in rows[k]: point_rollout once per run of equal rows, the results
    stitched; each run's slice of the pending force copied in and out, contiguously.  (The base class lives in the oracle
    package, which the suite imports lazily.)"""
    class _Stitched(O.OraclePointPlanner):
        def __init__(self, cfg, delta, rows, **kw):
            super().__init__(cfg, delta, **kw)
            assert len(rows) == cfg.K
            self.rows = list(rows)
            self.scenes = [X.oracle_scene(O, r) for r in self.rows]
            self.shift_rows = 0   # the guard's "what if sample k took row k + shift_rows" (None: every sample the default arena)

        def _row_of(self, k):
            if self.shift_rows is None:
                return None, X.oracle_scene(O, None)
            j = (k + self.shift_rows) % len(self.rows)
            return self.rows[j], self.scenes[j]

        def _rollout(self, world0, act):
            K = self.cfg.K
            parts, k0 = [], 0
            while k0 < K:
                row, sc = self._row_of(k0)
                k1 = k0 + 1
                while k1 < K and self._row_of(k1)[0] == row:
                    k1 += 1
                pend = np.ascontiguousarray(self.pend[k0:k1])
                parts.append(O.point_rollout(self.cfg, sc, world0, np.ascontiguousarray(act[k0:k1]), pend, k0, k1))
                self.pend[k0:k1] = pend
                k0 = k1
            return {name: np.concatenate([p[name] for p in parts], axis=0) for name in parts[0]}

    return _Stitched(cfg, delta, rows, **kw)


def row_shares(O, task, mm, K, w0, T=X.T, rows=None):
    """On the oracle alone, the shares of the samples whose robot states differ between their own arena and (the next row's
    arena, the previous row's arena, the default arena): what makes an off-by-one row or a wave-uniform arena visible."""
    rows = cycle_rows(K) if rows is None else rows
    out = []
    for shift in (0, 1, -1, None):
        opl = make_stitched(O, O.make_cfg(K, T, 2, task=task, goal=X.GOAL, multi_modal=mm, filter_u=False), X.actions(K, T), rows)
        opl.shift_rows = shift
        opl.command(w0)
        assert np.isfinite(opl.last["cost_h"]).all()
        out.append(opl.last["states"].view(np.uint32).reshape(K, -1).copy())
    return tuple(float((out[0] != o).any(1).mean()) for o in out[1:])


def assert_rows_matter(O, task, mm, K, w0, label, T=X.T, rows=None):
    nxt, prv, dflt = row_shares(O, task, mm, K, w0, T, rows)
    print(f"{label}: share of samples that differ from the next row's arena {nxt:.3f}, the previous row's {prv:.3f}, "
          f"the default arena {dflt:.3f}")
    assert nxt >= 0.8 and prv >= 0.8 and dflt >= 0.5, (label, nxt, prv, dflt)
