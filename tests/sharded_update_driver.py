"""Driver of tests/test_sharded_update_f64_gpu.py and tests/test_sharded_update_f64_cpu.py: N shard engines with the
phase interface (rollout / update / update_b / finalize + buffers) in one process, driven in lock step with every
collective done by hand, on synthetic costs, and every rank compared with the float64 restatement of the reference
(tests/update_ref.py) evaluated on the whole cost vector.  The engines are HipEngine handles (GPU module) or
tests/oracle_engine.OracleEngine (CPU self-check); nothing here waits on a flag or needs a second process.

Protocols (`proto`): 0 gather + reduce, 1 / 2 / 3 = cfg.shard_mix.  `mode`: single / simple / multi; nu = 9 is Panda.
"""
import copy

import numpy as np
import torch

from tests import update_ref as R
from tests.update_f64_checks import U32, check_call, check_weights, make_costs, new_state, stage_a_survivors

TOPK = R.TOPK
# What the mixture of the shards adds to the relative bound on a weight / an eta (derivation: docstring of
# tests/test_sharded_update_f64_gpu.py): (3 (ln 2^24 + 1) + 32 + 16) u
MIX_EXTRA = (3 * (np.log(2.0 ** 24) + 1) + 32 + 16) * U32


class Case:
    def __init__(self, id, proto, mode, shards, dist, T=12, nu=2, calls=1, cov=False, null_action=True, u_scale=1.0,
                 min_iters=0):
        self.id, self.proto, self.mode, self.shards, self.dist = id, proto, mode, list(shards), dist
        self.T, self.nu, self.calls, self.cov, self.null_action, self.u_scale = T, nu, calls, cov, null_action, u_scale
        self.min_iters = min_iters
        self.K = sum(self.shards)
        self.offsets = np.concatenate([[0], np.cumsum(self.shards)]).astype(int)
        self.regen = mode == "multi" and proto in (1, 2)      # the other ranks' actions are re-generated

    def rank_of(self, k):
        return int(np.searchsorted(self.offsets, k, side="right") - 1)


# ---- cost vectors: make_costs on the whole vector, or a layout relative to the rank boundaries ------------------------

def _must(pred):
    def claim(J):
        assert pred(J)
    return claim


def sharded_costs(case, rng, call):
    """(J, claim): the global cost vector and a function that asserts what the case's id claims about it."""
    K, off, N, dist = case.K, case.offsets, len(case.shards), case.dist
    order = lambda J: np.argsort(J, kind="stable")[:TOPK]
    ranks = lambda idx: [case.rank_of(k) for k in idx]
    if dist.startswith("shift"):          # rank r's costs lie 1e3 r / 1e8 r above rank 0's: whole ranks vanish in the mixture
        step = float(dist[5:])
        J = np.abs(rng.standard_normal(K))
        for r in range(N):
            J[off[r]:off[r + 1]] += step * r
        J = J.astype(np.float32)

        def claim(J):
            assert all(J[off[r]:off[r + 1]].min() > J[off[r - 1]:off[r]].max() for r in range(1, N))
        return J, claim
    base = (np.abs(rng.standard_normal(K)) + 0.5).astype(np.float32)
    J = base
    if dist == "lastmin":                 # the global minimum is the last sample of the last rank
        J[K - 1] = 0.25
        return J, _must(lambda J: int(np.argmin(J)) == K - 1)
    if dist == "dup2ranks":               # the minimum twice, in the first and in the last rank
        a, b = int(off[1]) - 2, int(off[N - 1]) + 1
        J[a] = J[b] = 0.125

        def claim(J):
            m = np.flatnonzero(J == J.min())
            assert len(m) == 2 and len(set(ranks(m))) == 2
        return J, claim
    if dist in ("edge_in", "edge_20_21"):  # equal costs at the last sample of rank r and the first of rank r + 1
        e = int(off[1])
        s = np.sort(J)
        v = np.float32(0.5 * (float(s[4]) + float(s[5]))) if dist == "edge_in" else None
        if dist == "edge_20_21":          # 19 samples below the pair: it takes places 20 and 21, the lower index wins
            low = rng.choice(np.setdiff1d(np.arange(K), [e - 1, e]), 19, replace=False)
            J[low] = (0.01 + 0.001 * np.arange(19)).astype(np.float32)
            v = np.float32(0.2)
        J[e - 1] = J[e] = v

        def claim(J):
            o = np.argsort(J, kind="stable")
            p = int(np.flatnonzero(o == e - 1)[0])
            assert o[p + 1] == e and (p < TOPK - 1 if dist == "edge_in" else p == TOPK - 1), (p, o[:22])
        return J, claim
    if dist == "top20_one_rank":
        r = N - 1
        J[off[r]:off[r] + 25] = (0.01 + 0.001 * rng.permutation(25)).astype(np.float32)
        return J, _must(lambda J: set(ranks(order(J))) == {r})
    if dist == "top20_spread":            # exactly one of the top-20 in each of 20 different ranks
        rs = rng.choice(N, TOPK, replace=False)
        for q, r in enumerate(rs):
            J[off[r] + int(rng.integers(case.shards[r]))] = np.float32(0.01 + 0.001 * q)
        return J, _must(lambda J: len(set(ranks(order(J)))) == TOPK)
    if dist == "rank_inf":                # one rank all +inf, the others finite
        J[off[1]:off[2]] = np.inf
        return J, _must(lambda J: np.isinf(J[off[1]:off[2]]).all() and np.isfinite(np.delete(J, np.arange(off[1], off[2]))).all())
    if dist == "rank_some_inf":
        J[off[1] + rng.choice(case.shards[1], min(7, case.shards[1] // 3), replace=False)] = np.inf
        return J, _must(lambda J: 0 < np.isinf(J[off[1]:off[2]]).sum() < case.shards[1])
    if dist == "tie3":                    # the weight argmax tie of "tie", its three samples in three ranks (per half when multi)
        halves = ((0, K),) if case.mode != "multi" else ((0, K // 2), (K // 2, K))
        pts = []
        for lo, hi in halves:
            rr = sorted({case.rank_of(lo), case.rank_of((lo + hi) // 2), case.rank_of(hi - 1)})
            ks = [max(lo, int(off[r])) + 1 for r in rr]
            pts.append(ks)
            for k, v in zip(ks, (3e-9, 1e-9, 0.0)):
                J[k] = v

        def claim(J):
            for ks in pts:
                assert len(ks) == 3 and len(set(ranks(ks))) == 3, ks
        return J, claim
    if dist == "zeros_edge":              # -0.0 / +0.0 either side of a rank boundary (equal costs, ordered by index)
        e = int(off[1])
        J[e - 1], J[e], J[e + 1] = 0.0, -0.0, 0.0
        if case.mode == "multi":
            e2 = int(off[case.rank_of(K // 2) + 1]) if case.rank_of(K // 2) + 1 < N else K - 1
            J[e2 - 1], J[e2] = -0.0, 0.0
        return J, _must(lambda J: np.signbit(J[e]) and J[e - 1] == J[e])
    if dist == "mode_inf":                # the mode-1 samples of the rank that straddles K / 2 all +inf, its mode-2 samples finite
        r = case.rank_of(K // 2)
        assert off[r] < K // 2 < off[r + 1]
        J[off[r]:K // 2] = np.inf
        return J, _must(lambda J: np.isinf(J[off[r]:K // 2]).all() and np.isfinite(J[K // 2:off[r + 1]]).all() and np.isfinite(J[:off[r]]).all())
    J = make_costs(dist, K, rng, call)
    h = K // 2
    claims = {
        "inf": lambda J: 0 < np.isinf(J).sum() < TOPK,
        "inf24": lambda J: K - np.isinf(J).sum() < TOPK,                       # the top-20 must hold +inf rows
        "neg": lambda J: (J < 0).all(),
        "offset": lambda J: J.min() >= 1e6,
        "s1e-5": lambda J: J.max() < 1e-4,
        "s1e8": lambda J: np.median(J) > 1e7,
        "zeros": lambda J: np.signbit(J[J == 0]).any() and (~np.signbit(J[J == 0])).any(),
        "tie": lambda J: J[3] > J[9] == J.min() and np.float32(np.exp(-np.float64(J[3]))) == np.float32(1.0),
        "dupmin": lambda J: (J == J.min()).sum() >= 2,
        "stageA": lambda J: all(stage_a_survivors(J[off[r]:off[r + 1]]) > 1024 for r in range(N)),
        # stage B of every rank: more than 1024 of its workgroups' candidates are copies of the smallest value
        "stageB": lambda J: all((J[off[r]:off[r + 1]] == 1.0).sum() > 1024 for r in range(N)),
        "cycle": lambda J: True, "s1": lambda J: True,                            # (no claim in the id beyond the geometry)
    }
    return J, _must(claims[dist])


# ---- back ends ----------------------------------------------------------------------------------------------------

def _cfg_kwargs(case):
    if case.nu == 9:
        return dict(u_min=[-2.0] * 7 + [-1.5] * 2, u_max=[2.0] * 7 + [1.5] * 2, noise_sigma_diag=[10.0] * 7 + [0.8] * 2,
                    lambda_=0.05, dt=0.01, env_type="panda_env", pre_height_diff=0.05)
    return dict(u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3], lambda_=0.5 if case.mode == "simple" else 1.0)


class HipBackend:
    name = "hip"

    def engine(self, case, r):
        from m3p2i_aip_amd.engine import HipEngine, make_config
        return HipEngine(make_config(K=case.K, K_local=case.shards[r], k_offset=int(case.offsets[r]), T=case.T, nu=case.nu,
                                     multi_modal=case.mode == "multi", mode_simple=case.mode == "simple",
                                     shard_mix=case.proto, update_cov=case.cov, sample_null_action=case.null_action,
                                     u_scale=case.u_scale, **_cfg_kwargs(case)))

    def prepare_rollout(self, e, case):
        if case.nu == 9:
            e.set_objective("reach", np.array([0.2, 0.2, 1.115, 0, 0, 0, 1], np.float32), gripper_cmd=1)
        else:
            e.set_objective("push_pull", (-3.75, -3.75))
            e.set_world_point_raw(np.array([0.0, 1.5, 0, 0, 0, 2, 1, 0, 0, 0, 0, -2, 2, 1, 0, 0, 0, 0], np.float32))

    def sync(self):
        torch.cuda.synchronize()


class OracleBackend:
    name = "oracle"

    def engine(self, case, r):
        from m3p2i_aip_amd.engine import make_config
        from tests.oracle_engine import OracleEngine
        return OracleEngine(make_config(K=case.K, K_local=case.shards[r], k_offset=int(case.offsets[r]), T=case.T, nu=case.nu,
                                        multi_modal=case.mode == "multi", shard_mix=case.proto, update_cov=case.cov,
                                        sample_null_action=case.null_action, u_scale=case.u_scale, **_cfg_kwargs(case)))

    def prepare_rollout(self, e, case):
        root = torch.zeros(1, 11, 13)
        root[0, :, 6] = 1.0
        root[0, 6, 0:2] = torch.tensor([0.0, 2.0])
        root[0, 5, 0:2] = torch.tensor([-2.0, 2.0])
        e.set_objective("push_pull", (-3.75, -3.75))
        e.bind_sim_point(torch.tensor([[0.0, 0.0, 1.5, 0.0]]), root, 6, 5)

    def sync(self):
        pass


def smooth_noise(K, T, nu, seed):
    """random smooth rows, distinct per sample (the Halton spline's role; values are inputs of the test)"""
    g = torch.Generator().manual_seed(seed)
    knots = torch.randn(K, nu, max(2, T // 4), generator=g)
    d = torch.nn.functional.interpolate(knots, size=T, mode="linear", align_corners=True)
    return d.permute(0, 2, 1).contiguous().numpy()


# ---- the driver -----------------------------------------------------------------------------------------------------

PLAN_BUFS = ("BUF_ACTION_OUT", "BUF_MEAN", "BUF_MEAN_1", "BUF_MEAN_2", "BUF_BEST", "BUF_BEST_1", "BUF_BEST_2", "BUF_TOP_TRAJS",
             "BUF_TOP_IDX")
INFO_FIELDS = ("eta", "eta_1", "eta_2", "beta", "beta_1", "beta_2", "iters", "iters_1", "iters_2", "best_idx", "best_idx_1",
               "best_idx_2", "wsum_push", "wsum_pull", "pull_preference", "calls")


def _np(t):
    return t.cpu().numpy().copy()


def _put(e, buf, a):
    e.buffer(buf).copy_(torch.from_numpy(np.ascontiguousarray(a)))


def _collect(engines, buf):
    return torch.stack([e.buffer(buf) for e in engines])


def exchange(L, case, engines):
    """Phases after the rollout, the collectives by hand (copies between the handles' buffers)."""
    if case.proto == 0:
        J = torch.cat([e.buffer(L.BUF_TRAJ_COST) for e in engines])                  # all_gather
        for e in engines:
            e.buffer(L.BUF_TRAJ_COST_ALL).copy_(J)
            e.update()
        red = _collect(engines, L.BUF_REDUCE).sum(0)                                 # all_reduce(sum)
        for e in engines:
            e.buffer(L.BUF_REDUCE).copy_(red)
            e.finalize()
        return
    for e in engines:
        e.update()
    rec = _collect(engines, L.BUF_RECORD).clone()                                    # all_gather of the records
    for e in engines:
        e.buffer(L.BUF_RECORDS_ALL).copy_(rec)
        if case.proto == 3:
            e.update_b()
        else:
            e.finalize()
    if case.proto == 3:
        recb = _collect(engines, L.BUF_RECORD_B).clone()                             # the second, small all_gather
        for e in engines:
            e.buffer(L.BUF_RECORDS_B_ALL).copy_(recb)
            e.finalize()


def _mix_best(got):
    """The mixture of local softmins returns products rounded per rank, so "first index of the maximum of the returned
    weights" is not defined by the formula.  What is: the reference's float32 weights tie exactly where exp(-x) rounds to
    the same binary32 value as the maximum; the first index among those wins.  Samples within 8 u of the maximum without
    rounding to it may go either way."""
    def best_of(wr):
        g = wr / wr.max()
        sure = np.flatnonzero(g.astype(np.float32) == np.float32(1.0))
        near = np.flatnonzero(g >= 1.0 - 8 * U32)
        if len(near) == len(sure):
            return int(sure[0])
        assert got in near, (got, near)
        return int(got)
    return best_of


def run_sharded_case(backend, case, seed):
    from m3p2i_aip_amd import _lib as L
    K, T, nu, N, off, mode, proto = case.K, case.T, case.nu, len(case.shards), case.offsets, case.mode, case.proto
    half = K // 2
    mix = proto == 1 and mode != "multi"
    own_slices = mix or proto == 3           # a rank materialises the weights of its own samples only
    # the mixture term: k_mix and the mixed ladder tables of shard_mix = 2 / 3.  Gather + reduce and shard_mix = 1
    # multi-modal run the unsharded kernels on all gathered costs: the unsharded bounds as they are.
    extra = MIX_EXTRA if (mix or proto in (2, 3)) else 0.0
    engines = [backend.engine(case, r) for r in range(N)]
    try:
        rng = np.random.default_rng(seed)
        ss = float(engines[0].cfg.step_size_mean)
        lam = float(engines[0].cfg.lambda_)
        mean = rng.uniform(-1, 1, (5, T, nu)).astype(np.float32)
        for e in engines:
            for q, b in enumerate((L.BUF_MEAN, L.BUF_MEAN_1, L.BUF_MEAN_2, L.BUF_BEST_1, L.BUF_BEST_2)):
                if q == 0 or mode == "multi":
                    _put(e, b, mean[q])
        if case.regen:
            delta = smooth_noise(K, T, nu, seed)
            for e in engines:
                assert e.needs_global_noise
                e.set_noise(delta)
                backend.prepare_rollout(e, case)
        st = new_state(mean[0], list(engines[0].cfg.noise_sigma_diag)[:nu])
        cov0 = [_np(e.buffer(L.BUF_COV)) for e in engines]
        seen_iters = 0
        for call in range(case.calls):
            J, claim = sharded_costs(case, rng, call)
            claim(J)
            if case.regen:
                for e in engines:
                    e.rollout()                                  # fills states / actions; its costs are replaced
                backend.sync()
                A = np.concatenate([_np(e.buffer(L.BUF_ACTIONS)) for e in engines], axis=1)
                S = np.concatenate([_np(e.buffer(L.BUF_STATES)) for e in engines], axis=1)
                assert A.shape == (T, K, nu) and np.isfinite(A).all() and np.isfinite(S).all()
            else:
                A = rng.uniform(-3, 3, (T, K, nu)).astype(np.float32)
                S = rng.uniform(-5, 5, (T, K, 4)).astype(np.float32)
            for r, e in enumerate(engines):
                lo, hi = off[r], off[r + 1]
                _put(e, L.BUF_TRAJ_COST, J[lo:hi])
                if not case.regen:
                    _put(e, L.BUF_ACTIONS, A[:, lo:hi])
                    _put(e, L.BUF_STATES, S[:, lo:hi])
            exchange(L, case, engines)
            backend.sync()
            infos = [e.info() for e in engines]
            gets = [(lambda b, e=e: _np(e.buffer(b))) for e in engines]
            # ---- the weights every rank holds ----
            full = [(g(L.BUF_WEIGHTS),) + ((g(L.BUF_WEIGHTS_1), g(L.BUF_WEIGHTS_2)) if mode == "multi" else (None, None)) for g in gets]
            if own_slices:
                asm = [np.zeros(K, np.float32), np.zeros(half, np.float32), np.zeros(K - half, np.float32)]
                for r in range(N):
                    lo, hi = off[r], off[r + 1]
                    asm[0][lo:hi] = full[r][0][lo:hi]
                    if mode == "multi":
                        asm[1][min(lo, half):min(hi, half)] = full[r][1][min(lo, half):min(hi, half)]
                        asm[2][max(lo - half, 0):max(hi - half, 0)] = full[r][2][max(lo - half, 0):max(hi - half, 0)]
            for r, e in enumerate(engines):
                i = infos[r]
                if r == 0 or not own_slices:     # (assembled slices: one vector for all ranks, compared once)
                    st_r = copy.deepcopy(st)
                    check_call(L, gets[r], i, J, A, S, st_r, K=K, nu=nu, mode=mode, cov=False, lambda_=lam, ss=ss, call=call,
                               weights=tuple(asm) if own_slices else full[r], extra=extra,
                               best_of=_mix_best(i.best_idx) if mix else None)
                if mix:      # ... and, beyond its slice, the weights at the global top-k indices (mppi.py:248)
                    ti = np.argsort(J, kind="stable")[:TOPK]
                    check_weights(full[r][0][ti], J, st_r["beta_used"], f"call {call} rank {r} top-k weights", MIX_EXTRA, only=ti)
                # ---- ranks among each other: bit-identical plans, top-k and info ----
                for name in PLAN_BUFS:
                    b = getattr(L, name)
                    assert torch.equal(e.buffer(b), engines[0].buffer(b)), f"call {call}: ranks {r} and 0 disagree on {name}"
                for f in INFO_FIELDS:
                    assert getattr(i, f) == getattr(infos[0], f), f"call {call}: ranks {r} and 0 disagree on info.{f}"
                if not own_slices:
                    for q in range(3 if mode == "multi" else 1):
                        assert np.array_equal(full[r][q], full[0][q]), f"call {call}: ranks {r} and 0 disagree on weights {q}"
            st = st_r
            seen_iters = max(seen_iters, infos[0].iters)
        assert seen_iters > case.min_iters, (seen_iters, case.min_iters)   # (the fallback passes beyond the ladder really ran)
        if case.cov:       # update_cov on a multi-modal handle: the no-op the reference makes of it
            assert mode == "multi" and case.calls >= 3
            for e, c0 in zip(engines, cov0):
                assert np.array_equal(_np(e.buffer(L.BUF_COV)), c0)
    finally:
        for e in engines:
            e.close()
