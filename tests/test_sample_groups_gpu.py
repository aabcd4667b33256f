"""Sample groups (m3_set_sample_groups) on the GPU.

1. The kernel alone on synthetic costs (m3_aggregate_sample_groups): K = 160, groups of 2, 3, 15 and 16 members, one across two
   wavefronts (samples 3 and 131), ties, signed zeros, a +inf member, an all-+inf group, a NaN member; worst_frac giving j = 1,
   j = M_g and a strict between.  TRAJ_COST equals the numpy binary32 emulation (groups.aggregate_reference, held to the host
   program and the committed fixture by tests/test_sample_groups_cpu.py) bit for bit, the raw block equals the input, samples on
   their own are untouched.
2. Whole commands, warm-started: a handle with groups against a TWIN with the same noise and arenas and no groups -- the
   controls are bitwise equal within every group, the raw costs are bitwise the twin's costs (the rollout is untouched),
   TRAJ_COST is bitwise the emulated aggregate, and plan, weights and m3_info are bitwise the twin's after its TRAJ_COST is
   overwritten with the aggregates and m3_update_finalize runs; the twin's plan buffers are re-synchronised per call
   (m3_set_plan).  point_env push K = 64, T = 8, M = 4 arenas; an unsharded multi-modal handle at the smallest K that takes the
   three-launch update (where stale wave minima would show); panda_env reach K = 32, T = 4, two workspaces.
3. Groups that change nothing: all members in one arena and worst_frac = 1 -- bit for bit the plain command for power-of-two
   sizes; for 3 members the plan within the bound the aggregate's two roundings allow.
4. Refusals with their texts, a refused call changes nothing, the batch and both lockstep episode sets refuse, NULL clears,
   the groups survive m3_reset, and the ledger's count of live blocks.
"""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd import groups, scenes  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, HipEpisodes, HipPandaEpisodes, make_config  # noqa: E402
from tests import point_scene_fixture as X  # noqa: E402
from tests.test_batch_command_gpu import PK  # noqa: E402
from tests.test_batch_panda_gpu import GOALS as PANDA_GOALS, PK as PANDA_PK, _worlds as panda_worlds  # noqa: E402
from tests.test_hip_parity_point import raw_world  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_BUFS = [L.BUF_MEAN, L.BUF_MEAN_1, L.BUF_MEAN_2, L.BUF_BEST, L.BUF_BEST_1, L.BUF_BEST_2]
OUT_BUFS = [L.BUF_ACTION_OUT, L.BUF_WEIGHTS, L.BUF_WEIGHTS_1, L.BUF_WEIGHTS_2, L.BUF_TOP_IDX, L.BUF_TOP_TRAJS, L.BUF_TRAJ_COST,
            L.BUF_COV] + PLAN_BUFS


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def buf(e, which):
    try:
        return e.buffer(which)
    except L.M3Error:
        return None


def assert_same_bits(a, b, label):
    assert np.array_equal(bits(a), bits(b)), f"{label}: {int((bits(a) != bits(b)).sum())} of {bits(a).size} words differ"


# ------------------------------------------------------------------ 1. the kernel alone
def _synthetic(K=160):
    rng = np.random.default_rng(7)
    J = (50.0 * np.abs(rng.standard_normal(K)) + 1.0).astype(F)
    g = np.full(K, -1, np.int64)
    g[[3, 131]] = 9                                  # 2 members in different wavefronts (and blocks of 64)
    g[[5, 70, 6]] = 0                                # 3 members, out of order across a wavefront
    g[10:25] = 24                                    # 15
    g[100:116] = 100                                 # 16
    g[[30, 31]] = 31                                 # a tie
    g[40:44] = 40                                    # all +inf
    g[[50, 51, 52]] = 50                             # a NaN member
    g[60:65] = 60                                    # a +inf member
    g[[66, 67]] = 66                                 # -0.0 and +0.0
    g[[80, 85, 90, 95]] = 159                        # ties inside a larger group; the id is a label (K - 1 is allowed as one)
    J[30] = J[31] = F(12.5)
    J[40:44] = np.inf
    J[51] = np.nan
    J[62] = np.inf
    J[66], J[67] = F(-0.0), F(0.0)
    J[[80, 90]] = J[85]
    J[12] = J[20] = J[11]
    return J, g


@pytest.mark.parametrize("worst", [1.0 / 16.0, 0.5, 1.0], ids=["j=1", "between", "j=M"])
def test_the_kernel_alone_on_synthetic_costs(worst):
    K = 160
    J, g = _synthetic(K)
    sizes = {int(i): int((g == i).sum()) for i in np.unique(g[g >= 0])}
    assert {2, 3, 15, 16} <= set(sizes.values())
    js = {m: groups.worst_j(worst, m) for m in sizes.values()}
    if worst == 0.5:
        assert all(1 < js[m] < m for m in (3, 15, 16))            # a strict between
    else:
        assert all(js[m] == (1 if worst < 0.5 else m) for m in js)
    eng = HipEngine(make_config(K=K, T=8, nu=2, filter_u=False, **PK))
    try:
        with pytest.raises(L.M3Error, match=r"error -4: m3_aggregate_sample_groups: the handle has no sample groups"):
            eng.aggregate_sample_groups()
        eng.set_sample_groups(g, worst)
        assert eng.sample_groups_set() == len(sizes)
        for k in range(K):
            want = (int(g[k]), sizes[int(g[k])], js[sizes[int(g[k])]]) if g[k] >= 0 else (-1, 1, 1)
            assert eng.sample_group(k) == want, k
        for rep in range(2):        # (the second launch aggregates the aggregates: the raw block follows its input again)
            src = J if rep == 0 else want_J
            eng.buffer(L.BUF_TRAJ_COST).copy_(torch.from_numpy(src))
            eng.aggregate_sample_groups()
            torch.cuda.synchronize()
            want_J = groups.aggregate_reference(src, g, worst)
            got = eng.buffer(L.BUF_TRAJ_COST).cpu().numpy()
            assert_same_bits(got, want_J, f"TRAJ_COST, launch {rep}")
            assert_same_bits(eng.raw_costs(), src, f"raw block, launch {rep}")
            assert np.array_equal(bits(got)[g < 0], bits(src)[g < 0])   # samples on their own: untouched
        first = groups.aggregate_reference(J, g, worst)
        assert np.isnan(first[[50, 51, 52]]).all() and np.isposinf(first[40:44]).all() and np.isposinf(first[60:65]).all()
        assert np.isfinite(first[[3, 131]]).all() and bits(first[3]) == bits(first[131])
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. whole commands against the twin
def _compare_outputs(A, B, label):
    for which in OUT_BUFS:
        a, b = buf(A, which), buf(B, which)
        assert (a is None) == (b is None), (label, which)
        if a is not None:
            assert_same_bits(a, b, f"{label}: buffer {which}")
    assert bytes(A.info()) == bytes(B.info()), f"{label}: m3_info differs"


def _grouped_command_equals_the_twin(A, B, g, worst, set_world, calls, label, expect_models_differ=False):
    """A has the groups, B is its twin without; both hold the same noise (tiled), arenas and objective"""
    differ = 0
    for call in range(calls):
        if call:
            for which in PLAN_BUFS:      # (bitwise equal already: the re-synchronisation keeps a miss from compounding)
                if buf(A, which) is not None:
                    B.set_plan(which, A.buffer(which).cpu().numpy())
        set_world(call)
        A.command()
        B.rollout()
        torch.cuda.synchronize()
        tag = f"{label} call {call}"
        raw = A.raw_costs().cpu().numpy()
        assert_same_bits(raw, B.buffer(L.BUF_TRAJ_COST), f"{tag}: raw costs against the twin's costs")
        assert_same_bits(A.buffer(L.BUF_ACTIONS), B.buffer(L.BUF_ACTIONS), f"{tag}: controls against the twin's")
        assert_same_bits(A.buffer(L.BUF_COST_HORIZON), B.buffer(L.BUF_COST_HORIZON), f"{tag}: step costs")
        act = bits(A.buffer(L.BUF_ACTIONS))                      # [T][K][nu]
        for gid in np.unique(g[g >= 0]):
            members = np.nonzero(g == gid)[0]
            assert (act[:, members, :] == act[:, members[:1], :]).all(), f"{tag}: group {gid}: members' controls differ"
            differ += int(len(set(bits(raw[members]).tolist())) > 1)
        agg = groups.aggregate_reference(raw, g, worst)
        assert_same_bits(A.buffer(L.BUF_TRAJ_COST), agg, f"{tag}: TRAJ_COST against the emulated aggregate")
        B.buffer(L.BUF_TRAJ_COST).copy_(torch.from_numpy(agg))
        B.update_finalize()
        torch.cuda.synchronize()
        _compare_outputs(A, B, tag)
    if expect_models_differ:      # (the guard that the arenas matter: else equal members would hide a wrong member table)
        n = len(np.unique(g[g >= 0])) * calls
        print(f"{label}: {differ} of {n} (group, call) pairs have members whose costs differ")
        assert differ >= n // 2, (differ, n)


def _point_pair(K, T, M, mm, task, worst, seed, arenas=True, set_groups=True):
    g, model_of = groups.grouped_layout(K, M, mm)
    delta = groups.tile_noise((np.random.default_rng(seed).standard_normal((K, T, 2)) * 1.5).astype(F), g)
    rows = None
    if arenas:
        models = scenes.spread_point_scenes(M, 0.4, seed=3, fields=("box_m", "box_mu_g", "mu_rb", "robot_m"))
        rows = [models[m] if m >= 0 else None for m in model_of.tolist()]
    engs = []
    for _ in range(2):
        e = HipEngine(make_config(K=K, T=T, nu=2, multi_modal=mm, filter_u=False, **PK))
        e.set_objective(task, X.GOAL)
        e.set_noise(delta)
        if rows is not None:
            e.set_point_rollout_scenes(rows)
        engs.append(e)
    if set_groups:
        engs[0].set_sample_groups(g, worst)
    return engs[0], engs[1], g.astype(np.int64)


def _point_worlds(oracle, engs):
    w0 = X.start_worlds(oracle)[2].copy()           # the robot at the box: the push meets the arenas' masses and frictions

    def set_world(call):
        w = w0.copy()
        w[0] += 0.02 * call
        for e in engs:
            e.set_world_point_raw(raw_world(w))
    return set_world


@pytest.mark.parametrize("worst", [1.0, 0.25, 0.5], ids=["mean", "max", "tail"])
def test_point_push_commands_with_groups_equal_the_twin(oracle, worst):
    A, B, g = _point_pair(64, 8, 4, False, "push", worst, seed=11)
    try:
        assert A.sample_groups_set() == 15 and B.sample_groups_set() == 0
        _grouped_command_equals_the_twin(A, B, g, worst, _point_worlds(oracle, (A, B)), 3, f"push worst {worst}",
                                         expect_models_differ=True)
    finally:
        A.close(); B.close()


def _plan_constants():
    src = open(os.path.join(ROOT, "m3p2i_aip_amd", "csrc", "update_plan.hpp")).read()
    return {n: int(v) for n, v in re.findall(r"constexpr int (UPDATE_\w+) = (\d+);", src)}


def test_the_three_launch_update_forms_its_own_minima(oracle):
    """the smallest K inside update_large_range for which update_small_applies is false (nu = 2, multi-modal), the shortest T
    the shape checks admit (T = 1 without the filter): m3_command hands the update rollout_minima = false while groups are set"""
    c = _plan_constants()
    K = max(c["UPDATE_LARGE_MIN_K"], c["UPDATE_SMALL_MAX_K_MULTI"]) + 1
    assert K <= c["UPDATE_LARGE_MAX_K"] and K == 8193
    A, B, g = _point_pair(K, 1, 4, True, "push_pull", 1.0, seed=13)
    try:
        _grouped_command_equals_the_twin(A, B, g, 1.0, _point_worlds(oracle, (A, B)), 2, "three-launch update")
    finally:
        A.close(); B.close()


def test_panda_reach_commands_with_groups_equal_the_twin():
    K, T, M, worst = 32, 4, 2, 1.0
    g, model_of = groups.grouped_layout(K, M, False)
    delta = groups.tile_noise(np.random.default_rng(5).standard_normal((K, T, 9)).astype(F), g)
    models = scenes.spread_panda_scenes(M, 0.3, seed=2)
    rows = [models[m] if m >= 0 else None for m in model_of.tolist()]
    engs = []
    for _ in range(2):
        e = HipEngine(make_config(K=K, T=T, nu=9, env_type="panda_env", filter_u=False, **PANDA_PK))
        e.set_objective("reach", PANDA_GOALS["reach"], gripper_cmd=1)
        e.set_noise(delta)
        e.set_panda_rollout_scenes(rows)
        engs.append(e)
    A, B = engs
    try:
        A.set_sample_groups(g, worst)
        w = panda_worlds()["near"]

        def set_world(call):
            for e in engs:
                e.set_world_panda_raw(w)
        _grouped_command_equals_the_twin(A, B, g.astype(np.int64), worst, set_world, 2, "panda reach")
        assert A.panda_lanes_per_sample_used() == B.panda_lanes_per_sample_used()
    finally:
        A.close(); B.close()


# ------------------------------------------------------------------ 3. groups that change nothing
@pytest.mark.parametrize("M", [2, 4, 16, 3])
def test_groups_of_members_in_one_arena_change_nothing(oracle, M):
    """every member of a group in the same (the default) arena with the same controls has the same cost c; with worst_frac = 1
    the aggregate is SUM16(c x M) / M.  M a power of two: the sums and the division are exact, so costs, weights and plan are the
    plain command's bit for bit.  M = 3: (c + c) + c and the division round once each, |dJ| <= 2 * 2^-24 * |J|; a weight
    exp(-(J - Jmin) / lambda) then moves by a relative exp(2 dJ / lambda) - 1 <= 4 dJ / lambda (dJ / lambda << 1) before and as
    much after the normalisation, and the mean is a convex combination of controls within u_max: |d mean| <= 8 u_max dJmax /
    lambda, plus 1e-5 for the binary32 sums of the update itself."""
    A, B, g = _point_pair(64, 8, M, False, "push", 1.0, seed=17, arenas=False)
    try:
        set_world = _point_worlds(oracle, (A, B))
        for call in range(2):
            set_world(call)
            A.command()
            B.command()
            torch.cuda.synchronize()
            if M != 3:
                _compare_outputs(A, B, f"M {M} call {call}")
                assert_same_bits(A.raw_costs(), A.buffer(L.BUF_TRAJ_COST), "raw costs are the costs")
            else:
                J = B.buffer(L.BUF_TRAJ_COST).cpu().numpy().astype(np.float64)
                dJ = 2.0 * 2.0 ** -24 * np.abs(J).max()
                assert np.abs(A.buffer(L.BUF_TRAJ_COST).cpu().numpy() - J).max() <= dJ
                tol = 8.0 * 3.0 * dJ / float(A.cfg.lambda_) + 1e-5
                d = np.abs(A.buffer(L.BUF_MEAN).cpu().numpy().astype(np.float64) - B.buffer(L.BUF_MEAN).cpu().numpy()).max()
                print(f"M 3 call {call}: |d mean| {d:.3g}, bound {tol:.3g}")
                assert d <= tol, (d, tol)
                for which in PLAN_BUFS:      # (the next call starts from the same plan)
                    if buf(A, which) is not None:
                        B.set_plan(which, A.buffer(which).cpu().numpy())
    finally:
        A.close(); B.close()


# ------------------------------------------------------------------ 4. refusals and life cycle
def _refused(eng, code, text, g, worst=1.0):
    with pytest.raises(L.M3Error, match=rf"error {code}: m3_set_sample_groups: {text}"):
        eng.set_sample_groups(g, worst)


def test_refusals_with_their_texts_and_a_refused_call_changes_nothing(oracle):
    K, T = 64, 8
    A, B, g = _point_pair(K, T, 4, False, "push", 0.5, seed=19)
    B.set_sample_groups(g, 0.5)            # (here the twin has the same groups: it never sees a refused call)
    none = np.full(K, -1, np.int64)
    try:
        def state():
            return A.sample_groups_set(), [A.sample_group(k) for k in range(K)]
        before = state()
        pair = none.copy(); pair[[3, 9]] = 5
        _refused(A, -1, "n is 63, must be K_local = 64", none[:63])
        bad = pair.copy(); bad[20] = K
        _refused(A, -1, r"sample 20: group id 64 is outside -1 \.\. K - 1 = 63", bad)
        bad = pair.copy(); bad[20] = -2
        _refused(A, -1, "sample 20: group id -2 is outside", bad)
        bad = pair.copy(); bad[40] = 7
        _refused(A, -1, r"group 7 has 1 member \(sample 40\)", bad)
        bad = none.copy(); bad[1:18] = 2
        _refused(A, -1, "group 2 has 17 members", bad)
        bad = pair.copy(); bad[K - 1] = 5
        _refused(A, -1, "sample 63 is the zero-noise / null-action sample", bad)
        for wf in (0.0, -1.0, 1.5, float("nan")):
            _refused(A, -1, r"worst_frac must be in \(0, 1\]", pair, wf)
        assert state() == before
        # the multi-modal conditions
        mm = HipEngine(make_config(K=K, T=T, nu=2, multi_modal=True, filter_u=False, **PK))
        try:
            bad = pair.copy(); bad[0] = 5
            _refused(mm, -1, "sample 0 is a best-trajectory sample", bad)
            bad = none.copy(); bad[[K // 2, K // 2 + 1]] = 1
            _refused(mm, -1, "sample 32 is a best-trajectory sample", bad)
            bad = none.copy(); bad[[10, 40]] = 3
            _refused(mm, -1, "group 3 has members in both halves", bad)
            assert mm.sample_groups_set() == 0
            mm.set_sample_groups(pair, 1.0)
            assert mm.sample_groups_set() == 1
        finally:
            mm.close()
        # the handles that cannot have groups
        for kw, text in ((dict(K_local=32), "sharded handle"), (dict(sim_only=True), "planner handles only"),
                         (dict(mode_simple=True, sampling_random=True), "mode_simple / sampling_random handle"),
                         (dict(sampling_random=True), "mode_simple / sampling_random handle")):
            e = HipEngine(make_config(K=K, T=T, nu=2, filter_u=False, **{**PK, **kw}))
            try:
                _refused(e, -5, text, none if kw.get("K_local") is None else none[:32])
                assert e.sample_groups_set() == 0
            finally:
                e.close()
        # priors and groups exclude each other, in both orders and both environments
        e = HipEngine(make_config(K=K, T=T, nu=2, filter_u=False, **PK))
        try:
            seqs = np.zeros((2, T, 2), F)
            e.set_prior_samples(seqs, [3, 4])
            _refused(e, -5, "the handle has prior samples or a prior controller", pair)
            e.set_prior_samples(None)
            e.set_prior_controller("go_to", 2, [3, 4])
            _refused(e, -5, "the handle has prior samples or a prior controller", pair)
            e.set_prior_controller(None)
            e.set_sample_groups(pair, 1.0)
            with pytest.raises(L.M3Error, match=r"error -5: m3_set_prior_samples: the handle has sample groups \(m3_set_sample_groups\)"):
                e.set_prior_samples(seqs, [3, 4])
            with pytest.raises(L.M3Error, match=r"error -5: m3_set_prior_controller: the handle has sample groups"):
                e.set_prior_controller("go_to", 2, [3, 4])
            assert e.prior_samples_set() == 0 and e.sample_groups_set() == 1
        finally:
            e.close()
        e = HipEngine(make_config(K=K, T=T, nu=9, env_type="panda_env", filter_u=False, **PANDA_PK))
        try:
            e.set_sample_groups(pair, 1.0)
            with pytest.raises(L.M3Error, match=r"error -5: m3_set_panda_prior_samples: the handle has sample groups"):
                e.set_panda_prior_samples(np.zeros((1, T, 9), F), [3])
            e.set_sample_groups(None)
            e.set_panda_prior_samples(np.zeros((1, T, 9), F), [3])
            _refused(e, -5, "the handle has prior samples or a prior controller", pair)
        finally:
            e.close()
        # the batch refuses the handle and leaves it as it was
        batch = HipBatch(2)
        try:
            with pytest.raises(L.M3Error, match=r"error -5: m3_batch_command: handle 0: it has sample groups \(m3_set_sample_groups\)"):
                batch.command([A])
        finally:
            batch.close()
        assert state() == before
        # ... and after all the refused calls the next commands are the twin's, bit for bit
        set_world = _point_worlds(oracle, (A, B))
        for call in range(2):
            set_world(call)
            A.command(); B.command()
            torch.cuda.synchronize()
            _compare_outputs(A, B, f"after the refused calls, call {call}")
            assert_same_bits(A.raw_costs(), B.raw_costs(), "raw costs")
    finally:
        A.close(); B.close()


def test_null_clears_reset_keeps_and_the_ledger_balances(oracle):
    live = lambda: int(L.load().m3_owned_blocks_live())      # noqa: E731
    start = live()
    K, T = 64, 8
    A, B, g = _point_pair(K, T, 4, False, "push", 1.0, seed=23, set_groups=False)     # B: never any groups
    try:
        with pytest.raises(L.M3Error, match=r"error -4: m3_sample_group_raw_costs: the handle never had sample groups"):
            A.raw_costs()
        set_world = _point_worlds(oracle, (A, B))
        set_world(0)
        A.command(); B.command()      # (lazy blocks of a first command, on both)
        torch.cuda.synchronize()
        _compare_outputs(A, B, "before any groups")
        n0 = live()
        A.set_sample_groups(g, 0.25)
        n1 = live()
        assert n1 > n0                # all of the feature's blocks come with the first setter call ...
        A.set_sample_groups(g, 1.0)
        assert live() == n1           # ... a second takes nothing
        for call in range(10):
            set_world(call)
            A.command()
        torch.cuda.synchronize()
        assert live() == n1           # ... and neither do ten commands
        # the groups survive m3_reset
        A.reset(); B.reset()
        assert A.sample_groups_set() == 15 and A.sample_group(0) == (0, 4, 4) and A.sample_group(K - 1) == (-1, 1, 1)
        set_world(0)
        A.command(); B.command()
        torch.cuda.synchronize()
        assert not np.array_equal(bits(A.buffer(L.BUF_TRAJ_COST)), bits(A.raw_costs()))
        # NULL clears: the next commands are the twin's bit for bit, TRAJ_COST is the rollout's again
        A.set_sample_groups(None)
        assert A.sample_groups_set() == 0 and A.sample_group(0) == (-1, 1, 1) and live() == n1
        A.reset(); B.reset()
        for call in range(2):
            set_world(call)
            A.command(); B.command()
            torch.cuda.synchronize()
            _compare_outputs(A, B, f"after the clear, call {call}")
    finally:
        A.close(); B.close()
    assert live() == start


def test_both_lockstep_episode_sets_refuse_a_planner_with_groups():
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    from tests.test_object_lifetimes_gpu import K, panda_planner, point_planner
    pair = np.full(K, -1, np.int64)
    pair[[3, 9]] = 5
    text = r"planner 1: it has sample groups \(m3_set_sample_groups\), which only m3_rollout / m3_command run"
    # point_env
    sim = IsaacGymWrapper(IsaacGymConfig(dt=0.05), "point_env", num_envs=2)
    world = sim._engine
    planners = [point_planner(seed=10 + i) for i in range(2)]
    spec = [("push", (-3.0, 3.0), 0, L.SUCTION_OFF, 400.0)] * 2
    batch = HipBatch(2)
    try:
        planners[1].set_sample_groups(pair, 1.0)
        for kw in ({}, dict(point_runtime=True), dict(point_priors=True)):
            with pytest.raises(L.M3Error, match=r"error -5: m3_episodes_create: " + text):
                HipEpisodes(world, planners, spec, 4, **kw)
        planners[1].set_sample_groups(None)
        eps = HipEpisodes(world, planners, spec, 4)
        try:
            planners[1].set_sample_groups(pair, 1.0)       # set after create: nothing of the tick is launched
            with pytest.raises(L.M3Error, match=r"error -5: m3_episodes_tick: " + text):
                eps.tick(batch)
            assert eps.ticks_done == 0
            planners[1].set_sample_groups(None)
            eps.tick(batch)
            assert eps.ticks_done == 1
        finally:
            eps.close()
    finally:
        batch.close()
        for e in planners:
            e.close()
        world.close()
    # panda_env
    sim = IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=2)
    world = sim._engine
    planners = [panda_planner(seed=20 + i) for i in range(2)]
    try:
        planners[1].set_sample_groups(pair, 1.0)
        for kw in ({}, dict(panda_runtime=True)):
            with pytest.raises(L.M3Error, match=r"error -5: m3_panda_episodes_create: " + text):
                HipPandaEpisodes(world, planners, max_ticks=4, settle_ticks=0, **kw)
        planners[1].set_sample_groups(None)
        eps = HipPandaEpisodes(world, planners, max_ticks=4, settle_ticks=0)
        try:
            planners[1].set_sample_groups(pair, 1.0)
            with pytest.raises(L.M3Error, match=r"error -5: m3_panda_episodes_observe: " + text):
                eps.observe()
        finally:
            eps.close()
    finally:
        for e in planners:
            e.close()
        world.close()


# ------------------------------------------------------------------ 5. the config key through the planner
def test_the_config_key_through_the_planner():
    """`rollout_arena_groups` on a planner built as tools/closed_loop.py builds it: the groups are set, the planner's K-env
    simulator carries the members' arenas, the noise table is tiled (so no relabelling tears the rows apart), the first command's
    probe finds the step path -- which aggregates through m3_aggregate_sample_groups -- equal to the fused one, later commands
    leave equal controls within every group and the emulated aggregates in cost_total, and command_batch refuses the planner."""
    from m3p2i_aip_amd import compat
    from m3p2i_aip_amd.episodes import _PlannerSide
    from m3p2i_aip_amd.planner import command_batch
    compat.install(force_standins=True)
    cfg = compat.make_config("config_point", ["task=push", "goal=[-1.0, -1.0]", "mppi.num_samples=64", "mppi.horizon=12",
                                              "mppi.u_per_command=12",
                                              "rollout_arena_groups={models: 4, spread: 0.4, seed: 2, worst: 0.5}"])
    t = _PlannerSide(cfg, point_scenes=compat.rollout_point_scenes(cfg))
    try:
        p = t.motion_planner
        g, model_of = groups.grouped_layout(64, 4, False)
        assert p.has_sample_groups and p._engine.sample_groups_set() == 15 and p._fused is None
        assert p._engine.sample_group(16) == (1, 4, 2)
        t.first_plan(t.sim._dof_state[0:1].clone(), t.sim._root_state[0:1].clone())
        print(f"probe {p.probe_result}")
        assert p.probe_result["fused"] is True
        assert p.has_rollout_scenes and p._engine.point_rollout_scenes_set()
        delta = bits(p.delta)                                      # [K][T][nu]
        assert np.array_equal(delta, delta[groups.first_members(g)]) and len(np.unique(delta[:15], axis=0)) == 15
        for call in range(2):
            p.command(t.sim._dof_state[0])
            torch.cuda.synchronize()
            act = bits(p._engine.buffer(L.BUF_ACTIONS))            # [T][K][nu]
            assert np.array_equal(act, act[:, groups.first_members(g), :]), call
            assert_same_bits(p.cost_total, groups.aggregate_reference(p.raw_costs.cpu().numpy(), g, 0.5), f"cost_total, call {call}")
        with pytest.raises(ValueError, match="planner 0 has sample groups"):
            command_batch([p], [t.sim._dof_state[0]])
        p.set_sample_groups(None)
        assert not p.has_sample_groups and p._engine.sample_groups_set() == 0
    finally:
        t.close()
