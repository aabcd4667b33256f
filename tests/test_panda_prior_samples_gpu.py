"""panda_env prior samples on the GPU (m3_set_panda_prior_samples, k_rollout_panda_pr; include/m3p2i_hip.h).

The reference of every rollout is the oracle planner of tests/panda_prior_samples_fixture.py, whose _rollout overwrites the
prior samples' assembled actions with clip(seqs) and re-applies the gripper command to their columns 7 and 8 -- compared as
bits: actions, states, cost_horizon and trajectory costs of EVERY command of a trace, the priors replaced between commands.
The two sides are re-synchronised after each command the way tests/test_resynchronised_traces_gpu.py does it (the oracle's
means, best rows and beta written into the handle through m3_set_plan / m3_set_beta), because two correct updates agree to
~1e-6 in the means and not to the bit -- a reason that predates this feature; what the update leaves (weights, means, the
action) is compared with that test's tolerances for the same quantities: weights rtol 2e-3 / atol 1e-6, plans atol 1e-4, the
best indices equal.  Each case first asserts, on the oracle alone, that every prior sample feels its prior.
Shapes: K = 64 and K = 61 (the ragged last wavefront), T = 20, worlds 41 (reach) and 40 (pick)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd import priors  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, HipPandaEpisodes, make_config  # noqa: E402
from tests import panda_prior_samples_fixture as PF  # noqa: E402
from tests import panda_rollout_scenes_ref as R  # noqa: E402
from tests import panda_scene_fixture as X  # noqa: E402
from tests.test_resynchronised_traces_gpu import assert_rollout_bits, resync  # noqa: E402

F = np.float32
PK = dict(u_min=X.UMIN, u_max=X.UMAX, noise_sigma_diag=X.SIG, lambda_=0.05, pre_height_diff=0.05, dt=0.01)
GOAL = np.array(X.GOAL, F)
COMMAND_BUFS = [L.BUF_STATES, L.BUF_ACTIONS, L.BUF_COST_HORIZON, L.BUF_TRAJ_COST, L.BUF_WEIGHTS, L.BUF_MEAN, L.BUF_ACTION_OUT,
                L.BUF_TOP_IDX, L.BUF_TOP_TRAJS]
MM_BUFS = [L.BUF_MEAN_1, L.BUF_MEAN_2, L.BUF_BEST_1, L.BUF_BEST_2]
ERR_BAD_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5     # (include/m3p2i_hip.h)
TUNED = (("pick_ori", 25.0), ("collision", 500.0), ("pick_goal", 7.5))


@pytest.fixture(scope="module")
def P(oracle):
    import oracle.panda as P
    P.lib()
    return P


def planner_engine(case, K=X.K, mm=False, lps=0, cost_kernel=True, **kw):
    _, task, grip = PF.CASES[case]
    eng = HipEngine(make_config(K=K, T=X.T, nu=9, env_type="panda_env", multi_modal=mm, **{**PK, **kw}))
    eng.set_objective(task, GOAL, gripper_cmd=grip)
    eng.set_panda_lanes_per_sample(lps)
    eng.set_panda_reach_cost_kernel(cost_kernel)
    if not kw.get("sampling_random"):
        eng.set_noise(X.delta_of(K))
    return eng


@functools.lru_cache(maxsize=None)
def guard(P, case, mm, K, rows):
    PF.assert_priors_matter(P, case, mm, K, f"{case} mm {mm} K {K} rows {rows}", rows=R.cycle_rows(case, K) if rows else None)
    return True


def priors_of_call(K, mm, call):
    """the priors of command `call` of a trace: all indices; every other one with new sequences; all, in reverse order"""
    idx = PF.prior_indices(K, mm)
    idx = [idx, idx[1::2], idx[::-1]][call % 3]
    return idx, PF.prior_seqs(len(idx), seed=11 + call)


def assert_update_close(eng, opl, a_hip, a_orc, mm, where):
    """what the update leaves, with the tolerances of tests/test_resynchronised_traces_gpu.py for the same quantities.  Returns
    whether it is finite: the multi-modal update normalises the costs of a half by their range (the reference's), so where
    every sample of a half costs the same -- pick in world 40, whose cost no control moves within the horizon -- the ORACLE's
    weights, means and action are NaN, and the device's must be NaN in the same places (assert_allclose: NaN equals NaN);
    the best indices mean nothing then."""
    finite = bool(np.isfinite(opl.last["w"]).all())
    assert finite or (mm and min(np.ptp(opl.last["J"][:opl.cfg.K // 2]), np.ptp(opl.last["J"][opl.cfg.K // 2:])) == 0.0), where
    np.testing.assert_allclose(eng.buffer(L.BUF_WEIGHTS).cpu().numpy(), opl.last["w"], rtol=2e-3, atol=1e-6, err_msg=where)
    np.testing.assert_allclose(a_hip, a_orc, atol=1e-4, err_msg=where)
    np.testing.assert_allclose(eng.buffer(L.BUF_MEAN).cpu().numpy(), opl.mean, atol=1e-4, err_msg=where)
    i, oi = eng.info(), opl.last["info"]
    if not finite:
        assert np.isnan(a_hip).all() and np.isnan(eng.buffer(L.BUF_WEIGHTS).cpu().numpy()).all(), where
    elif mm:
        assert (i.best_idx_1, i.best_idx_2) == (oi.best_idx_1, oi.best_idx_2 + opl.cfg.K // 2), where
        np.testing.assert_allclose(eng.buffer(L.BUF_MEAN_1).cpu().numpy(), opl.mean1, atol=1e-4, err_msg=where)
        np.testing.assert_allclose(eng.buffer(L.BUF_MEAN_2).cpu().numpy(), opl.mean2, atol=1e-4, err_msg=where)
        # (the best rows are rows of the actions, which are bit-equal: equal bits)
        np.testing.assert_array_equal(eng.buffer(L.BUF_BEST_1).cpu().numpy(), opl.best1, err_msg=where)
        np.testing.assert_array_equal(eng.buffer(L.BUF_BEST_2).cpu().numpy(), opl.best2, err_msg=where)
    else:
        assert i.best_idx == oi.best_idx and i.beta == pytest.approx(opl.beta, rel=1e-6), where
    return finite


def run_trace(P, case, mm=False, K=X.K, lps=1, cost_kernel=True, calls=3, lanes=0, rows=False, scene=None, weights=None,
              update_cov=False):
    assert guard(P, case, mm, K, rows)
    world, task, _ = PF.CASES[case]
    cfg = PF.make_cfg(P, case, K, mm)
    table = R.cycle_rows(case, K) if rows else None
    okw = dict(update_cov=True) if update_cov else {}
    if weights is not None:         # (tuned weights: the stitched planner forms the cost of tests/panda_cost_ref.py)
        from tests import panda_cost_ref as CR
        w = CR.weights(**dict(weights))
        cost = lambda o, kk: CR.cost_of_obs(task, o, goal=GOAL, w=w, multi_modal=mm, half_K=K // 2, k=kk)  # noqa: E731
        opl = PF.make_panda_prior_planner(P, cfg, X.delta_of(K), [], [], rows=table or [None] * K, task=task, cost=cost, **okw)
    elif table is not None:
        opl = PF.make_panda_prior_planner(P, cfg, X.delta_of(K), [], [], rows=table, task=task, **okw)
    else:
        opl = PF.make_panda_prior_planner(P, cfg, X.delta_of(K), [], [], scene=X.oracle_scene(P, scene) if scene else None, **okw)
    eng = planner_engine(case, K, mm, lps, cost_kernel, update_cov=update_cov)
    try:
        if lanes:
            eng.set_rollout_lanes(lanes)
        if weights is not None:
            eng.set_panda_cost_weights(dict(weights))
        if scene:
            eng.set_panda_scene(scene)
        if table is not None:
            eng.set_panda_rollout_scenes(table)
        w0 = X.world_of(world)
        eng.set_world_panda_raw(P.raw57(w0))
        assert eng.panda_prior_samples_used() == -1
        for call in range(calls):
            idx, seqs = priors_of_call(K, mm, call)
            eng.set_panda_prior_samples(seqs, idx)
            opl.set_priors(idx, seqs)
            a_hip, a_orc = eng.command(sync_host=True), opl.command(w0)
            where = f"{case} mm {mm} K {K} lps {lps} cost kernel {cost_kernel} lanes {lanes} rows {rows} call {call}"
            assert eng.panda_prior_samples_set() == len(idx) and eng.panda_prior_samples_used() == 1, where
            assert eng.panda_lanes_per_sample_used() == lps, where
            assert eng.panda_scene_instance_used() and eng.panda_weighted_cost_instance_used() == (weights is not None), where
            assert np.isfinite(eng.states.cpu().numpy()).all()
            assert_rollout_bits(eng, opl, L, where)
            if not assert_update_close(eng, opl, a_hip, a_orc, mm, where):
                # (a NaN plan on both sides: the next command starts from a fresh warm start on both, so that its rollout
                # compares finite numbers)
                for name in ("mean", "mean1", "mean2", "best", "best1", "best2"):
                    getattr(opl, name)[:] = 0.0
            # the stored actions of the prior samples are the clamped sequences under the gripper command (CASES: close, -1.5)
            got = eng.actions.cpu().numpy()[idx]
            assert got[:, :, :7].tobytes() == PF.clip(cfg, seqs)[:, :, :7].tobytes() and (got[:, :, 7:] == F(-1.5)).all(), where
            resync(eng, opl, L)
            if update_cov:          # (the adapted scale is the device's: the oracle takes it over, as the handle takes the means)
                cov = eng.buffer(L.BUF_COV).cpu().numpy()
                np.testing.assert_allclose(cov[1], [opl.cfg.scale_tril[j] for j in range(9)], rtol=1e-4)
                np.testing.assert_allclose(cov[0], opl.cov_action, rtol=1e-4)
                assert np.abs(cov[1] - np.sqrt(np.array(X.SIG, F))).max() > 1e-3           # it did adapt
                opl.cov_action = cov[0].copy()
                for j in range(9):
                    opl.cfg.scale_tril[j] = float(cov[1][j])
    finally:
        eng.close()


# ------------------------------------------------------------------ 1. bit for bit against the oracle with overwritten actions
@pytest.mark.parametrize("K", [X.K, X.K_RAGGED])
@pytest.mark.parametrize("mm", [False, True])
@pytest.mark.parametrize("lps", [1, 8, 16])
def test_pick_traces_in_every_lane_form(P, lps, mm, K):
    run_trace(P, "pick", mm, K, lps)


# reach: quirk Q8 in both realisations -- the shadow slots (the shadow of sample 0 takes sample 0's prior) and the record + the
# reach-cost kernel behind a many-lane rollout (sample 0's record is a prior's)
@pytest.mark.parametrize("K", [X.K, X.K_RAGGED])
@pytest.mark.parametrize("mm", [False, True])
@pytest.mark.parametrize("lps,cost_kernel", [(1, False), (1, True), (8, False), (8, True), (16, False), (16, True)])
def test_reach_traces_in_every_lane_form_and_both_realisations_of_q8(P, lps, cost_kernel, mm, K):
    run_trace(P, "reach", mm, K, lps, cost_kernel)


def test_fewer_samples_per_wavefront_than_the_default(P):
    run_trace(P, "pick", lps=1, lanes=32, calls=2)            # (m3_set_rollout_lanes: a power of two, coprime to 5 too)
    run_trace(P, "reach", lps=16, cost_kernel=False, lanes=2, calls=2)
    run_trace(P, "reach", mm=True, lps=8, cost_kernel=False, lanes=4, calls=2)


def test_update_cov(P):
    run_trace(P, "pick", lps=16, update_cov=True)


def test_tuned_cost_weights(P):
    run_trace(P, "pick", lps=8, weights=TUNED, calls=2)
    run_trace(P, "reach", lps=16, weights=TUNED, calls=2)     # (the weighted reach-cost kernel behind the rollout)


def test_a_workspace_of_its_own(P):
    run_trace(P, "reach", lps=1, cost_kernel=False, scene=X.COMBINED, calls=2)
    run_trace(P, "pick", lps=16, scene=X.COMBINED, calls=2)


@pytest.mark.parametrize("lps,cost_kernel", [(1, False), (8, True), (16, False)])
def test_a_workspace_per_sample_against_the_stitched_planner(P, lps, cost_kernel):
    run_trace(P, "reach", lps=lps, cost_kernel=cost_kernel, rows=True, calls=2)


def test_simple_mode_with_the_random_sampler(P, oracle):
    """mppi_mode simple + the in-kernel sampler (noise mean, full noise_sigma, noise_abs_cost, u_scale 0.9): the prior samples'
    rows do not depend on the noise stream, so their stored actions and their states are the oracle's bits; the rest with the
    tolerances tests/test_hip_parity_panda.py uses for this mode (plans and weights)."""
    from tests.test_oracle_panda import PANDA_MU, PANDA_SIG
    K, T = X.K, X.T
    world, task, grip = PF.CASES["reach"]
    kw = dict(mode_simple=True, u_per_command=T, lambda_=0.05, noise_mu=PANDA_MU, noise_sigma=PANDA_SIG, noise_abs_cost=True, u_scale=0.9)
    cfg = P.make_cfg(K, T, task=task, goal=GOAL, gripper_cmd=0, **kw)
    idx = PF.prior_indices(K)
    opl = PF.make_panda_prior_planner(P, cfg, None, idx, PF.prior_seqs(len(idx)), seed=7)
    eng = HipEngine(make_config(K=K, T=T, nu=9, env_type="panda_env", seed=7, sampling_random=True, **{**PK, **kw}))
    try:
        eng.set_objective(task, GOAL, gripper_cmd=0)
        w0 = X.world_of(world)
        eng.set_world_panda_raw(P.raw57(w0))
        for call in range(2):
            seqs = PF.prior_seqs(len(idx), seed=11 + call)
            eng.set_panda_prior_samples(seqs, idx)
            opl.set_priors(idx, seqs)
            a_hip, a_orc = eng.command(sync_host=True), opl.command(w0)
            assert eng.panda_prior_samples_used() == 1
            got, st = eng.actions.cpu().numpy(), eng.states.cpu().numpy()
            # gripper_cmd 0: the prior's columns 7 and 8 are taken; u_scale multiplies behind the select
            assert got[idx].tobytes() == (PF.clip(cfg, seqs) * F(0.9)).astype(F).tobytes() == opl.last["actions"][idx].tobytes()
            assert st[idx].tobytes() == opl.last["states"][idx].tobytes()
            np.testing.assert_array_equal(eng.cost_horizon.cpu().numpy()[idx], opl.last["cost_h"][idx])
            np.testing.assert_allclose(got, opl.last["actions"], atol=1e-3)
            # simple mode's perturbation cost e - m of a prior sample: its J is the oracle's cost_total up to the update's own
            # arithmetic (the oracle's cost_total carries + mean(S), quirk Q1, which the softmin cancels: compare the weights)
            np.testing.assert_allclose(eng.buffer(L.BUF_WEIGHTS).cpu().numpy(), opl.last["w"], rtol=2e-3, atol=1e-6)
            np.testing.assert_allclose(a_hip[:a_orc.shape[0]], a_orc, atol=1e-3)
            U = eng.buffer(L.BUF_MEAN).cpu().numpy().copy()   # (every call starts from the same U on both sides)
            opl.U = U
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. byte for byte against a twin on the forced run-time instances
@pytest.mark.parametrize("case,mm,lps,cost_kernel", [("pick", False, 1, True), ("pick", True, 8, True), ("reach", False, 16, True),
                                                     ("reach", True, 1, False), ("reach", False, 8, False)])
def test_priors_that_repeat_the_twins_own_rows_give_the_twins_bytes(P, case, mm, lps, cost_kernel):
    """a: priors; b: no priors, both run-time instances forced on (k_rollout_panda_w: the parent's code object).  Each command b
    runs first and a's priors are b's own stored rows of those samples: every output buffer of three commands, byte for byte"""
    K = X.K
    idx = PF.prior_indices(K, mm)
    a, b = planner_engine(case, K, mm, lps, cost_kernel), planner_engine(case, K, mm, lps, cost_kernel)
    try:
        b.set_panda_scene_instance(1)
        b.set_panda_weighted_cost_instance(1)
        for e in (a, b):
            e.set_world_panda_raw(P.raw57(X.world_of(PF.CASES[case][0])))
        for call in range(3):
            pb = b.command(sync_host=True)
            a.set_panda_prior_samples(b.actions.cpu().numpy()[idx].copy(), idx)      # (u_scale 1: the stored rows are the controls)
            pa = a.command(sync_host=True)
            assert a.panda_prior_samples_used() == 1 and b.panda_prior_samples_used() == 0
            assert a.panda_scene_instance_used() and b.panda_scene_instance_used()
            assert not a.panda_weighted_cost_instance_used() and b.panda_weighted_cost_instance_used()
            assert a.panda_lanes_per_sample_used() == b.panda_lanes_per_sample_used() == lps
            assert np.asarray(pa).tobytes() == np.asarray(pb).tobytes(), call
            for buf in COMMAND_BUFS + (MM_BUFS if mm else []):
                assert a.buffer(buf).cpu().numpy().tobytes() == b.buffer(buf).cpu().numpy().tobytes(), (call, buf)
            assert bytes(a.info()) == bytes(b.info()), call
        assert np.ptp(a.states.cpu().numpy(), axis=0).max() > 0 and np.ptp(a.cost_horizon.cpu().numpy()) > 0
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------ 3. the device entry point
def test_the_device_entry_point_gives_the_host_entry_points_results(P):
    K = X.K
    idx = PF.prior_indices(K)
    a, b = planner_engine("pick", K, lps=8), planner_engine("pick", K, lps=8)
    try:
        for e in (a, b):
            e.set_world_panda_raw(P.raw57(X.world_of(40)))
        for call in range(2):
            seqs = PF.prior_seqs(len(idx), seed=11 + call)
            a.set_panda_prior_samples(seqs, idx)
            b.set_panda_prior_samples(torch.from_numpy(seqs).to(b.device), idx)
            pa, pb = a.command(sync_host=True), b.command(sync_host=True)
            assert np.asarray(pa).tobytes() == np.asarray(pb).tobytes(), call
            for buf in COMMAND_BUFS:
                assert a.buffer(buf).cpu().numpy().tobytes() == b.buffer(buf).cpu().numpy().tobytes(), (call, buf)
        k, seq = a.panda_prior_sample(3)
        assert k == idx[3] and seq.tobytes() == seqs[3].tobytes()
        kk = C.c_int()
        out = np.empty((X.T, 9), F)
        assert b.lib.m3_get_panda_prior_sample(b._h, 3, C.byref(kk), None) == 0 and kk.value == idx[3]
        assert b.lib.m3_get_panda_prior_sample(b._h, 3, C.byref(kk), out.ctypes.data) == ERR_STATE      # (device-set: no host values)
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------ 4. life cycle
def test_life_cycle_set_replace_clear(P):
    """set, replace with other indices, clear: the handle is back on the kernels it ran before -- its bytes are those of a
    handle that never had priors -- and the getters report the state"""
    K = X.K
    a, plain = planner_engine("reach", K, lps=16), planner_engine("reach", K, lps=16)
    try:
        for e in (a, plain):
            e.set_world_panda_raw(P.raw57(X.world_of(41)))
        assert a.panda_prior_samples_set() == 0 and a.panda_prior_samples_used() == -1
        pa, pp = a.command(sync_host=True), plain.command(sync_host=True)
        assert a.panda_prior_samples_used() == 0 and not a.panda_scene_instance_used()
        assert np.asarray(pa).tobytes() == np.asarray(pp).tobytes()
        idx = PF.prior_indices(K)
        seqs = PF.prior_seqs(len(idx))
        a.set_panda_prior_samples(seqs, idx)
        assert a.panda_prior_samples_set() == len(idx)
        for j in (0, 5, len(idx) - 1):
            k, s = a.panda_prior_sample(j)
            assert k == idx[j] and s.tobytes() == seqs[j].tobytes()
        with pytest.raises(L.M3Error):
            a.panda_prior_sample(len(idx))
        first = a.command(sync_host=True)
        assert a.panda_prior_samples_used() == 1 and a.panda_scene_instance_used()
        assert np.asarray(first).tobytes() != np.asarray(plain.command(sync_host=True)).tobytes()       # the priors show
        other = [3, 7, 11]
        a.set_panda_prior_samples(seqs[:3], other)
        assert a.panda_prior_samples_set() == 3 and [a.panda_prior_sample(j)[0] for j in range(3)] == other
        a.command(sync_host=True)
        got = a.actions.cpu().numpy()
        assert got[other, :, :7].tobytes() == np.clip(seqs[:3, :, :7], -2, 2).tobytes()
        assert got[5, :, :7].tobytes() != np.clip(seqs[1, :, :7], -2, 2).tobytes()                     # the old slots are gone
        a.reset()
        assert a.panda_prior_samples_set() == 3                                                         # survives m3_reset
        a.set_panda_prior_samples(None)
        assert a.panda_prior_samples_set() == 0
        with pytest.raises(L.M3Error):
            a.panda_prior_sample(0)
        # cleared: from the same warm start the bytes of the handle that never had priors, on the kernels from before
        plain.reset()
        for e in (a, plain):
            e.set_world_panda_raw(P.raw57(X.world_of(41)))
        for call in range(2):
            pa, pp = a.command(sync_host=True), plain.command(sync_host=True)
            assert a.panda_prior_samples_used() == 0 and not a.panda_scene_instance_used()
            assert np.asarray(pa).tobytes() == np.asarray(pp).tobytes(), call
            for buf in COMMAND_BUFS:
                assert a.buffer(buf).cpu().numpy().tobytes() == plain.buffer(buf).cpu().numpy().tobytes(), (call, buf)
        # the point entry points keep refusing the arm
        with pytest.raises(L.M3Error, match="m3_set_prior_samples: point_env only"):
            a.set_prior_samples(seqs, idx)
        assert a.prior_samples_set() == 0
    finally:
        a.close(); plain.close()


# ------------------------------------------------------------------ 5. refusals: every check before any state changes
def test_refusals_of_the_setter(P):
    K, T = X.K, X.T
    eng = planner_engine("pick", K)
    mm = planner_engine("reach", K, mm=True)
    shard = HipEngine(make_config(K=K, T=T, nu=9, env_type="panda_env", K_local=32, k_offset=32, **PK))
    world = HipEngine(make_config(K=K, T=1, nu=9, env_type="panda_env", dt=0.01, sim_only=True, filter_u=False))
    pt = HipEngine(make_config(K=64, T=10, nu=2, env_type="point_env"))
    try:
        eng.set_world_panda_raw(P.raw57(X.world_of(40)))
        keep_idx, keep = [4, 9], PF.prior_seqs(2)
        eng.set_panda_prior_samples(keep, keep_idx)
        eng.command(sync_host=True)
        calls, J = eng.info().calls, eng.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes()
        s3 = PF.prior_seqs(3)
        bad = s3.copy()
        bad[1, 2, 3] = np.nan
        who = "m3_set_panda_prior_samples"
        for e, seqs, idx, msg in ((eng, s3, [1, 2, K - 1], "prior 2: sample 63 is the zero-noise / null-action sample K_global - 1"),
                                  (eng, s3, [1, 2, K], "prior 2: sample 64 is outside 0 .. K_global - 1 = 63"),
                                  (eng, s3, [1, -1, 2], "prior 1: sample -1 is outside"),
                                  (eng, s3, [1, 17, 17], "prior 2: sample 17 listed twice"),
                                  (eng, bad, [1, 2, 3], "prior 1: step 2 control 3 is not finite"),
                                  (eng, PF.prior_seqs(257), list(range(257)), "n is 257, must be in 0 .. 256"),
                                  (mm, s3, [1, 0, 2], "prior 1: sample 0 is a best-trajectory sample"),
                                  (mm, s3, [1, 2, K // 2], "prior 2: sample 32 is a best-trajectory sample"),
                                  (shard, s3, [33, 34, 35], "sharded handle"),
                                  (world, np.zeros((3, 1, 9), F), [1, 2, 3], "planner handles only")):
            with pytest.raises(L.M3Error, match=f"{who}: {msg}"):
                e.set_panda_prior_samples(seqs, idx)
            assert e.panda_prior_samples_set() == (2 if e is eng else 0)
        arr = (C.c_int * 3)(1, 2, 3)
        # (the device variant: the same checks but the values'; its own name in the message)
        with pytest.raises(L.M3Error, match="m3_set_panda_prior_samples_device: prior 2: sample 17 listed twice"):
            eng.set_panda_prior_samples(torch.from_numpy(s3).to(eng.device), [1, 17, 17])
        assert eng.lib.m3_set_panda_prior_samples(eng._h, s3.ctypes.data, None, 3) == ERR_BAD_ARG
        assert eng.lib.m3_set_panda_prior_samples(shard._h, s3.ctypes.data, arr, 3) == ERR_UNSUPPORTED
        assert eng.lib.m3_set_panda_prior_samples(world._h, s3.ctypes.data, arr, 3) == ERR_STATE
        # a point_env handle: "panda_env only", from all three entry points that take a handle's kind
        p2 = np.zeros((3, 10, 9), F)
        with pytest.raises(L.M3Error, match="m3_set_panda_prior_samples: panda_env only"):
            pt._ck(pt.lib.m3_set_panda_prior_samples(pt._h, p2.ctypes.data, arr, 3))
        with pytest.raises(L.M3Error, match="m3_set_panda_prior_samples_device: panda_env only"):
            pt._ck(pt.lib.m3_set_panda_prior_samples_device(pt._h, p2.ctypes.data, arr, 3))
        assert pt.lib.m3_set_panda_prior_samples(pt._h, p2.ctypes.data, arr, 3) == ERR_UNSUPPORTED
        assert pt.lib.m3_get_panda_prior_sample(pt._h, 0, None, None) == ERR_UNSUPPORTED and pt.lib.m3_panda_prior_samples_set(pt._h) == 0
        # the handle is as it was: its priors, its results, and the next command runs with them
        assert [eng.panda_prior_sample(j)[0] for j in range(2)] == keep_idx and eng.panda_prior_sample(1)[1].tobytes() == keep[1].tobytes()
        torch.cuda.synchronize()
        assert eng.info().calls == calls and eng.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes() == J
        # a switch forced off with priors set: the next rollout is refused (M3_ERR_STATE), nothing runs
        for force, name in ((eng.set_panda_scene_instance, "m3_set_panda_scene_instance 0"),
                            (eng.set_panda_weighted_cost_instance, "m3_set_panda_weighted_cost_instance 0")):
            force(0)
            for run in (eng.command, eng.rollout):
                with pytest.raises(L.M3Error, match=f"forced off .{name}. but the handle has prior samples .m3_set_panda_prior_samples."):
                    run()
            assert eng.lib.m3_rollout(eng._h) == ERR_STATE
            force(-1)
        torch.cuda.synchronize()
        assert eng.info().calls == calls and eng.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes() == J
        eng.command(sync_host=True)
        assert eng.info().calls == calls + 1 and eng.panda_prior_samples_used() == 1
    finally:
        for e in (eng, mm, shard, world, pt):
            e.close()


@pytest.mark.parametrize("runtime", [False, True])
def test_batch_refuses_a_handle_with_priors_and_then_works_without_it(P, runtime):
    engs = [planner_engine("pick", X.K) for _ in range(3)]
    batch = HipBatch(3, panda_runtime=runtime)
    try:
        for e in engs:
            e.set_world_panda_raw(P.raw57(X.world_of(40)))
        batch.command(engs)
        torch.cuda.synchronize()
        engs[1].set_panda_prior_samples(PF.prior_seqs(2), [4, 9])
        before = [e.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes() for e in engs]
        infos = [bytes(e.info()) for e in engs]
        with pytest.raises(L.M3Error, match="m3_batch_command: handle 1: it has prior samples .m3_set_panda_prior_samples."):
            batch.command(engs)
        assert engs[0].lib.m3_batch_command(batch._b, (C.c_void_p * 3)(*[e._h.value for e in engs]), 3, None) == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert [e.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes() for e in engs] == before
        assert [bytes(e.info()) for e in engs] == infos                      # nothing was launched
        batch.command([engs[0], engs[2]])                                    # the same batch without that handle
        torch.cuda.synchronize()
        assert engs[0].info().calls == 2 and engs[2].info().calls == 2 and engs[1].info().calls == 1
        engs[1].set_panda_prior_samples(None)                                # ... and with it again, once its priors are cleared
        batch.command(engs)
        torch.cuda.synchronize()
        assert [e.info().calls for e in engs] == [3, 2, 3]
    finally:
        batch.close()
        for e in engs:
            e.close()


@pytest.mark.parametrize("runtime", [False, True])
def test_panda_episodes_refuse_a_planner_with_priors(P, runtime):
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    n = 2
    world = IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=n, device="cuda:0")
    planners = [planner_engine("reach", X.K) for _ in range(n)]
    try:
        for e in planners:
            e.set_action_out(torch.zeros(X.T, 9, device="cuda:0"))
        planners[1].set_panda_prior_samples(PF.prior_seqs(2), [4, 9])
        with pytest.raises(L.M3Error, match="m3_panda_episodes_create(_ex)?: planner 1: it has prior samples .m3_set_panda_prior_samples."):
            HipPandaEpisodes(world._engine, planners, max_ticks=4, panda_runtime=runtime)
        planners[1].set_panda_prior_samples(None)
        eps = HipPandaEpisodes(world._engine, planners, max_ticks=4, panda_runtime=runtime)
        try:
            planners[0].set_panda_prior_samples(PF.prior_seqs(2), [4, 9])    # set after create: the tick is refused, not run
            infos = [bytes(e.info()) for e in planners]
            with pytest.raises(L.M3Error, match="m3_panda_episodes_observe: planner 0: it has prior samples .m3_set_panda_prior_samples."):
                eps.observe()
            rb = C.POINTER(C.c_float)()
            assert eps.lib.m3_panda_episodes_observe(eps._eps, C.byref(rb)) == ERR_UNSUPPORTED
            assert eps.lib.m3_panda_episodes_act_first(eps._eps, (C.c_void_p * n)(), (C.c_int * n)()) == ERR_UNSUPPORTED
            torch.cuda.synchronize()
            assert [bytes(e.info()) for e in planners] == infos and planners[0].panda_prior_samples_set() == 2
            planners[0].set_panda_prior_samples(None)
            eps.observe()                                                     # ... and runs once they are cleared
        finally:
            eps.close()
    finally:
        world.stop_sim()
        for e in planners:
            e.close()


# ------------------------------------------------------------------ 6. a winning prior
def test_a_joint_go_to_prior_the_oracle_ranks_lowest_wins_the_weights(P):
    """reach, world 41: of joint_go_to towards the joints that put the finger tips at the goal point / at the cube, the
    candidate whose rollout the ORACLE costs lowest -- lower than every sampled rollout.  On the device its sample gets the
    largest weight and the mean, which starts at zero, moves toward it in one command."""
    K, T, k = X.K, X.T, 23
    w0 = X.world_of(41)
    cfg = PF.make_cfg(P, "reach", K)
    best = None
    for point in (X.GOAL[:3], w0[P.W_CUBEA:P.W_CUBEA + 3]):
        seq = priors.joint_go_to(w0[:9], PF.joints_that_reach(P, w0[:9], point), T, 0.01, X.UMAX, speeds=(1.0,))
        opl = PF.make_panda_prior_planner(P, cfg, X.delta_of(K), [k], seq)
        opl.command(w0)
        if best is None or opl.last["J"][k] < best[1].last["J"][k]:
            best = (seq, opl)
    seq, opl = best
    J = opl.last["J"]
    assert J[k] < np.delete(J, k).min() and int(np.argmax(opl.last["w"])) == k                     # the oracle's word
    eng = planner_engine("reach", K)
    try:
        eng.set_world_panda_raw(P.raw57(w0))
        eng.set_panda_prior_samples(seq, [k])
        eng.command(sync_host=True)
        w = eng.buffer(L.BUF_WEIGHTS).cpu().numpy()
        assert int(np.argmax(w)) == k and w[k] > 2.0 * np.delete(w, k).max()
        mean = eng.buffer(L.BUF_MEAN).cpu().numpy()
        want = eng.actions.cpu().numpy()[k]
        assert np.linalg.norm(mean - want) < 0.75 * np.linalg.norm(want)                           # (the distance of the zero mean)
        # ... and without the prior it does not: the mean of the plain handle stays further away
        eng.reset()
        eng.set_panda_prior_samples(None)
        eng.set_world_panda_raw(P.raw57(w0))
        eng.command(sync_host=True)
        assert np.linalg.norm(eng.buffer(L.BUF_MEAN).cpu().numpy() - want) > np.linalg.norm(mean - want)
    finally:
        eng.close()


# ------------------------------------------------------------------ 7. commands allocate nothing because of priors
def test_commands_with_priors_leave_the_ledger_alone(P):
    """m3_command with priors set, m3_enable_timing off: the ledger's block count between the second and the tenth command
    (the setter's blocks -- table, slot map, pinned mirror, event -- come with its first call, not with a command)"""
    K = X.K
    idx = PF.prior_indices(K)
    eng = planner_engine("reach", K)
    try:
        lib = eng.lib
        eng.enable_timing(False)
        eng.set_world_panda_raw(P.raw57(X.world_of(41)))
        before = lib.m3_owned_blocks_live()
        eng.set_panda_prior_samples(PF.prior_seqs(len(idx)), idx)
        assert lib.m3_owned_blocks_live() == before + 4
        live = None
        for call in range(10):
            if call % 3 == 1:                                        # (replaced now and then: the setter reuses its blocks)
                eng.set_panda_prior_samples(PF.prior_seqs(len(idx), seed=20 + call), idx[::-1] if call % 2 else idx)
            eng.command()
            if call == 1:
                live = lib.m3_owned_blocks_live()
            elif call > 1:
                assert lib.m3_owned_blocks_live() == live, call
        torch.cuda.synchronize()
        assert live == before + 4 and eng.panda_prior_samples_used() == 1
    finally:
        eng.close()


# ------------------------------------------------------------------ 8. Python end to end
@pytest.mark.parametrize("task,mm", [("reach", True), ("pick", False)])
def test_planner_probe_finds_fused_equal_to_step_with_priors(P, task, mm):
    """MPPI.set_panda_prior_samples ahead of the first command of a fused='auto' planner: the probe runs the fused rollout and
    the step path (_write_priors: clamp, then the gripper command) and finds 0 difference; then both paths forced"""
    from tests.test_planner_api_panda_gpu import Tamp, make_cfg
    K, T = X.K, X.T
    idx = PF.prior_indices(K, mm)
    seqs = PF.prior_seqs(len(idx))
    plans = {}
    for fused in (None, True, False):
        tamp = Tamp(make_cfg(K, T, mm, fused))
        try:
            pl = tamp.motion_planner
            pl.set_noise(X.delta_of(K).copy())
            pl.update_gripper_command(task)
            tamp.objective.update_objective(task, torch.tensor(list(X.GOAL)))
            with pytest.raises(ValueError, match="point_env only"):
                pl.set_prior_samples(seqs, idx)
            pl.set_panda_prior_samples(seqs, idx)
            assert pl.has_prior_samples
            a = pl.command(tamp.sim._dof_state[0])
            assert torch.isfinite(a).all()
            if fused is None:
                assert pl.probe_result["fused"] is True and pl.probe_result["max_abs_diff"] == 0.0
            if fused is not False:
                assert pl._engine.panda_prior_samples_used() == 1
            got = pl._engine.actions.cpu().numpy()[idx]
            grip = 1.5 if task == "reach" else -1.5                   # (update_gripper_command: reach opens, pick closes)
            assert got[:, :, :7].tobytes() == np.clip(seqs[:, :, :7], -2, 2).tobytes() and (got[:, :, 7:] == F(grip)).all()
            plans[fused] = a.cpu().numpy().copy()
            if fused is not False:                                    # (a step-mode planner is refused for that, first)
                from m3p2i_aip_amd.planner import command_batch
                with pytest.raises(ValueError, match=r"planner 0 has prior samples \(set_panda_prior_samples\)"):
                    command_batch([pl], [tamp.sim._dof_state[0]], panda_runtime=True)
            pl.set_panda_prior_samples(None)
            assert not pl.has_prior_samples and pl._engine.panda_prior_samples_set() == 0
        finally:
            tamp.sim.stop_sim()
    assert plans[None].tobytes() == plans[True].tobytes()
    np.testing.assert_allclose(plans[False], plans[True], atol=1e-4)
