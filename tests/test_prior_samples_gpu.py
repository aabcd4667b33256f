"""Prior samples (m3_set_prior_samples) on the GPU: the fused rollout and the command of a planner handle some of whose samples
take the caller's control sequences, against the CPU oracle planner that overwrites those samples' actions before it rolls out
(tests/prior_samples_fixture.py), bit for bit where the single custom arena is held bit for bit (tests/test_point_scene_gpu.py);
priors that repeat what the planner would assemble anyway against a twin handle on the forced run-time-scene instance, byte for
byte; the combinations with an arena per sample, tuned weights, avoid_dyn_obs, simple mode and update_cov; fused versus step;
the life cycle, every refusal, and the device entry point.  Every rollout case first asserts, on the oracle alone, that each
prior sample differs from the run without priors and from what its neighbour's sequence would give."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd import priors as A  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, make_config  # noqa: E402
from tests import point_scene_fixture as X  # noqa: E402
from tests import prior_samples_fixture as P  # noqa: E402
from tests import rollout_scenes_fixture as R  # noqa: E402
from tests.test_batch_command_gpu import BUFS, PK, Twin, _noise  # noqa: E402
from tests.test_hip_parity_point import raw_world  # noqa: E402
from tests.test_point_scene_gpu import TASKS, W_TUNED, _assert_rollout_bits  # noqa: E402

F = np.float32
BAD_ARG, STATE, UNSUPPORTED = -1, -4, -5


def _pair(oracle, task, mm, K, idx=None, seqs=None, rows=None, T=X.T, eng_kw=None, opl_kw=None, **kw):
    """(HIP engine with the priors set, oracle planner with the same priors): the same config, noise table, objective"""
    kw = kw or dict(filter_u=False)
    idx = P.prior_indices(K, mm) if idx is None else idx
    seqs = P.prior_seqs(len(idx), T) if seqs is None else seqs
    delta = X.actions(K, T)
    opl = P.make_prior_planner(oracle, oracle.make_cfg(K, T, 2, task=task, goal=X.GOAL, multi_modal=mm, **kw), delta, idx, seqs,
                               rows=rows, **(opl_kw or {}))
    eng = HipEngine(make_config(K=K, T=T, nu=2, multi_modal=mm, **kw, **(eng_kw or {}), **PK))
    eng.set_objective(task, X.GOAL)
    eng.set_noise(delta)
    if rows is not None:
        eng.set_point_rollout_scenes(rows)
    eng.set_prior_samples(seqs, idx)
    return eng, opl


def _plan_of(eng, task, mm, K, scene):
    out = (C.c_int * 9)()
    assert eng.lib.m3_point_rollout_plan_ex(L.TASKS[task], int(mm), 0, 0, 0, K, eng.cfg.T, 64, 0.05, 2, 6, 0, scene, 0, 0,
                                            int(eng.prior_samples_set() > 0), out) == 0
    return list(out)


# ------------------------------------------------------------------ 1: fused rollout vs the oracle planner with priors
@pytest.mark.parametrize("K", [64, 100])
@pytest.mark.parametrize("task,mm", TASKS)
def test_rollout_with_priors_equals_the_oracle(oracle, task, mm, K):
    eng, _ = _pair(oracle, task, mm, K)
    try:
        assert eng.prior_samples_set() == len(P.prior_indices(K, mm)) and eng.prior_samples_used() == -1
        for wi, w0 in enumerate(X.start_worlds(oracle)):
            label = f"{task} K={K} world {X.WORLD_NAMES[wi]}"
            P.assert_priors_matter(oracle, task, mm, K, w0, label)
            opl = P.make_prior_planner(oracle, oracle.make_cfg(K, X.T, 2, task=task, goal=X.GOAL, multi_modal=mm, filter_u=False),
                                       X.actions(K, X.T), P.prior_indices(K, mm), P.prior_seqs(len(P.prior_indices(K, mm))))
            eng.reset()
            eng.set_world_point_raw(raw_world(w0))
            eng.command(sync_host=True)
            opl.command(w0)
            _assert_rollout_bits(eng, opl, label)
            assert eng.prior_samples_used() == 1
        assert _plan_of(eng, task, mm, K, 1)[:5] + [_plan_of(eng, task, mm, K, 1)[8]] == [-1, 0, 0, 1, 1, 1]
    finally:
        eng.close()


# ------------------------------------------------------------------ 2: the two- and three-wave builds
# (the smallest sizes the launch rule sends to the occ2 / occ3 builds with one sample per wavefront: tests/test_point_scene_gpu.py)
@pytest.mark.parametrize("K,build", [(1025, "occ2"), (4097, "occ3")])
def test_rollout_through_the_two_and_three_wave_builds(oracle, K, build):
    w0 = X.start_worlds(oracle)[2]
    P.assert_priors_matter(oracle, "push", False, K, w0, f"{build} K={K}")
    eng, opl = _pair(oracle, "push", False, K)
    try:
        eng.set_rollout_lanes(1)
        eng.set_world_point_raw(raw_world(w0))
        eng.command(sync_host=True)
        opl.command(w0)
        _assert_rollout_bits(eng, opl, f"{build} K={K}")
        assert eng.prior_samples_used() == 1
    finally:
        eng.close()


# ------------------------------------------------------------------ 3: GPU against GPU
@pytest.mark.parametrize("task,mm", TASKS)
def test_priors_that_repeat_the_assembled_rows_are_the_plain_command(oracle, task, mm):
    """before each of three warm-started commands the priors are set to the rows oracle.assemble_actions yields for their
    indices from the handle's means and best rows: every buffer then equals, byte for byte, that of a twin without priors on
    the forced run-time-scene instance"""
    K = 100
    idx = P.prior_indices(K, mm)
    t = Twin(0, K=K, T=X.T, task=task, goal=X.GOAL, multi_modal=mm, filter_u=False)
    ocfg = oracle.make_cfg(K, X.T, 2, task=task, goal=X.GOAL, multi_modal=mm, filter_u=False)
    delta = _noise(K, X.T, 100).astype(F)
    delta[-1] = 0.0
    try:
        t.B.set_point_scene_instance(1)
        for c in range(3):
            t.set_world(c)
            torch.cuda.synchronize()
            m = {b: t.A.buffer(b).cpu().numpy() for b in (L.BUF_MEAN, L.BUF_MEAN_1, L.BUF_MEAN_2, L.BUF_BEST_1, L.BUF_BEST_2)}
            sh = oracle.shift
            act = oracle.assemble_actions(ocfg, delta, sh(m[L.BUF_MEAN]), sh(m[L.BUF_MEAN_1]), sh(m[L.BUF_MEAN_2]),
                                          sh(m[L.BUF_BEST_1]), sh(m[L.BUF_BEST_2]))
            t.A.set_prior_samples(act[idx], idx)
            t.A.command()
            t.B.command()
            torch.cuda.synchronize()
            assert t.assert_same(f"{task} call {c}") == c + 1
            assert t.A.prior_samples_used() == 1 and t.B.prior_samples_used() == 0
    finally:
        t.close()


# ------------------------------------------------------------------ 4: commands vs the oracle planner
@pytest.mark.parametrize("task,mm", [("push", False), ("push_pull", True)])
def test_three_commands_with_fresh_priors_vs_the_oracle_planner(oracle, task, mm):
    """the figures of tests/test_point_scene_gpu.py::test_three_commands_in_the_custom_arena_vs_the_oracle_planner: control output
    atol 1e-3 on every command, the first command's rollout bit for bit and mean atol 1e-4, weights rtol 2e-3 atol 1e-6 with
    frac 0 on the first command and 0.01, cap 1e-3 afterwards.  push_pull: one prior in each half."""
    from tests.conftest import assert_close_but_few
    K, T = 256, 12
    idx = [K // 2 - 3, K // 2 + 5] if mm else P.prior_indices(K)
    w0 = X.start_worlds(oracle)[2].copy()
    P.assert_priors_matter(oracle, task, mm, K, w0, f"{task} K={K} T={T}", T=T, idx=idx, filter_u=True)
    eng, opl = _pair(oracle, task, mm, K, idx=idx, seqs=P.prior_seqs(len(idx), T, seed=20), T=T, filter_u=True)
    try:
        for call in range(3):
            w0[0] += 0.02 * call
            seqs = P.prior_seqs(len(idx), T, seed=20 + call)
            eng.set_prior_samples(seqs, idx)
            opl.set_priors(idx, seqs)
            eng.set_world_point_raw(raw_world(w0))
            a_hip = eng.command(sync_host=True)
            a_orc = opl.command(w0)
            np.testing.assert_allclose(a_hip[:a_orc.shape[0]], a_orc, atol=1e-3, err_msg=f"call {call}")
            assert_close_but_few(eng.buffer(L.BUF_WEIGHTS).cpu().numpy(), opl.last["w"], rtol=2e-3, atol=1e-6,
                                 frac=0.0 if call == 0 else 0.01, cap=1e-3, err_msg=f"call {call} weights")
            np.testing.assert_array_equal(eng.actions.cpu().numpy()[idx].view(np.uint32), P.clip(opl.cfg, seqs).view(np.uint32))
            if call == 0:
                _assert_rollout_bits(eng, opl, "first command")
                if not mm:
                    np.testing.assert_allclose(eng.buffer(L.BUF_MEAN).cpu().numpy(), opl.mean, atol=1e-4)
    finally:
        eng.close()


# ------------------------------------------------------------------ 5: the prior follows the sample, not the slot
@pytest.mark.parametrize("how", ["wave_order", "relabel", "lanes"])
def test_priors_follow_the_sample(oracle, how):
    K = 256 if how != "lanes" else 100      # (the wavefront order is formed from K_local = 128 on)
    w0 = X.start_worlds(oracle)[2]
    P.assert_priors_matter(oracle, "push", False, K, w0, f"{how} K={K}")
    eng, opl = _pair(oracle, "push", False, K)
    try:
        if how == "lanes":
            eng.set_rollout_lanes(16)
        else:
            eng.set_wave_order(True)
        if how == "relabel":
            eng.relabel_samples()
        eng.set_world_point_raw(raw_world(w0))
        eng.command(sync_host=True)
        if how == "relabel":
            # (the rollout permuted the noise rows once: the oracle gets the permuted table; the priors keep their indices)
            table = eng.buffer(L.BUF_NOISE).cpu().numpy()               # [T][K][nu]
            opl.delta = np.ascontiguousarray(table.transpose(1, 0, 2)).astype(F)
            assert opl.delta.tobytes() != X.actions(K, X.T).tobytes() and eng.wave_order() is None
            opl.delta[-1] = 0.0
        else:
            assert (eng.wave_order() is not None) == (how == "wave_order")
        opl.command(w0)
        _assert_rollout_bits(eng, opl, how)
        np.testing.assert_array_equal(eng.actions.cpu().numpy()[opl.prior_idx].view(np.uint32),
                                      P.clip(opl.cfg, opl.prior_seqs).view(np.uint32))
    finally:
        eng.close()


# ------------------------------------------------------------------ 6: combinations
def test_priors_with_an_arena_per_sample(oracle):
    K = 100
    w0 = X.start_worlds(oracle)[2]
    rows = R.cycle_rows(K)
    P.assert_priors_matter(oracle, "push", False, K, w0, "rows K=100", rows=rows)
    R.assert_rows_matter(oracle, "push", False, K, w0, "rows K=100")
    eng, opl = _pair(oracle, "push", False, K, rows=rows)
    try:
        eng.set_world_point_raw(raw_world(w0))
        eng.command(sync_host=True)
        opl.command(w0)
        _assert_rollout_bits(eng, opl, "priors + rows")
        assert _plan_of(eng, "push", False, K, 2)[4] == 2 and eng.prior_samples_used() == 1
        # the rows cleared: the priors on the single scene
        eng.set_point_rollout_scenes(None)
        eng.reset()
        eng.command(sync_host=True)
        opl2 = P.make_prior_planner(oracle, oracle.make_cfg(K, X.T, 2, task="push", goal=X.GOAL, filter_u=False), X.actions(K, X.T),
                                    opl.prior_idx, opl.prior_seqs)
        opl2.command(w0)
        _assert_rollout_bits(eng, opl2, "priors, rows cleared")
    finally:
        eng.close()


def test_priors_with_tuned_cost_weights(oracle):
    """Tuned weights leave the states and actions (which do not depend on the cost) at the oracle's bits.  The oracle has no cost
    weights; the reference of the tuned costs is the weighted default-arena kernel of a handle WITHOUT priors (which
    tests/test_cost_weights_* hold to the numpy restatement) that rolls out the same actions: the priors are fl32(d * scale_tril)
    of rows d, the reference's noise table carries d in those rows, and on the first command (zero mean) its action is
    clamp(0 + d * scale_tril).  Every sample's costs, the prior samples' included, are then its bytes."""
    K = 64
    w0 = X.start_worlds(oracle)[2]
    idx = P.prior_indices(K)
    d = (P.prior_seqs(len(idx), seed=9) * F(0.6)).astype(F)
    seqs = (d * np.sqrt(F(PK["noise_sigma_diag"][0]))).astype(F)          # (one f32 product, as the kernel forms it)
    assert (np.abs(seqs) > P.U_LIM).any() and (np.abs(seqs) < P.U_LIM).any()
    P.assert_priors_matter(oracle, "push", False, K, w0, "weights K=64", idx=idx, seqs=seqs)
    eng, opl = _pair(oracle, "push", False, K, idx=idx, seqs=seqs)
    ref = HipEngine(make_config(K=K, T=X.T, nu=2, filter_u=False, **PK))
    try:
        eng.set_point_cost_weights(W_TUNED)
        eng.set_world_point_raw(raw_world(w0))
        eng.command(sync_host=True)
        opl.command(w0)
        np.testing.assert_array_equal(eng.states.cpu().numpy().view(np.uint32), opl.last["states"].view(np.uint32))
        np.testing.assert_array_equal(eng.actions.cpu().numpy().view(np.uint32), opl.last["actions"].view(np.uint32))
        assert (eng.cost_horizon.cpu().numpy() != opl.last["cost_h"]).mean() > 0.9
        table = X.actions(K, X.T).copy()
        table[idx] = d
        ref.set_objective("push", X.GOAL); ref.set_noise(table); ref.set_point_cost_weights(W_TUNED)
        ref.set_world_point_raw(raw_world(w0))
        ref.command(sync_host=True)
        assert ref.prior_samples_used() == 0 and eng.prior_samples_used() == 1
        for b in (L.BUF_ACTIONS, L.BUF_STATES, L.BUF_COST_HORIZON, L.BUF_TRAJ_COST, L.BUF_WEIGHTS, L.BUF_MEAN, L.BUF_ACTION_OUT):
            assert eng.buffer(b).cpu().numpy().tobytes() == ref.buffer(b).cpu().numpy().tobytes(), b
    finally:
        eng.close()
        ref.close()


def test_priors_with_avoid_dyn_obs(oracle):
    K = 64
    w0 = X.start_worlds(oracle)[1]
    P.assert_priors_matter(oracle, "push", False, K, w0, "avoid K=64")
    eng, opl = _pair(oracle, "push", False, K)
    try:
        eng.set_avoid_dyn_obs(True)
        opl.cfg.avoid_dyn_obs = 1
        eng.set_world_point_raw(raw_world(w0))
        eng.command(sync_host=True)
        opl.command(w0)
        _assert_rollout_bits(eng, opl, "priors + avoid_dyn_obs")
    finally:
        eng.close()


def test_priors_in_simple_mode_with_the_random_sampler(oracle):
    """The prior samples' actions and states are the oracle's bit for bit (they do not depend on the in-kernel draws); the
    other samples agree within the figures of tests/test_hip_parity_point.py for in-kernel noise.  On the second command (U is
    no longer zero) the trajectory cost of a prior sample is S + sum_t U[t] . (lambda (e[t] - U[t]) / sigma), with e the
    clamped prior: the simple mode's perturbation cost of the stored action.  Its bound: sixteen roundings of the magnitudes
    summed.  Against the oracle: the prior samples' cost_h bit for bit (their states are), and their trajectory cost against
    oracle.simple_update's cost_total -- which carries + mean_k(S), oracle/mppi_core.c, taken off here -- at the parity figure
    of the costs (rtol 1e-5, atol 1e-4)."""
    K, T = 64, X.T
    idx = P.prior_indices(K)
    kw = dict(mode_simple=True, u_per_command=4, lambda_=0.5, filter_u=False)
    delta = None
    opl = P.make_prior_planner(oracle, oracle.make_cfg(K, T, 2, task="navigation", goal=X.GOAL, **kw), delta, idx,
                               P.prior_seqs(len(idx), T), seed=7)
    eng = HipEngine(make_config(K=K, T=T, nu=2, sampling_random=True, seed=7, **kw, **PK))
    w0 = X.start_worlds(oracle)[0]
    try:
        eng.set_objective("navigation", X.GOAL)
        for call in range(2):
            seqs = P.prior_seqs(len(idx), T, seed=30 + call)
            eng.set_prior_samples(seqs, idx)
            opl.set_priors(idx, seqs)
            torch.cuda.synchronize()
            U = np.roll(eng.buffer(L.BUF_MEAN).cpu().numpy().astype(np.float64), -1, axis=0)
            eng.set_world_point_raw(raw_world(w0))
            eng.command(sync_host=True)
            opl.command(w0)
            ac, st = eng.actions.cpu().numpy(), eng.states.cpu().numpy()
            e = P.clip(opl.cfg, seqs)
            np.testing.assert_array_equal(ac[idx].view(np.uint32), e.view(np.uint32))
            np.testing.assert_array_equal(st[idx].view(np.uint32), opl.last["states"][idx].view(np.uint32))
            np.testing.assert_allclose(ac, opl.last["actions"], atol=2e-6)
            np.testing.assert_allclose(st, opl.last["states"], atol=1e-4)
            ch = eng.cost_horizon.cpu().numpy().astype(np.float64)
            terms = U[None] * (0.5 * (e.astype(np.float64) - U[None]) / 3.0)
            want = ch[idx].sum(1) + terms.sum(axis=(1, 2))
            bound = 16 * 2.0 ** -24 * (np.abs(ch[idx]).sum(1) + np.abs(terms).sum(axis=(1, 2)))
            got = eng.buffer(L.BUF_TRAJ_COST).cpu().numpy()[idx].astype(np.float64)
            print(f"call {call}: perturbation cost of the priors {terms.sum(axis=(1, 2))}, |got - want| {np.abs(got - want)}, bound {bound}")
            assert (np.abs(got - want) <= bound).all(), call
            np.testing.assert_array_equal(eng.cost_horizon.cpu().numpy()[idx].view(np.uint32), opl.last["cost_h"][idx].view(np.uint32))
            mean_s = F(opl.last["S"].astype(np.float64).sum() / K)
            ct = opl.last["cost_total"][idx].astype(np.float64) - float(mean_s)
            print(f"call {call}: trajectory cost of the priors {got}, the oracle's cost_total - mean(S) {ct}")
            np.testing.assert_allclose(got, ct, rtol=1e-5, atol=1e-4, err_msg=f"call {call}")
            if call == 1:
                assert np.abs(terms.sum(axis=(1, 2))).min() > 0.0
        assert eng.prior_samples_used() == 1
    finally:
        eng.close()


def test_priors_with_update_cov(oracle):
    K, T = 128, 12
    w0 = X.start_worlds(oracle)[2].copy()
    eng, opl = _pair(oracle, "push", False, K, T=T, eng_kw=dict(update_cov=True), opl_kw=dict(update_cov=True), filter_u=True)
    try:
        for call in range(2):
            w0[0] += 0.02 * call
            eng.set_world_point_raw(raw_world(w0))
            eng.command(sync_host=True)
            opl.command(w0)
            if call == 0:
                _assert_rollout_bits(eng, opl, "update_cov first command")
            # (the figure of tests/test_hip_parity_point.py for scale_tril after the call)
            np.testing.assert_allclose(eng.buffer(L.BUF_COV).cpu().numpy()[1], [opl.cfg.scale_tril[j] for j in range(2)], rtol=1e-4)
            np.testing.assert_array_equal(eng.actions.cpu().numpy()[opl.prior_idx].view(np.uint32),
                                          P.clip(opl.cfg, opl.prior_seqs).view(np.uint32))
    finally:
        eng.close()


# ------------------------------------------------------------------ 7: fused versus step
def _side(extra=()):
    from tests.test_cost_weights_gpu import _side as side
    return side(["task=push", "goal=[-1.0, -1.0]", "mppi.num_samples=64", "mppi.horizon=12", "mppi.u_per_command=12", *extra])


def test_fused_path_is_the_step_path_with_priors():
    t = _side()
    try:
        p = t.motion_planner
        assert p._fused is None
        seqs = P.prior_seqs(4, 12, seed=3)
        p.set_prior_samples(seqs)
        assert p._engine.prior_samples_set() == 4
        t.first_plan(t.sim._dof_state[0:1].clone(), t.sim._root_state[0:1].clone())
        print(f"probe {p.probe_result}")
        assert p.probe_result == dict(fused=True, max_abs_diff=0.0)
        lim = np.maximum(np.minimum(seqs, F(p.u_max.cpu().numpy())), F(p.u_min.cpu().numpy()))
        np.testing.assert_array_equal(p.perturbed_action[:4].cpu().numpy().view(np.uint32), lim.view(np.uint32))   # the step leg's rows
        assert p._engine.prior_samples_used() == 1
    finally:
        t.close()


def test_step_path_rows_are_the_clipped_priors():
    t = _side(["mppi.fused=false"])
    try:
        p = t.motion_planner
        seqs = P.prior_seqs(3, 12, seed=4)
        p.set_prior_samples(seqs, [5, 17, 40])
        t.first_plan(t.sim._dof_state[0:1].clone(), t.sim._root_state[0:1].clone())
        assert p._fused is False
        lim = np.maximum(np.minimum(seqs, F(p.u_max.cpu().numpy())), F(p.u_min.cpu().numpy()))
        np.testing.assert_array_equal(p.perturbed_action[[5, 17, 40]].cpu().numpy().view(np.uint32), lim.view(np.uint32))
        # (the rows the update consumed: the scaled controls of those samples)
        got = p._buf(L.BUF_ACTIONS).cpu().numpy()[:, [5, 17, 40]].transpose(1, 0, 2)
        np.testing.assert_array_equal(got.view(np.uint32), (F(p.u_scale) * lim).astype(F).view(np.uint32))
    finally:
        t.close()


# ------------------------------------------------------------------ 8: the prior sample with the lowest cost
def test_a_go_to_prior_wins_a_planner_with_little_noise(oracle):
    K, T, p_idx = 64, X.T, 21
    goal = np.array(X.GOAL, np.float64)
    kw = dict(filter_u=False, noise_sigma_diag=[0.01, 0.01])
    # a start world in free space, chosen on the oracle: the robot between the origin and the goal, the box and the dyn-obs away
    w0 = oracle.init_world(1)[0].astype(F)
    w0[0:2] = (0.0, 0.3); w0[oracle.W_B:oracle.W_B + 2] = (-2.5, -2.5); w0[oracle.W_D:oracle.W_D + 2] = (3.0, -3.0)
    start = w0[0:2].astype(np.float64)
    seq = A.go_to(start, goal, T, 0.05, [3.0, 3.0], speeds=(1.0,))
    mk = lambda: oracle.make_cfg(K, T, 2, task="navigation", goal=X.GOAL, **kw)
    with_p = P.make_prior_planner(oracle, mk(), X.actions(K, T), [p_idx], seq)
    without = oracle.OraclePointPlanner(mk(), X.actions(K, T))
    u_with, u_without = with_p.command(w0), without.command(w0)
    d = (goal - start) / np.hypot(*(goal - start))
    proj_with, proj_without = float(u_with[0] @ d), float(u_without[0] @ d)
    print(f"oracle: best sample {with_p.last['info'].best_idx} (prior {p_idx}), first control along the goal direction with the prior "
          f"{proj_with:.4f}, without {proj_without:.4f}")
    assert int(np.argmin(with_p.last["J"])) == p_idx and with_p.last["info"].best_idx == p_idx
    assert proj_with > 0 and proj_with >= 10 * abs(proj_without)
    eng = HipEngine(make_config(K=K, T=T, nu=2, filter_u=False, **{**PK, "noise_sigma_diag": [0.01, 0.01]}))
    try:
        eng.set_objective("navigation", X.GOAL)
        eng.set_noise(X.actions(K, T))
        eng.set_prior_samples(seq, [p_idx])
        eng.set_world_point_raw(raw_world(w0))
        a = eng.command(sync_host=True)
        assert eng.info().best_idx == p_idx
        np.testing.assert_allclose(a[:u_with.shape[0]], u_with, atol=1e-3)
    finally:
        eng.close()


# ------------------------------------------------------------------ 9: life cycle and refusals
ALL = (L.BUF_ACTION_OUT, L.BUF_MEAN, L.BUF_BEST, L.BUF_WEIGHTS, L.BUF_TRAJ_COST, L.BUF_COST_HORIZON, L.BUF_STATES, L.BUF_ACTIONS,
       L.BUF_PENDING_FORCE)


def test_life_cycle(oracle):
    K = 100
    w0 = X.start_worlds(oracle)[2]
    idx5, idx2 = [3, 17, 63, 64, 98], [64, 5]
    s5, s2 = P.prior_seqs(5, seed=11), P.prior_seqs(2, seed=12)
    P.assert_priors_matter(oracle, "push", False, K, w0, "five", idx=idx5, seqs=s5)
    P.assert_priors_matter(oracle, "push", False, K, w0, "two", idx=idx2, seqs=s2)
    eng, _ = _pair(oracle, "push", False, K, idx=idx5, seqs=s5)
    never = HipEngine(make_config(K=K, T=X.T, nu=2, filter_u=False, **PK))
    mk = lambda: oracle.make_cfg(K, X.T, 2, task="push", goal=X.GOAL, filter_u=False)
    try:
        never.set_objective("push", X.GOAL); never.set_noise(X.actions(K, X.T))
        plan_never = _plan_of(never, "push", False, K, 0)
        eng.set_world_point_raw(raw_world(w0))
        eng.command(sync_host=True)
        for j in range(5):
            k, seq = eng.prior_sample(j)
            assert k == idx5[j] and seq.tobytes() == s5[j].tobytes()
        # n = 5 replaced by n = 2 with other indices; the setting survives m3_reset
        eng.set_prior_samples(s2, idx2)
        eng.reset()
        assert eng.prior_samples_set() == 2
        eng.command(sync_host=True)
        opl = P.make_prior_planner(oracle, mk(), X.actions(K, X.T), idx2, s2)
        opl.command(w0)
        _assert_rollout_bits(eng, opl, "two priors after five and a reset")
        assert [eng.prior_sample(j)[0] for j in range(2)] == idx2 and eng.prior_sample(1)[1].tobytes() == s2[1].tobytes()
        with pytest.raises(L.M3Error):
            eng.prior_sample(2)
        # the same indices again with other values: the slot map is not what changes
        s2b = P.prior_seqs(2, seed=13)
        eng.set_prior_samples(s2b, idx2)
        eng.reset()
        eng.command(sync_host=True)
        opl = P.make_prior_planner(oracle, mk(), X.actions(K, X.T), idx2, s2b)
        opl.command(w0)
        _assert_rollout_bits(eng, opl, "the same indices, other values")
        # cleared: byte for byte the handle that never had priors, and its plan
        eng.set_prior_samples(None)
        assert eng.prior_samples_set() == 0
        assert _plan_of(eng, "push", False, K, 0) == plan_never and plan_never[8] == 0
        eng.reset()
        for c in range(3):
            w = w0.copy(); w[0] += 0.02 * c
            for e in (eng, never):
                e.set_world_point_raw(raw_world(w))
                e.command()
            torch.cuda.synchronize()
            for b in ALL:
                assert eng.buffer(b).cpu().numpy().tobytes() == never.buffer(b).cpu().numpy().tobytes(), (c, b)
            assert bytes(eng.info()) == bytes(never.info())
            assert eng.prior_samples_used() == 0
        # set again after a clear, with the indices the device map was last built from
        eng.set_prior_samples(s2b, idx2)
        eng.reset()
        eng.set_world_point_raw(raw_world(w0))
        eng.command(sync_host=True)
        _assert_rollout_bits(eng, opl, "set again after a clear")
    finally:
        eng.close()
        never.close()


def _refused(eng, code, match, seqs, idx, device=False):
    lib = eng.lib
    arr = (C.c_int * max(len(idx), 1))(*idx)
    n = len(idx)
    s = np.ascontiguousarray(seqs, F)
    fn = lib.m3_set_prior_samples_device if device else lib.m3_set_prior_samples
    rc = fn(eng._h, s.ctypes.data, arr, n)
    msg = lib.m3_last_error(eng._h).decode()
    assert rc == code, (rc, msg)
    assert ("m3_set_prior_samples_device" if device else "m3_set_prior_samples") in msg and match in msg, msg


def test_refusals_of_the_setter(oracle):
    K, T = 64, X.T
    w0 = X.start_worlds(oracle)[2]
    idx, seqs = [3, 40], P.prior_seqs(2, seed=5)
    for mm, task in ((False, "push"), (True, "push_pull")):
        eng, opl = _pair(oracle, task, mm, K, idx=idx, seqs=seqs)
        try:
            lib = eng.lib
            good = P.prior_seqs(6, seed=6)
            assert lib.m3_set_prior_samples(eng._h, good.ctypes.data, (C.c_int * 1)(1), -1) == BAD_ARG
            assert "m3_set_prior_samples: n is -1" in lib.m3_last_error(eng._h).decode()
            assert lib.m3_set_prior_samples(eng._h, good.ctypes.data, (C.c_int * 1)(1), L.MAX_PRIOR_SAMPLES + 1) == BAD_ARG
            _refused(eng, BAD_ARG, "prior 1: sample 64 is outside", good[:2], [5, K])
            _refused(eng, BAD_ARG, "prior 0: sample -1 is outside", good[:1], [-1])
            _refused(eng, BAD_ARG, "prior 2: sample 63 is the zero-noise", good[:3], [5, 6, K - 1])
            _refused(eng, BAD_ARG, "prior 3: sample 17 listed twice", good[:4], [17, 5, 6, 17])
            _refused(eng, BAD_ARG, "prior 3: sample 17 listed twice", good[:4], [17, 5, 6, 17], device=True)
            bad = good[:3].copy()
            bad[2, 5, 1] = np.nan
            _refused(eng, BAD_ARG, "prior 2: step 5 control 1 is not finite", bad, [5, 6, 7])
            bad[2, 5, 1] = np.inf
            _refused(eng, BAD_ARG, "prior 2: step 5 control 1 is not finite", bad, [5, 6, 7])
            if mm:
                _refused(eng, BAD_ARG, "prior 0: sample 0 is a best-trajectory sample", good[:1], [0])
                _refused(eng, BAD_ARG, "prior 1: sample 32 is a best-trajectory sample", good[:2], [5, K // 2])
            else:
                eng.set_prior_samples(good[:2], [0, K // 2])       # no special samples there in single mode
                eng.set_prior_samples(seqs, idx)
            # every refusal left the state alone: the priors come back, and the next command is the oracle's
            assert eng.prior_samples_set() == 2
            for j in range(2):
                k, s = eng.prior_sample(j)
                assert k == idx[j] and s.tobytes() == seqs[j].tobytes()
            eng.set_world_point_raw(raw_world(w0))
            eng.command(sync_host=True)
            opl.command(w0)
            _assert_rollout_bits(eng, opl, f"{task} after the refusals")
            # the run-time-scene instance forced off
            calls = eng.info().calls
            eng.set_point_scene_instance(0)
            with pytest.raises(L.M3Error, match=r"forced off.*m3_set_prior_samples"):
                eng.command()
            assert eng.info().calls == calls
            eng.set_point_scene_instance(-1)
            eng.command(sync_host=True)
        finally:
            eng.close()


def test_refusals_by_the_kind_of_handle():
    lib = L.load()
    seqs = P.prior_seqs(2, 12)
    arr = (C.c_int * 2)(3, 4)
    sim = HipEngine(make_config(K=64, T=12, nu=2, sim_only=True, filter_u=False, **PK))
    try:
        assert lib.m3_set_prior_samples(sim._h, seqs.ctypes.data, arr, 2) == STATE
        assert b"m3_set_prior_samples: planner handles only" in lib.m3_last_error(sim._h)
        assert lib.m3_prior_samples_set(sim._h) == 0
    finally:
        sim.close()
    p = HipEngine(make_config(K=64, T=12, nu=9, env_type="panda_env", u_min=[-2] * 9, u_max=[2] * 9, noise_sigma_diag=[1] * 9))
    try:
        assert lib.m3_set_prior_samples(p._h, seqs.ctypes.data, arr, 2) == UNSUPPORTED
        assert b"m3_set_prior_samples: point_env only" in lib.m3_last_error(p._h)
        assert lib.m3_set_prior_samples_device(p._h, None, None, 0) == UNSUPPORTED
        assert lib.m3_get_prior_sample(p._h, 0, None, None) == UNSUPPORTED
    finally:
        p.close()
    sh = HipEngine(make_config(K=128, K_local=64, k_offset=64, T=12, nu=2, **PK))
    try:
        assert lib.m3_set_prior_samples(sh._h, seqs.ctypes.data, arr, 2) == UNSUPPORTED
        assert b"m3_set_prior_samples: sharded handle (K_local != K_global)" in lib.m3_last_error(sh._h)
        assert lib.m3_prior_samples_set(sh._h) == 0
    finally:
        sh.close()


def test_batched_command_refuses_a_handle_with_priors():
    K = 64
    twins = [Twin(i, K=K, T=12, task="push", goal=X.GOAL) for i in range(3)]
    batch = HipBatch(3)
    try:
        twins[1].A.set_prior_samples(P.prior_seqs(2, 12), [3, 4])
        for t in twins:
            t.set_world(0)
        before = [t.A.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes() for t in twins]
        with pytest.raises(L.M3Error, match=r"error -5: .*handle 1.*m3_set_prior_samples"):
            batch.command([t.A for t in twins])
        torch.cuda.synchronize()
        assert [t.A.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes() for t in twins] == before
        assert all(t.A.info().calls == 0 for t in twins)
        # the other two afterwards, and the refused one by its own command: identical to the control run
        batch.command([twins[0].A, twins[2].A])
        twins[0].B.command(); twins[2].B.command()
        twins[1].B.set_prior_samples(P.prior_seqs(2, 12), [3, 4])
        twins[1].A.command(); twins[1].B.command()
        torch.cuda.synchronize()
        assert [t.assert_same("after the refusal") for t in twins] == [1, 1, 1]
    finally:
        batch.close()
        for t in twins:
            t.close()


def test_lockstep_episodes_refuse_a_planner_with_priors():
    """m3_episodes_create, and m3_episodes_tick / _begin for priors set afterwards: M3_ERR_UNSUPPORTED, the message names
    m3_set_prior_samples and the planner; nothing is launched, planners and world stay as they were"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
    from m3p2i_aip_amd.engine import HipEpisodes
    from m3p2i_aip_amd.episodes import build_set
    push = ["task=push", "goal=[-3,3]", "mppi.num_samples=64", "mppi.horizon=12", "mppi.u_per_command=12"]
    es = build_set([("config_point", push, dict(dyn_phase=0, box=(0.0, 0.0), robot=(0.0, 0.0))),
                    ("config_point", push, dict(dyn_phase=24, box=(0.02, -0.03), robot=(-0.01, 0.04)))], max_ticks=6)
    try:
        es.start()
        world = es.real._engine
        engs = [s.motion_planner._engine for s in es.sides]
        spec = [("push", (-3.0, 3.0), 0, L.SUCTION_OFF, 400.0)] * 2
        es.eps.close()
        seqs = P.prior_seqs(2, 12)

        def snapshot():
            torch.cuda.synchronize()
            return [(e.buffer(L.BUF_MEAN).clone(), e.buffer(L.BUF_TRAJ_COST).clone(), e.info().calls) for e in engs], \
                world.buffer(L.BUF_SIM_WORLD).clone()

        def unchanged(before):
            after = snapshot()
            for (m0, j0, c0), (m1, j1, c1) in zip(before[0], after[0]):
                assert torch.equal(m0, m1) and torch.equal(j0, j1) and c0 == c1
            assert torch.equal(before[1], after[1])

        engs[1].set_prior_samples(seqs, [3, 4])
        before = snapshot()
        for runtime in (False, True):
            with pytest.raises(L.M3Error, match=r"error -5: m3_episodes_create: planner 1: it has prior samples \(m3_set_prior_samples\)"):
                HipEpisodes(world, engs, spec, 6, point_runtime=runtime)
        unchanged(before)
        engs[1].set_prior_samples(None)
        plain = HipEpisodes(world, engs, spec, 6)
        batch = HipBatch(2)
        try:
            engs[1].set_prior_samples(seqs, [3, 4])
            before = snapshot()
            with pytest.raises(L.M3Error, match=r"error -5: m3_episodes_tick: planner 1: it has prior samples \(m3_set_prior_samples\)"):
                plain.tick(batch)
            rc = plain.lib.m3_episodes_begin(plain._eps)
            assert rc == UNSUPPORTED and b"m3_episodes_begin: planner 1: it has prior samples (m3_set_prior_samples)" in \
                plain.lib.m3_episodes_last_error(plain._eps)
            unchanged(before)
            assert plain.ticks_done == 0
            # m3_episodes_end: priors set between begin and end
            engs[1].set_prior_samples(None)
            assert plain.lib.m3_episodes_begin(plain._eps) == 0
            engs[1].set_prior_samples(seqs, [3, 4])
            before = snapshot()
            rc = plain.lib.m3_episodes_end(plain._eps)
            assert rc == UNSUPPORTED and b"m3_episodes_end: planner 1: it has prior samples (m3_set_prior_samples)" in \
                plain.lib.m3_episodes_last_error(plain._eps)
            unchanged(before)
            assert plain.ticks_done == 0
            engs[1].set_prior_samples(None)          # cleared: the tick ends, and the set runs
            assert plain.lib.m3_episodes_end(plain._eps) == 0
            plain.tick(batch)
            assert plain.ticks_done == 2
        finally:
            batch.close()
            plain.close()
    finally:
        es.close()


# ------------------------------------------------------------------ 10: the device entry point
def test_device_entry_point_gives_the_bits_of_the_host_entry_point(oracle):
    K = 100
    idx, seqs = P.prior_indices(K), P.prior_seqs(4)
    t = Twin(0, K=K, T=X.T, task="push", goal=X.GOAL, filter_u=False)
    try:
        for c in range(2):
            s = P.prior_seqs(4, seed=40 + c)
            t.A.set_prior_samples(torch.as_tensor(s, device=t.A.device), idx)
            t.B.set_prior_samples(s, idx)
            t.set_world(c)
            t.A.command()
            t.B.command()
            torch.cuda.synchronize()
            assert t.assert_same(f"device call {c}") == c + 1
            np.testing.assert_array_equal(t.A.actions.cpu().numpy()[idx].view(np.uint32),
                                          np.clip(s, -3, 3).astype(F).view(np.uint32))
        assert t.A.prior_samples_set() == 4 and t.B.prior_sample(0)[0] == idx[0]
        with pytest.raises(L.M3Error):          # the values of a device-set prior are not kept on the host
            t.A.prior_sample(0)
        k = C.c_int()
        assert t.A.lib.m3_get_prior_sample(t.A._h, 1, C.byref(k), None) == 0 and k.value == idx[1]
        assert seqs.shape == (4, X.T, 2)
    finally:
        t.close()
