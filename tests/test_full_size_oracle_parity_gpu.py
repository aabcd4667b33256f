"""The BASELINE configs at their FULL sizes against the CPU oracle directly (not through properties): the
one-launch update instantiations the bench configs actually run -- k_update_small<2,false,8> (C2, K=2000),
<2,true,16> (C3, K=4000), <9,false,16> (C4 panda, K=4000), <2,false,64> (north-star, K=10000), <2,true,32>
(a C5 shard, K=8000) -- and the large-K multi-launch path (C5 unsharded, K=64000).  The oracle (C, OpenMP)
finishes a command at these sizes in milliseconds to a second.  Bars: rollout states / actions / costs
bit-exact on the first call; control output and weights within 1e-3 (BASELINE.json north_star) on every call;
multi-modal iteration counts equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# weights: relative, not absolute -- with eta in [3, 10] all but a handful of the K weights are below 1e-3, so an
# absolute bar of 1e-3 asserts nothing about the tail; the form of test_hip_parity_point.py:152
W_TOL = dict(rtol=2e-3, atol=1e-6)

POINT = {
    "C2_push_K2000": dict(K=2000, task="push", goal=(-1.0, -1.0), mm=False),
    "C3_hybrid_K4000": dict(K=4000, task="push_pull", goal=(-3.75, -3.75), mm=True),
    "northstar_push_K10000": dict(K=10000, task="push", goal=(-1.0, -1.0), mm=False),
    "C5shard_hybrid_K8000": dict(K=8000, task="push_pull", goal=(-3.75, -3.75), mm=True),
    "C5_hybrid_K64000": dict(K=64000, task="push_pull", goal=(-3.75, -3.75), mm=True),
    # more wavefronts (1094) than the chip has SIMDs (1024): the two-waves-per-SIMD build of the rollout kernel
    # (k_rollout_point_occ<2>: 256 VGPRs, ~175 values in scratch) -- same bits as the oracle
    "occ2_push_K70016": dict(K=70016, task="push", goal=(-1.0, -1.0), mm=False),
    "occ2_hybrid_K70016": dict(K=70016, task="push_pull", goal=(-3.75, -3.75), mm=True),
    # more than four wavefronts per SIMD (8192 > 4096): the THREE-waves build (k_rollout_point_occ<3>: 170 VGPRs, the rest
    # in scratch) and the saturated update (k_mins / k_ladder / k_search / k_apply_weights / k_wsum with the top-k
    # stage B) against the full oracle command -- every state, action, cost and J of the 524 288 rollouts bit for bit
    "occ3_push_K524288": dict(K=524288, task="push", goal=(-1.0, -1.0), mm=False, calls=2),
    "occ3_hybrid_K524288": dict(K=524288, task="push_pull", goal=(-3.75, -3.75), mm=True, calls=2),
}


def _smooth_noise(K, T, nu, seed):
    g = torch.Generator().manual_seed(seed)
    knots = torch.randn(K, nu, T // 4, generator=g)
    d = torch.nn.functional.interpolate(knots, size=T, mode="linear", align_corners=True)
    return d.permute(0, 2, 1).contiguous().numpy()


@pytest.mark.parametrize("name", list(POINT))
def test_point_env_full_size_vs_oracle(oracle, name):
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipEngine, make_config
    c = POINT[name]
    K, T = c["K"], 30
    delta = _smooth_noise(K, T, 2, 21)
    w0 = oracle.init_world(1)[0]
    w0[0:2] = (0.05, 1.5)                      # next to the box: contacts and suction inside the horizon
    opl = oracle.OraclePointPlanner(oracle.make_cfg(K, T, 2, task=c["task"], goal=c["goal"], multi_modal=c["mm"]), delta)
    eng = HipEngine(make_config(K=K, T=T, nu=2, multi_modal=c["mm"], u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3]))
    eng.set_objective(c["task"], c["goal"])
    eng.set_noise(delta)
    raw = np.concatenate([w0[[0, 1, 4, 5]], w0[7:14], w0[14:21]]).astype(np.float32)
    eng.set_world_point_raw(raw)
    for call in range(c.get("calls", 3)):
        a = eng.command(sync_host=True)
        b = opl.command(w0)
        if call == 0:
            assert np.array_equal(eng.states.cpu().numpy(), opl.last["states"])
            assert np.array_equal(eng.actions.cpu().numpy(), opl.last["actions"])
            assert np.array_equal(eng.cost_horizon.cpu().numpy(), opl.last["cost_h"])
            assert np.array_equal(eng.buffer(L.BUF_TRAJ_COST).cpu().numpy(), opl.last["J"])
        np.testing.assert_allclose(a, b, atol=1e-3, err_msg=f"{name} call {call}")
        from tests.conftest import assert_close_but_few
        few = dict(frac=0.0 if call == 0 else 1e-3, cap=1e-3, **W_TOL)      # (later calls: conftest.assert_close_but_few)
        assert_close_but_few(eng.buffer(L.BUF_WEIGHTS).cpu().numpy(), opl.last["w"], err_msg=f"{name} call {call} weights", **few)
        i, oi = eng.info(), opl.last["info"]
        if c["mm"]:
            assert_close_but_few(eng.buffer(L.BUF_WEIGHTS_1).cpu().numpy(), opl.last["w1"], err_msg="weights_1", **few)
            assert_close_but_few(eng.buffer(L.BUF_WEIGHTS_2).cpu().numpy(), opl.last["w2"], err_msg="weights_2", **few)
            assert (i.iters, i.iters_1, i.iters_2) == (oi.iters, oi.iters_1, oi.iters_2), f"{name} call {call}"
            assert (i.best_idx_1, i.best_idx_2) == (oi.best_idx_1, K // 2 + oi.best_idx_2)
            assert i.pull_preference == opl.pull_preference()
        else:
            assert i.best_idx == oi.best_idx
        top = eng.buffer(L.BUF_TOP_IDX).cpu().numpy()
        assert np.array_equal(np.sort(opl.last["J"][top]), np.sort(opl.last["J"])[:20]) or call > 0
        # top_trajs = states[top_idx][:, :, [0, 2]] of THIS handle's rollout (mppi.py:248-254), every call
        Jh = eng.buffer(L.BUF_TRAJ_COST).cpu().numpy()
        assert np.array_equal(np.sort(Jh[top]), np.sort(Jh)[:20])
        np.testing.assert_array_equal(eng.buffer(L.BUF_TOP_TRAJS).cpu().numpy(), eng.states.cpu().numpy()[top][:, :, [0, 2]])
    eng.close()


@pytest.mark.parametrize("task,grip,start", [("reach", 1, "init"), ("pick", 2, "held"), ("place", 1, "held"),
                                             ("pick", 2, "open3")])
def test_panda_full_size_vs_oracle(oracle, task, grip, start):
    """C4: panda_env K=4000, T=20 at full size -- k_update_small<9,false,16> and both panda rollout instances:
    reach (k_rollout_panda<false,..>, the first commands of the reactive pick) and the config BASELINE names,
    reactive PICK: start from a grasp (cube held), gripper override close (mppi.py:412-416), pick cost + motion
    cost on the penalty forces (cost_functions.py:116-125, :158-169) = the <FORCES=true> instance; place from the
    same grasp (gripper override open: the cube is released inside the horizon); and pick with the OPEN gripper
    3 cm above the grasp pose (rollouts grasp, or just miss, on their own).  Three calls each: persistent beta
    (mppi.py:446-454) and the warm start are part of the trace."""
    import oracle.panda as P
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipEngine, make_config
    from tests.panda_worlds import grasp_world
    K, T = 4000, 20
    delta = _smooth_noise(K, T, 9, 22)
    goal = np.array([0.2, 0.2, 1.115, 0, 0, 0, 1], np.float32)
    sc = P.default_scene()
    if start == "init":
        w0 = P.init_world(1)[0]
    elif start == "held":
        w0 = grasp_world(P, sc)
    else:
        w0 = grasp_world(P, sc, close_gripper=False, lift=0.03)
    opl = P.OraclePandaPlanner(P.make_cfg(K, T, task=task, goal=goal, gripper_cmd=grip), delta)
    eng = HipEngine(make_config(K=K, T=T, nu=9, env_type="panda_env", u_min=[-2.0] * 7 + [-1.5] * 2,
                                u_max=[2.0] * 7 + [1.5] * 2, noise_sigma_diag=[10.0] * 7 + [0.8] * 2, lambda_=0.05,
                                pre_height_diff=0.05, dt=0.01))
    eng.set_objective(task, goal, gripper_cmd=grip)
    eng.set_noise(delta)
    eng.set_world_panda_raw(P.raw57(w0))
    for call in range(3):
        a = eng.command(sync_host=True)
        b = opl.command(w0)
        if call == 0:
            assert np.array_equal(eng.states.cpu().numpy(), opl.last["states"])
            assert np.array_equal(eng.actions.cpu().numpy(), opl.last["actions"])
            assert np.array_equal(eng.cost_horizon.cpu().numpy(), opl.last["cost_h"])
            assert np.array_equal(eng.buffer(L.BUF_TRAJ_COST).cpu().numpy(), opl.last["J"])
        np.testing.assert_allclose(a, b, atol=1e-3, err_msg=f"call {call}")
        wh, wo = eng.buffer(L.BUF_WEIGHTS).cpu().numpy(), opl.last["w"]
        Jh, Jo = eng.buffer(L.BUF_TRAJ_COST).cpu().numpy(), opl.last["J"]
        bi_h, bi_o = eng.info().best_idx, opl.last["info"].best_idx
        if call == 0:
            np.testing.assert_allclose(wh, wo, **W_TOL)
            assert bi_h == bi_o
        else:
            # Later calls start from plans that agree to ~1e-7, not to the bit (two implementations of the mean update).  The
            # model of what that can do: a rollout whose contact history FLIPS (unilateral contacts, Coulomb friction: not
            # continuous) gets another trajectory cost; every other rollout keeps its cost to rounding, so its weight changes
            # only by the common factor eta_oracle / eta_hip.  Asserted as exactly that: the flipped rollouts are counted
            # (reported below; bounded at 5 % of K), every weight outside the tolerance belongs to one of them once the common
            # factor is divided out, and the best sample is the same one unless the two candidates' costs tie to 1e-4.
            flipped = ~np.isclose(Jh, Jo, rtol=1e-5, atol=1e-5)
            n_flip = int(flipped.sum())
            print(f"{task}/{start} call {call}: {n_flip} of {K} rollouts with another contact history")
            assert n_flip <= 0.05 * K
            keep = ~flipped & (wo > 1e-12)
            ratio = float(np.median(wh[keep] / wo[keep])) if keep.any() else 1.0
            assert abs(ratio - 1.0) < 0.05
            bad = ~np.isclose(wh, ratio * wo, **W_TOL)
            assert not (bad & ~flipped).any(), f"call {call}: {int((bad & ~flipped).sum())} weights of unflipped rollouts differ"
            assert np.abs(wh - wo).max() < 1e-3
            assert bi_h == bi_o or flipped[bi_h] or flipped[bi_o] or abs(Jo[bi_h] - Jo[bi_o]) <= 1e-4 * max(1.0, abs(Jo[bi_o]))
        assert eng.info().beta == pytest.approx(opl.beta, rel=1e-4)
    if task == "pick" and start == "held":
        ch = eng.cost_horizon.cpu().numpy()
        assert np.ptp(ch) > 0.05          # the held cube really travels with the hand in these rollouts
    eng.close()


@pytest.mark.parametrize("task,mm", [("push", False), ("push_pull", True)])
def test_the_three_rollout_builds_give_identical_bits(task, mm):
    """The point_env rollout kernel exists in three builds, chosen by the number of wavefronts of the launch
    (rollout_point_kernel.hpp: one resident wave per SIMD / `amdgpu_waves_per_eu(2, 2)` above 1024 wavefronts / `(3, 3)`
    above 4096).  The SAME noise rows through all three -- K = 2000 (occ1), 70 016 (occ2), 524 288 (occ3), the first
    1999 rows (per mode: 998) shared -- must give the same states, actions, step costs and trajectory costs bit for bit:
    a sample's rollout depends on nothing but its own noise row, the (zero) mean and the world."""
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipEngine, make_config
    T = 30
    goal = (-3.75, -3.75) if mm else (-1.0, -1.0)
    out = {}
    sizes = (2000, 70016, 524288)
    base = _smooth_noise(sizes[0], T, 2, 31)
    n_half = sizes[0] // 2 - 2        # (rows 1..998 of each half: 0 and K/2 carry the best trajectories, K-1 the null action)
    for K in sizes:
        delta = _smooth_noise(K, T, 2, 100 + K)
        if mm:   # the modes are the two halves of the sample range: share rows inside each half
            delta[1:1 + n_half] = base[1:1 + n_half]
            delta[K // 2 + 1:K // 2 + 1 + n_half] = base[sizes[0] // 2 + 1:sizes[0] // 2 + 1 + n_half]
        else:
            delta[:sizes[0] - 1] = base[:sizes[0] - 1]
        eng = HipEngine(make_config(K=K, T=T, nu=2, multi_modal=mm, u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3]))
        eng.set_objective(task, goal)
        eng.set_noise(delta)
        import oracle as O
        ow = O.init_world(1)[0]
        ow[0:2] = (0.05, 1.5)
        eng.set_world_point_raw(np.concatenate([ow[[0, 1, 4, 5]], ow[7:14], ow[14:21]]).astype(np.float32))
        eng.command(sync_host=True)
        rows = (np.r_[1:1 + n_half, K // 2 + 1:K // 2 + 1 + n_half] if mm else np.arange(sizes[0] - 1))
        idx = torch.as_tensor(rows, device="cuda")
        out[K] = [eng.states[idx].cpu().numpy(), eng.actions[idx].cpu().numpy(), eng.cost_horizon[idx].cpu().numpy(),
                  eng.buffer(L.BUF_TRAJ_COST)[idx].cpu().numpy()]
        eng.close()
    for K in sizes[1:]:
        for a, b, what in zip(out[sizes[0]], out[K], ("states", "actions", "cost_h", "J")):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: K={K} build differs from the K={sizes[0]} build"
    assert np.ptp(out[sizes[0]][2]) > 1.0     # (contacts and costs really vary over these rows)
