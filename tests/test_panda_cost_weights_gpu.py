"""The panda_env cost weights on the GPU (m3_set_panda_cost_weights, include/m3p2i_hip.h).

The oracle keeps the reference's literals, so the reference for non-default weights is tests/panda_cost_ref.py -- the float32
restatement of the three costs, pinned to the reference's values, the oracle's bits and a host build of the device header by
tests/test_panda_cost_weights_cpu.py -- applied to oracle.panda.observe of the oracle's own per-step worlds of the same
actions (tests/panda_cost_fixture.py).  Every value case first repeats that comparison at the default weights against the
oracle's own cost_horizon (which validates the replay) and is compared bit for bit: every operation is a correctly rounded
binary32 one in the same order, so there is no bound to state and no entry is left out.

Shapes: K = 61 (no multiple of 4, 8 or 64: a partial last wavefront in every kernel form), K = 62 multi-modal (half = 31), T = 6.
The fixtures' conditions (collision test live in the pick case, each table's shelf_force flips it) are asserted on the oracle
alone in the CPU file.

tests/test_hip_parity_panda.py holds no equality between the fused cost horizon and step + m3_cost replayed at the default
weights, so none is claimed here with weights: both paths are compared with the oracle's worlds instead.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, HipPandaEpisodes, make_config  # noqa: E402
from tests import panda_cost_fixture as Fx  # noqa: E402
from tests import panda_cost_ref as R  # noqa: E402
from tests import panda_scene_fixture as X  # noqa: E402

F = np.float32
# (filter_u off: the plan's Savitzky-Golay filter needs nine rows, T = 6 has six; it reads no cost)
PK = dict(u_min=X.UMIN, u_max=X.UMAX, noise_sigma_diag=X.SIG, lambda_=0.05, pre_height_diff=0.05, dt=0.01, filter_u=False)
GOAL = np.array(Fx.GOAL, F)
LANES = [1, 8, 16]
ERR_STATE, ERR_UNSUPPORTED = -4, -5          # M3_ERR_STATE, M3_ERR_UNSUPPORTED (include/m3p2i_hip.h)
# cost horizon, trajectory cost, weights, means, best, action out, top-k (+ what the rollout leaves for the update)
COMMAND_BUFS = [L.BUF_COST_HORIZON, L.BUF_TRAJ_COST, L.BUF_WEIGHTS, L.BUF_MEAN, L.BUF_MEAN_1, L.BUF_MEAN_2, L.BUF_BEST_1,
                L.BUF_BEST_2, L.BUF_ACTION_OUT, L.BUF_TOP_IDX, L.BUF_TOP_TRAJS, L.BUF_STATES, L.BUF_ACTIONS]


@pytest.fixture(scope="module")
def P(oracle):
    import oracle.panda as P
    P.lib()
    return P


def engine_of(case, lps=0, cost_kernel=True, weights=None, scene=None, **kw):
    """a planner handle of a fixture case (tests/panda_cost_fixture.py) with its world, objective and noise set"""
    import oracle.panda as P
    task, grip, mm, _ = Fx.CASES[case]
    k = Fx.K_of(mm)
    eng = HipEngine(make_config(K=k, T=Fx.T, nu=9, env_type="panda_env", multi_modal=mm, **{**PK, **kw}))
    eng.set_objective(task, GOAL, gripper_cmd=grip)
    eng.set_panda_lanes_per_sample(lps)
    eng.set_panda_reach_cost_kernel(cost_kernel)
    if not kw.get("sampling_random"):
        k0 = kw.get("k_offset", 0)
        eng.set_noise(Fx.delta_of(k)[k0:k0 + kw.get("K_local", k)])
    if scene is not None:
        eng.set_panda_scene(scene)
    if weights is not None:
        eng.set_panda_cost_weights(weights)
    eng.set_world_panda_raw(P.raw57(Fx.world_of(case)))
    return eng


def same_bytes(a, b, buf):
    return a.buffer(buf).cpu().numpy().tobytes() == b.buffer(buf).cpu().numpy().tobytes()


def bits(d):
    return bytes(L.PandaCostWeights(**{**L.PANDA_COST_WEIGHT_DEFAULTS, **d}))


# ------------------------------------------------------------------ 6. entry points (the symbols do not exist on the parent)
def test_entry_points_round_trip_and_life_cycle(P):
    eng = engine_of("pick")
    try:
        d = L.PandaCostWeights()
        eng.lib.m3_default_panda_cost_weights(C.byref(d))
        assert bytes(d) == bits({}) and {n: getattr(d, n) for n in R.NAMES} == L.PANDA_COST_WEIGHT_DEFAULTS
        assert eng.panda_cost_weights() == L.PANDA_COST_WEIGHT_DEFAULTS
        eng.set_panda_cost_weights(Fx.RANDOM_TABLE)
        assert bits(eng.panda_cost_weights()) == bits(Fx.RANDOM_TABLE)                  # round trip
        eng.set_panda_cost_weights(dict(pick_ori=25.0))
        assert eng.panda_cost_weights() == {**L.PANDA_COST_WEIGHT_DEFAULTS, "pick_ori": 25.0}    # missing keys: the defaults
        eng.reset()
        assert eng.panda_cost_weights()["pick_ori"] == 25.0                             # survive m3_reset
        eng.set_panda_cost_weights(dict(collision=0.0, pick_goal=-1.0))                 # zero and negative weights are legal
        eng.set_panda_cost_weights(None)
        assert bits(eng.panda_cost_weights()) == bits({})                               # None: the defaults
        with pytest.raises(ValueError, match=r"unknown panda cost weight\(s\) \['pick_orientation'\]"):
            eng.set_panda_cost_weights(dict(pick_orientation=1.0))
        with pytest.raises(L.M3Error, match="-1 .*0 or 1"):
            eng.set_panda_weighted_cost_instance(2)
        assert not eng.panda_weighted_cost_instance_used()
    finally:
        eng.close()


# ------------------------------------------------------------------ 7. identity: the forced instance at the default weights
IDENTITY = ([(c, lps, True, {}) for c in ("reach", "pick", "place") for lps in LANES] +
            [("reach", 16, False, {}), ("reach", 8, False, {}), ("reach_mm", 16, True, {}), ("reach_mm", 1, False, {}),
             ("pick", 0, True, dict(sampling_random=True, seed=3)),
             ("reach", 0, True, dict(mode_simple=True, sampling_random=True, seed=5, u_per_command=3))])


def _identity_id(c, lps, cost_kernel, kw):
    return "-".join([c, f"lps{lps}", "cost_kernel" if cost_kernel else "shadow_slots"] + [n for n in ("mode_simple", "sampling_random") if kw.get(n)])


@pytest.mark.parametrize("case,lps,cost_kernel,kw", IDENTITY, ids=[_identity_id(*x) for x in IDENTITY])
def test_forced_instance_at_default_weights_is_the_untouched_handle(P, case, lps, cost_kernel, kw):
    a, b = engine_of(case, lps, cost_kernel, **kw), engine_of(case, lps, cost_kernel, **kw)
    try:
        b.set_panda_weighted_cost_instance(1)
        for call in range(2):                         # (the second command goes through the warm start)
            pa, pb = a.command(sync_host=True), b.command(sync_host=True)
            assert not a.panda_weighted_cost_instance_used() and b.panda_weighted_cost_instance_used()
            assert not a.panda_scene_instance_used() and not b.panda_scene_instance_used()      # (the workspace did not need it)
            assert a.panda_lanes_per_sample_used() == b.panda_lanes_per_sample_used()
            if lps:
                assert a.panda_lanes_per_sample_used() == lps
            assert np.asarray(pa).tobytes() == np.asarray(pb).tobytes(), call
            for buf in COMMAND_BUFS:
                assert same_bytes(a, b, buf), (call, buf)
            assert bytes(a.info()) == bytes(b.info()), call
        ch = a.cost_horizon.cpu().numpy()
        assert np.isfinite(ch).all() and np.ptp(ch) > 0
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------ 8. values, fused
def assert_cost_horizon(eng, want, label):
    ch = eng.cost_horizon.cpu().numpy()
    assert ch.shape == want.shape
    bad = np.argwhere(ch.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{label}: {len(bad)} of {ch.size} costs differ, first {bad[0]}: {ch[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


def discounted(cost_h, gamma=F(0.95)):
    """the rollout's own recurrence over the steps: J = J + g c; g = g gamma"""
    J, g = np.zeros(cost_h.shape[0], F), F(1.0)
    for t in range(cost_h.shape[1]):
        J = J + g * cost_h[:, t]
        g = F(g * gamma)
    return J.astype(F)


@pytest.mark.parametrize("lps", LANES)
@pytest.mark.parametrize("case", list(Fx.CASES))
def test_fused_cost_horizon_equals_the_restatement_on_the_oracles_worlds(P, case, lps):
    ref = Fx.oracle_case(case)
    eng = engine_of(case, lps)
    try:
        # the harness first: at the default weights, on the weighted kernels, the oracle's own cost_horizon
        eng.set_panda_weighted_cost_instance(1)
        eng.rollout()
        torch.cuda.synchronize()
        assert eng.panda_weighted_cost_instance_used() and eng.panda_lanes_per_sample_used() == lps
        np.testing.assert_array_equal(eng.actions.cpu().numpy().view(np.uint32), ref["actions"].view(np.uint32))
        np.testing.assert_array_equal(eng.states.cpu().numpy().view(np.uint32), ref["states"].view(np.uint32))
        assert_cost_horizon(eng, ref["cost_h"], f"{case} lps {lps} defaults")
        assert Fx.restated_cost_h(case).tobytes() == ref["cost_h"].tobytes()
        eng.set_panda_weighted_cost_instance(-1)
        for name, table in Fx.TABLES.items():
            want = Fx.restated_cost_h(case, table)
            eng.set_panda_cost_weights(table)
            eng.rollout()
            torch.cuda.synchronize()
            reads = want.tobytes() != ref["cost_h"].tobytes()
            assert eng.panda_weighted_cost_instance_used() and eng.panda_lanes_per_sample_used() == lps
            assert_cost_horizon(eng, want, f"{case} lps {lps} {name}")
            if name == "random":
                assert reads
            # the states and actions read no weight; the trajectory cost is the discounted sum of these costs
            np.testing.assert_array_equal(eng.states.cpu().numpy().view(np.uint32), ref["states"].view(np.uint32))
            np.testing.assert_array_equal(eng.buffer(L.BUF_TRAJ_COST).cpu().numpy().view(np.uint32), discounted(want).view(np.uint32))
    finally:
        eng.close()


# ------------------------------------------------------------------ 9. values, step mode
def test_step_mode_cost_equals_the_restatement(P):
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    n = Fx.K
    sc = P.default_scene()
    w = np.concatenate([X.fuzz_worlds(), X.fuzz_worlds()[:n - 42]]).astype(F)       # the 42 fuzz worlds + 19 copies ...
    rng = np.random.default_rng(61)
    for _ in range(5):                                                                # ... stepped on, so that they differ
        u = rng.uniform(-2, 2, (n - 42, 9)).astype(F)
        tail = np.ascontiguousarray(w[42:])
        P.step_batch(sc, tail, u)
        w[42:] = tail
    w[0] = Fx.pick_world()                                                            # (a world that presses on the shelf stand)
    sim = IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=n, device="cuda:0")
    try:
        eng = sim._engine
        ia, ib, io = (int(sim._get_actor_index_by_name(x)) for x in ("cubeA", "cubeB", "dyn-obs"))
        dof = torch.zeros(n, 18)
        dof[:, 0::2] = torch.from_numpy(w[:, P.W_Q:P.W_Q + 9])
        dof[:, 1::2] = torch.from_numpy(w[:, P.W_QD:P.W_QD + 9])
        root = sim._root_state.clone().cpu()
        root[:, ia, :] = torch.from_numpy(w[:, P.W_CUBEA:P.W_CUBEA + 13])
        root[:, ib, :] = torch.from_numpy(w[:, P.W_CUBEB:P.W_CUBEB + 13])
        root[:, io, :] = torch.from_numpy(w[:, P.W_OBS:P.W_OBS + 13])
        sim._dof_state[:] = dof.to("cuda:0")
        sim._root_state[:] = root.to("cuda:0")
        sim.set_dof_state_tensor(sim._dof_state)
        sim.set_actor_root_state_tensor(sim._root_state)
        w[:, P.W_HELD:] = 0.0                      # a load from the wrapper's tensors: nothing derived, then inferred
        w[:, P.W_RELQ + 3] = 1.0
        w[:, P.W_AWAKE:P.W_AWAKE + 2] = 1.0
        for i in range(n):
            row = np.ascontiguousarray(w[i])
            P.infer_state(sc, row)
            w[i] = row
        for t in range(3):                         # steps, so that the contact forces the pick cost reads exist
            u = rng.uniform(-2, 2, (n, 9)).astype(F)
            u[:, 7:] = -1.5
            P.step_batch(sc, w, u)
            sim.set_dof_velocity_target_tensor(torch.from_numpy(u).to("cuda:0"))
            sim.step()
        obs = np.stack([P.observe(sc, w[e]) for e in range(n)])
        assert (np.abs(obs[:, 24:30]).sum(axis=1) > 0).sum() >= 3            # some worlds press on the table / shelf / cubeB
        for task, g, mm in (("reach", 1, False), ("reach", 1, True), ("pick", 2, False), ("place", 1, False)):
            o = obs.copy()
            if task == "reach":                    # quirk Q8 as m3_cost applies it
                o[:, 17:20], o[:, 20:24] = obs[0, 10:13], obs[0, 13:17]
                if mm:
                    o[n // 2:, 20:24] = obs[n // 2, 13:17]
            eng.set_multi_modal(mm)
            eng.set_objective(task, GOAL, gripper_cmd=g)
            cfg = P.make_cfg(n, Fx.T, multi_modal=mm, task=task, goal=GOAL, gripper_cmd=g)
            eng.set_panda_cost_weights(None)
            eng.set_panda_weighted_cost_instance(1)                          # the harness: the oracle's bits at the defaults
            got = eng.cost().cpu().numpy()
            assert eng.panda_weighted_cost_instance_used()
            np.testing.assert_array_equal(got.view(np.uint32), P.cost_obs(cfg, o).view(np.uint32), err_msg=task)
            eng.set_panda_weighted_cost_instance(-1)
            assert eng.cost().cpu().numpy().tobytes() == got.tobytes() and not eng.panda_weighted_cost_instance_used()
            for name, table in Fx.TABLES.items():
                eng.set_panda_cost_weights(table)
                got = eng.cost().cpu().numpy()
                want = R.cost_of_obs(task, o, goal=GOAL, w=R.weights(**table), multi_modal=mm, half_K=n // 2)
                assert eng.panda_weighted_cost_instance_used()
                np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"{task} mm {mm} {name}")
        # forced off with weights: m3_cost is refused; the step, which reads no weight, is not
        eng.set_panda_weighted_cost_instance(0)
        with pytest.raises(L.M3Error, match="m3_cost: .*forced off .*m3_set_panda_cost_weights"):
            eng.cost()
        sim.step()
    finally:
        sim.stop_sim()


# ------------------------------------------------------------------ 10. scaling
@pytest.mark.parametrize("case", ["reach", "pick", "place"])
def test_scaling_the_outer_weights_and_lambda_by_four_scales_the_costs_exactly(P, case):
    task = Fx.CASES[case][0]
    table = dict(Fx.RANDOM_TABLE)
    scaled = {n: (4.0 * v if n in R.OUTER[task] else v) for n, v in table.items()}
    assert scaled["shelf_force"] == table["shelf_force"]
    a = engine_of(case, weights=table)
    b = engine_of(case, weights=scaled, lambda_=4.0 * PK["lambda_"])
    # The temperature of the halton-spline update is beta, not lambda_ (mppi.py:430-454: exp(-1 / beta * (J - min J)), beta = 1
    # at the start and adapted from eta for the panda_env; lambda_ enters mppi_mode 'simple' alone), so the scaled handle starts
    # from 4 beta as well: (4 J) * (-1 / (4 beta)) has the bits of J * (-1 / beta), eta and with it every later beta follow.
    b.set_beta(4.0)
    try:
        for call in range(2):
            pa, pb = a.command(sync_host=True), b.command(sync_host=True)
            Ja, Jb = (e.buffer(L.BUF_TRAJ_COST).cpu().numpy() for e in (a, b))
            assert np.ptp(Ja) > 0 and (F(4.0) * Ja).tobytes() == Jb.tobytes(), call       # exactly: a power of two
            assert (F(4.0) * a.cost_horizon.cpu().numpy()).tobytes() == b.cost_horizon.cpu().numpy().tobytes()
            assert np.asarray(pa).tobytes() == np.asarray(pb).tobytes(), call
            for buf in (L.BUF_WEIGHTS, L.BUF_MEAN, L.BUF_ACTION_OUT, L.BUF_TOP_IDX, L.BUF_TOP_TRAJS, L.BUF_STATES):
                assert same_bytes(a, b, buf), (call, buf)
            assert F(4.0) * F(a.info().beta) == F(b.info().beta)
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------ 11. workspace and weights together
def test_combined_workspace_with_the_random_table(P):
    ref = Fx.oracle_case("pick", "COMBINED")
    dflt = Fx.oracle_case("pick")
    assert (ref["cost_h"].view(np.uint32) != dflt["cost_h"].view(np.uint32)).any(axis=1).mean() >= 0.5    # the scene shows
    want = Fx.restated_cost_h("pick", Fx.RANDOM_TABLE, "COMBINED")
    assert Fx.restated_cost_h("pick", None, "COMBINED").tobytes() == ref["cost_h"].tobytes()
    eng = engine_of("pick", lps=16, weights=Fx.RANDOM_TABLE, scene=X.COMBINED)
    try:
        eng.command(sync_host=True)
        assert eng.panda_weighted_cost_instance_used() and eng.panda_scene_instance_used()
        assert eng.panda_lanes_per_sample_used() == 16
        np.testing.assert_array_equal(eng.states.cpu().numpy().view(np.uint32), ref["states"].view(np.uint32))
        assert_cost_horizon(eng, want, "COMBINED + random table")
        # scene instance 0 with this geometry refuses as before, whatever the weights
        eng.set_panda_scene_instance(0)
        with pytest.raises(L.M3Error, match="forced off .*m3_set_panda_scene"):
            eng.command()
    finally:
        eng.close()


# ------------------------------------------------------------------ 12. refusals and life cycle
def test_refusals_launch_nothing(P):
    eng = engine_of("pick")
    pt = HipEngine(make_config(K=64, T=10, nu=2, env_type="point_env"))
    try:
        eng.set_panda_cost_weights(Fx.RANDOM_TABLE)
        for field in ("pick_ori", "shelf_force"):
            for bad in (float("nan"), float("inf")):
                with pytest.raises(L.M3Error, match=f"m3_set_panda_cost_weights: {field} is not finite"):
                    eng.set_panda_cost_weights({field: bad})
                assert bits(eng.panda_cost_weights()) == bits(Fx.RANDOM_TABLE)          # the handle is left unchanged
        with pytest.raises(L.M3Error, match="error -?\\d+: m3_set_panda_cost_weights: panda_env only") as ei:
            pt.set_panda_cost_weights(dict(pick_ori=25.0))
        assert f"error {ERR_UNSUPPORTED}:" in str(ei.value)
        with pytest.raises(L.M3Error, match="m3_set_panda_weighted_cost_instance: panda_env only"):
            pt.set_panda_weighted_cost_instance(1)
        assert eng.lib.m3_get_panda_cost_weights(pt._h, C.byref(L.PandaCostWeights())) == ERR_UNSUPPORTED
        # the existing refusal in the other direction stays
        with pytest.raises(L.M3Error, match="m3_set_point_cost_weights: point_env only"):
            eng.set_point_cost_weights(dict(push_align=2.0))
        # forced off with non-default weights: M3_ERR_STATE, nothing ran
        eng.set_panda_weighted_cost_instance(0)
        calls = eng.info().calls
        for run in (eng.command, eng.rollout):
            with pytest.raises(L.M3Error, match="forced off .*m3_set_panda_cost_weights") as ei:
                run()
            assert f"error {ERR_STATE}:" in str(ei.value)
        assert eng.info().calls == calls
        eng.set_panda_cost_weights(None)                                                # the defaults: nothing to refuse
        eng.command(sync_host=True)
        assert not eng.panda_weighted_cost_instance_used() and eng.info().calls == calls + 1
    finally:
        eng.close(); pt.close()


def test_setting_weights_allocates_nothing(P):
    eng = engine_of("pick")
    try:
        eng.command(sync_host=True)
        live = eng.lib.m3_owned_blocks_live()
        eng.set_panda_cost_weights(Fx.RANDOM_TABLE)
        eng.command(sync_host=True)
        eng.command(sync_host=True)
        assert eng.panda_weighted_cost_instance_used()
        assert eng.lib.m3_owned_blocks_live() == live
    finally:
        eng.close()


def test_batch_refuses_a_weighted_handle_and_then_works_without_it(P):
    engs = [engine_of("pick") for _ in range(3)]
    twins = [engine_of("pick") for _ in range(3)]
    batch = HipBatch(3)
    try:
        engs[1].set_panda_cost_weights(dict(pick_ori=25.0))
        infos = [bytes(e.info()) for e in engs]
        with pytest.raises(L.M3Error, match="m3_batch_command: handle 1: .*m3_set_panda_cost_weights") as ei:
            batch.command(engs)
        assert f"error {ERR_UNSUPPORTED}:" in str(ei.value)
        torch.cuda.synchronize()
        assert [bytes(e.info()) for e in engs] == infos                                 # nothing was launched
        engs[1].set_panda_weighted_cost_instance(0)                                     # forced off: refused for the other reason
        with pytest.raises(L.M3Error, match="handle 1: .*forced off"):
            batch.command(engs)
        batch.command([engs[0], engs[2]])                                               # the same batch without that handle
        for e in (twins[0], twins[2]):
            e.command()
        torch.cuda.synchronize()
        for i in (0, 2):
            for buf in COMMAND_BUFS:
                assert same_bytes(engs[i], twins[i], buf), (i, buf)
        assert engs[1].info().calls == 0
    finally:
        batch.close()
        for e in engs + twins:
            e.close()


def test_panda_episodes_refuse_a_weighted_planner_but_take_a_weighted_world(P):
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    n = 2
    world = IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=n, device="cuda:0")
    planners = [engine_of("reach") for _ in range(n)]
    try:
        for e in planners:
            e.set_action_out(torch.zeros(Fx.T, 9, device="cuda:0"))
        planners[1].set_panda_cost_weights(dict(reach_tilt=5.0))
        with pytest.raises(L.M3Error, match="m3_panda_episodes_create: planner 1: .*m3_set_panda_cost_weights") as ei:
            HipPandaEpisodes(world._engine, planners, max_ticks=4)
        assert f"error {ERR_UNSUPPORTED}:" in str(ei.value)
        planners[1].set_panda_cost_weights(None)
        world._engine.set_panda_cost_weights(dict(pick_ori=25.0))                       # a sim_only world: its step reads no weight
        eps = HipPandaEpisodes(world._engine, planners, max_ticks=4)
        try:
            planners[0].set_panda_cost_weights(dict(reach_dist=20.0))                 # set after create: the tick is refused
            with pytest.raises(L.M3Error, match="planner 0: .*m3_set_panda_cost_weights"):
                eps.observe()
        finally:
            eps.close()
    finally:
        world.stop_sim()
        for e in planners:
            e.close()


def test_two_shards_equal_the_unsharded_handle(P):
    k, task, grip = Fx.K_MM, "pick", 2              # (K = 62: two shards of 31, k_offset 0 and 31)

    def make(**kw):
        eng = HipEngine(make_config(K=k, T=Fx.T, nu=9, env_type="panda_env", **{**PK, **kw}))
        eng.set_objective(task, GOAL, gripper_cmd=grip)
        k0 = kw.get("k_offset", 0)
        eng.set_noise(Fx.delta_of(k)[k0:k0 + kw.get("K_local", k)])
        eng.set_panda_cost_weights(Fx.RANDOM_TABLE)
        eng.set_world_panda_raw(P.raw57(Fx.pick_world()))
        return eng

    full, lo, hi = make(), make(K_local=31, k_offset=0), make(K_local=31, k_offset=31)
    try:
        for e in (full, lo, hi):
            e.rollout()
        torch.cuda.synchronize()
        assert all(e.panda_weighted_cost_instance_used() for e in (full, lo, hi))
        J = full.buffer(L.BUF_TRAJ_COST).cpu().numpy()
        parts = np.concatenate([e.buffer(L.BUF_TRAJ_COST).cpu().numpy() for e in (lo, hi)])
        assert np.ptp(J) > 0 and J.tobytes() == parts.tobytes()
    finally:
        for e in (full, lo, hi):
            e.close()


# ------------------------------------------------------------------ 13. the planner, end to end
def test_planner_from_a_config_with_panda_cost_weights_keeps_the_fused_path(P):
    from m3p2i_aip_amd import compat
    from tests.test_planner_api_panda_gpu import Tamp
    table = dict(pick_ori=25.0, collision=500.0)
    cfg = compat.make_config("config_panda", ["panda_cost_weights={pick_ori: 25.0, collision: 500.0}", "mppi.num_samples=200",
                                              "mppi.horizon=12", "mppi.u_per_command=12"])
    assert cfg.panda_cost_weights == table
    tamp = Tamp(cfg)
    try:
        pl = tamp.motion_planner
        pl.update_gripper_command("pick")
        tamp.objective.update_objective("pick", torch.tensor(list(Fx.GOAL)))
        for call in range(2):
            a = pl.command(tamp.sim._dof_state[0])
            assert torch.isfinite(a).all()
            assert pl._engine.panda_weighted_cost_instance_used()
            assert pl._engine.panda_cost_weights() == {**L.PANDA_COST_WEIGHT_DEFAULTS, **table}
        # the probe of the first command took the fused path: its two legs -- the fused rollout and step + m3_cost on the wrapper's
        # engine -- are both weighted
        assert pl.probe_result["fused"] is True and pl.probe_result["max_abs_diff"] == 0.0
        assert tamp.sim._engine.panda_cost_weights() == {**L.PANDA_COST_WEIGHT_DEFAULTS, **table}
        assert tamp.sim._engine.panda_weighted_cost_instance_used()
    finally:
        tamp.sim.stop_sim()
