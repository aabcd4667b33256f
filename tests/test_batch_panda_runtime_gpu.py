"""m3_batch_command on a batch created with M3_BATCH_PANDA_RUNTIME (include/m3p2i_hip.h): panda_env
handles with a run-time workspace (m3_set_panda_scene), tuned cost weights (m3_set_panda_cost_weights) or a workspace per sample
(m3_set_panda_rollout_scenes) in one batched call.

Every comparison is byte equality with a TWIN handle, configured identically, that ran its own m3_command: every buffer of
BUFS, m3_info and the four *_used getters.  The twins are themselves pinned to the oracle by tests/test_panda_scene_gpu.py,
tests/test_panda_cost_weights_gpu.py and tests/test_panda_scene_rows_gpu.py, so no tolerance is stated anywhere.

A batch that ignored the scene, the weights or the rows must not pass: every case asserts that its twin's TRAJ_COST differs from
that of a default-scene, default-weight twin.  The entries were chosen on the CPU oracle at these shapes (T = 10): the reach
cycle's scenes on fuzz world 41; for pick the world of tests/panda_cost_fixture.py (the held cube at the shelf stand -- on fuzz
world 40 nothing touches anything within ten steps and no workspace shows) with mu, base and COMBINED; for place fuzz world 22
with base, COMBINED and shelf_x.  The rows are the 5-cycles of tests/test_panda_scene_rows_gpu.py (row i = cycle[(i + offset) %
5]; 5 is coprime to every samples-per-wavefront count, so a kernel that indexed the rows by lane, slot or handle cannot pass).

Shapes: K = 64 and K = 61 (a ragged last wavefront; at sixteen lanes per sample wavefronts whose shadow slots do not fill),
T = 10; lanes per sample forced to 1, 8 and 16.
"""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, make_config  # noqa: E402
from tests import panda_cost_fixture as Fx  # noqa: E402
from tests import panda_rollout_scenes_ref as R  # noqa: E402
from tests import panda_scene_fixture as X  # noqa: E402

F = np.float32
T = 10
PK = dict(u_min=X.UMIN, u_max=X.UMAX, noise_sigma_diag=X.SIG, lambda_=0.05, pre_height_diff=0.05, dt=0.01)
GOAL = np.array(X.GOAL, F)
ERR_BAD_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5          # (include/m3p2i_hip.h)
BUFS = [L.BUF_ACTIONS, L.BUF_STATES, L.BUF_COST_HORIZON, L.BUF_TRAJ_COST, L.BUF_WEIGHTS, L.BUF_WEIGHTS_1, L.BUF_WEIGHTS_2,
        L.BUF_MEAN, L.BUF_MEAN_1, L.BUF_MEAN_2, L.BUF_BEST, L.BUF_BEST_1, L.BUF_BEST_2, L.BUF_ACTION_OUT, L.BUF_TOP_IDX,
        L.BUF_TOP_TRAJS]
# task -> objective, gripper command, world (a fuzz world of panda_scene_fixture, or the pick fixture's), the three workspaces
# of a batch's three handles, the 5-cycle its rows are taken from
TASKS = {
    "reach": ("reach", 2, 41, ("table_z", "mu", "base"), "reach"),
    "pick": ("pick", 2, "pick_world", ("mu", "base", "COMBINED"), "pick"),
    "place": ("place", 1, 22, ("base", "COMBINED", "shelf_x"), "pick"),
}
# three weight tables that move every weight (so every task's cost reads a changed one)
TABLES = (Fx.RANDOM_TABLE,
          dict(reach_dist=20.0, reach_tilt=5.0, pick_goal=7.5, pick_ori=25.0, collision=500.0, shelf_force=3.0, place_grip=3.0),
          {n: 0.5 * v for n, v in Fx.RANDOM_TABLE.items()})
VARIANTS = ("scene", "weights", "scene+weights", "rows", "rows+weights")
# form -> task, m3_set_panda_reach_cost_kernel
FORMS = {"reach_record": ("reach", True), "reach_shadow_slots": ("reach", False), "pick": ("pick", True), "place": ("place", True)}


@pytest.fixture(scope="module")
def P(oracle):
    import oracle.panda as P
    P.lib()
    return P


@pytest.fixture(scope="module")
def flagged():
    b = HipBatch(16, panda_runtime=True)
    yield b
    b.close()


def world_of(P, task):
    spec = TASKS[task][2]
    return P.raw57(Fx.pick_world().copy() if spec == "pick_world" else X.world_of(spec))


def delta_of(K):
    return np.ascontiguousarray(X.delta_of(K)[:, :T])


def settings_of(task, variant, j, K):
    """what handle j of a batch of `variant` is given: (scene, weights, rows)"""
    scene = X.SCENES[TASKS[task][3][j]] if "scene" in variant else None
    weights = TABLES[j] if "weights" in variant else None
    rows = R.cycle_rows(TASKS[task][4], K, offset=j) if "rows" in variant else None
    return scene, weights, rows


def engine_of(P, K, task, lps=0, cost_kernel=True, scene=None, weights=None, rows=None, mm=False, **kw):
    name, grip = TASKS[task][:2]
    eng = HipEngine(make_config(K=K, T=T, nu=9, env_type="panda_env", multi_modal=mm, **{**PK, **kw}))
    eng.set_objective(name, GOAL, gripper_cmd=grip)
    eng.set_panda_lanes_per_sample(lps)
    eng.set_panda_reach_cost_kernel(cost_kernel)
    k0 = kw.get("k_offset", 0)
    eng.set_noise(delta_of(K)[k0:k0 + kw.get("K_local", K)])
    if scene is not None:
        eng.set_panda_scene(scene)
    if weights is not None:
        eng.set_panda_cost_weights(weights)
    if rows is not None:
        eng.set_panda_rollout_scenes(rows)
    eng.set_world_panda_raw(world_of(P, task))
    return eng


def buf_bytes(eng, which):
    try:
        return eng.buffer(which).cpu().numpy().tobytes()
    except L.M3Error:
        return None          # (not allocated for this handle, e.g. the per-mode buffers of a single-mode one: on both sides then)


def used(eng):
    return (eng.panda_lanes_per_sample_used(), eng.panda_near_share(), bool(eng.panda_scene_instance_used()),
            bool(eng.panda_weighted_cost_instance_used()))


def assert_same(a, b, label):
    """handle a (batched) against its twin b (own m3_command): buffers, m3_info (calls included), what ran"""
    torch.cuda.synchronize()
    for buf in BUFS:
        assert buf_bytes(a, buf) == buf_bytes(b, buf), (label, buf)
    assert buf_bytes(a, L.BUF_TRAJ_COST) is not None and buf_bytes(a, L.BUF_ACTION_OUT) is not None
    assert bytes(a.info()) == bytes(b.info()), label
    assert used(a) == used(b), (label, used(a), used(b))


def traj_cost(eng):
    return eng.buffer(L.BUF_TRAJ_COST).cpu().numpy().copy()


def close_all(engs):
    for e in engs:
        e.close()


# ------------------------------------------------------------------ 1. each variant, each form
@pytest.mark.parametrize("K", [64, 61])
@pytest.mark.parametrize("lps", [1, 8, 16])
@pytest.mark.parametrize("form", list(FORMS))
def test_each_variant_in_each_form_equals_its_twins(P, flagged, form, lps, K):
    task, cost_kernel = FORMS[form]
    plain = engine_of(P, K, task, lps, cost_kernel)
    try:
        plain.command()
        base = traj_cost(plain)
        assert np.isfinite(base).all() and np.ptp(base) > 0
    finally:
        plain.close()
    for variant in VARIANTS:
        sets = [settings_of(task, variant, j, K) for j in range(3)]
        engs = [engine_of(P, K, task, lps, cost_kernel, *s) for s in sets]
        twins = [engine_of(P, K, task, lps, cost_kernel, *s) for s in sets]
        try:
            for call in range(2):                          # (the second command goes through the warm start)
                flagged.command(engs)
                assert flagged.launches() == (1, 1), (variant, flagged.launches())      # one key: one rollout, one update launch
                for t in twins:
                    t.command()
                for j, (e, t) in enumerate(zip(engs, twins)):
                    assert_same(e, t, (form, lps, K, variant, j, call))
                    assert e.panda_lanes_per_sample_used() == lps
                    assert bool(e.panda_scene_instance_used()) == (variant != "weights")
                    assert bool(e.panda_weighted_cost_instance_used()) == ("weights" in variant)
                    if call == 0:       # the scene, the weights or the rows show: a batch that ignored them cannot pass
                        assert traj_cost(t).tobytes() != base.tobytes(), (form, lps, K, variant, j)
            # the three handles differ in their values, and so do their results
            assert len({traj_cost(e).tobytes() for e in engs}) == 3, (form, variant)
        finally:
            close_all(engs + twins)


@pytest.mark.parametrize("variant,lps,cost_kernel", [("rows", 16, False), ("rows", 1, False), ("rows+weights", 16, True),
                                                     ("scene+weights", 8, True)])
def test_multi_modal_reach(P, flagged, variant, lps, cost_kernel):
    """quirk Q8 reads sample K / 2 as well -- with rows, as simulated in ITS row"""
    K = 64
    plain = engine_of(P, K, "reach", lps, cost_kernel, mm=True)
    sets = [settings_of("reach", variant, j, K) for j in range(3)]
    engs = [engine_of(P, K, "reach", lps, cost_kernel, *s, mm=True) for s in sets]
    twins = [engine_of(P, K, "reach", lps, cost_kernel, *s, mm=True) for s in sets]
    try:
        plain.command()
        base = traj_cost(plain)
        for call in range(2):
            flagged.command(engs)
            for t in twins:
                t.command()
            for j, (e, t) in enumerate(zip(engs, twins)):
                assert_same(e, t, (variant, lps, j, call))
                assert buf_bytes(e, L.BUF_MEAN_2) is not None and e.panda_lanes_per_sample_used() == lps
                if call == 0:
                    assert traj_cost(t).tobytes() != base.tobytes()
    finally:
        close_all([plain] + engs + twins)


# ------------------------------------------------------------------ 2. a mixed call
def mixed_specs():
    """(task, K, lps, cost_kernel, variant (None: literal), index of the values) of one call's handles"""
    return [
        ("pick", 64, 16, True, None, 0), ("reach", 61, 16, True, None, 0),                 # two literal handles
        ("pick", 64, 16, True, "scene", 0), ("reach", 61, 16, True, "scene", 1),           # two scene handles ...
        ("pick", 64, 16, True, "weights", 1), ("place", 61, 8, True, "weights", 2),        # ... two weighted ones
        ("pick", 64, 16, True, "rows", 0), ("reach", 64, 1, False, "rows+weights", 1),     # ... two with rows
        ("reach", 64, 8, False, None, 0), ("pick", 61, 1, True, None, 0), ("place", 64, 16, True, None, 0),   # one more of each task
    ]


def key_of(spec):
    """the rollout key m3_batch_command groups by, from the handle's form: family, lanes per sample, FORCES, shadow slots,
    record kept, K (T is shared; the adjusted lanes follow from lanes per sample and the shadow slots)"""
    task, K, lps, cost_kernel, variant, _ = spec
    family = 0 if variant is None else 2 if "rows" in variant else 1
    record = task == "reach" and cost_kernel and lps != 1
    shadows = 1 if task == "reach" and not record else 0
    return (family, lps, task == "pick", shadows, record, K)


def build_mixed(P):
    out = []
    for task, K, lps, cost_kernel, variant, j in mixed_specs():
        s = settings_of(task, variant, j, K) if variant else (None, None, None)
        out.append(engine_of(P, K, task, lps, cost_kernel, *s))
    return out


def test_one_mixed_call_in_shuffled_order(P, flagged):
    specs = mixed_specs()
    engs, twins = build_mixed(P), build_mixed(P)
    order = list(range(len(specs)))
    random.Random(7).shuffle(order)
    assert order != sorted(order)
    dst = [torch.zeros(T, 9, device="cuda:0") for _ in specs]
    tdst = [torch.zeros(T, 9, device="cuda:0") for _ in specs]
    try:
        for e, d in zip(engs + twins, dst + tdst):
            e.set_action_out(d)                                                          # the m3_set_action_out destination
        for call in range(2):
            flagged.command([engs[i] for i in order])
            # each group of handles that share a key is one rollout launch
            assert flagged.launches()[0] == len({key_of(s) for s in specs}) == 10
            for t in twins:
                t.command()
            for i, (e, t) in enumerate(zip(engs, twins)):
                assert_same(e, t, (specs[i], call))
                assert dst[i].cpu().numpy().tobytes() == tdst[i].cpu().numpy().tobytes(), specs[i]
                assert np.abs(dst[i].cpu().numpy()).sum() > 0
                assert e.panda_lanes_per_sample_used() == specs[i][2]
        for i in (0, 1):                                                                 # the two literal handles
            assert not engs[i].panda_scene_instance_used() and not engs[i].panda_weighted_cost_instance_used()
        # the two pick handles of family 1 shared a launch, and differ
        assert key_of(specs[2]) == key_of(specs[4]) and traj_cost(engs[2]).tobytes() != traj_cost(engs[4]).tobytes()
    finally:
        close_all(engs + twins)


# ------------------------------------------------------------------ 3. default handles in a flagged batch
def test_default_handles_in_a_flagged_batch_are_the_unflagged_batchs(P, flagged):
    specs = [("reach", 64, 16, True), ("reach", 61, 1, False), ("pick", 61, 8, True), ("place", 64, 16, True)]
    a = [engine_of(P, K, task, lps, ck) for task, K, lps, ck in specs]
    b = [engine_of(P, K, task, lps, ck) for task, K, lps, ck in specs]
    forced = [engine_of(P, K, task, lps, ck) for task, K, lps, ck in specs]      # family 1 at the default values
    plain = HipBatch(4)
    try:
        assert plain.flags() == 0 and flagged.flags() == L.BATCH_PANDA_RUNTIME
        for i, e in enumerate(forced):
            if i % 2 == 0:
                e.set_panda_scene_instance(1)
            else:
                e.set_panda_weighted_cost_instance(1)
        for call in range(2):
            flagged.command(a)
            assert flagged.launches()[0] == 4
            plain.command(b)
            assert plain.launches()[0] == 4
            flagged.command(forced)
            torch.cuda.synchronize()
            for i, (x, y, z) in enumerate(zip(a, b, forced)):
                for buf in BUFS:
                    assert buf_bytes(x, buf) == buf_bytes(y, buf) == buf_bytes(z, buf), (specs[i], buf, call)
                assert bytes(x.info()) == bytes(y.info()) == bytes(z.info())
                assert used(x)[:2] == used(y)[:2] == used(z)[:2]
                assert used(x)[2:] == (False, False)                                     # the literal kernels ran
                assert used(z)[2:] == ((True, False) if i % 2 == 0 else (False, True))   # as m3_rollout would report it
        assert np.ptp(traj_cost(a[0])) > 0
    finally:
        plain.close()
        close_all(a + b + forced)


# ------------------------------------------------------------------ 4. refusals
def test_refusals_launch_nothing(P, flagged):
    K = 64
    good = engine_of(P, K, "pick")
    scene = engine_of(P, K, "pick", scene=X.SCENES["mu"])
    weights = engine_of(P, K, "pick", weights=TABLES[0])
    rows = engine_of(P, K, "pick", rows=R.cycle_rows("pick", K))
    engs = [good, scene, weights, rows]       # the planner handles whose m3_info is watched
    made = list(engs)
    plain = HipBatch(4)

    def refused(batch, hs, code, pattern):
        before = [bytes(e.info()) for e in engs]
        with pytest.raises(L.M3Error, match=pattern) as ei:
            batch.command(hs)
        assert f"error {code}:" in str(ei.value), str(ei.value)
        torch.cuda.synchronize()
        assert [bytes(e.info()) for e in engs] == before                                 # nothing was launched

    try:
        # a batch without the flag: the three existing refusals, word for word
        refused(plain, [good, scene], ERR_UNSUPPORTED, "m3_batch_command: handle 1: its workspace \\(m3_set_panda_scene\\) needs the "
                "run-time-scene instance, which only m3_rollout / m3_command and the handle's own step, cost and views run")
        refused(plain, [good, weights], ERR_UNSUPPORTED, "m3_batch_command: handle 1: its cost weights \\(m3_set_panda_cost_weights\\) need "
                "the weighted cost instance, which only m3_rollout / m3_command and the handle's own m3_cost run")
        refused(plain, [good, rows], ERR_UNSUPPORTED, "m3_batch_command: handle 1: it has a workspace per sample "
                "\\(m3_set_panda_rollout_scenes\\), which only m3_rollout / m3_command run")
        # the flagged batch: forced off is M3_ERR_STATE, as m3_rollout's
        scene.set_panda_scene_instance(0)
        refused(flagged, [good, scene], ERR_STATE, "handle 1: .*forced off \\(m3_set_panda_scene_instance 0\\).*m3_set_panda_scene")
        scene.set_panda_scene_instance(-1)
        rows.set_panda_scene_instance(0)
        refused(flagged, [good, rows], ERR_STATE, "handle 1: .*forced off .*m3_set_panda_rollout_scenes")
        rows.set_panda_scene_instance(-1)
        weights.set_panda_weighted_cost_instance(0)
        refused(flagged, [good, weights], ERR_STATE, "handle 1: .*forced off \\(m3_set_panda_weighted_cost_instance 0\\)")
        weights.set_panda_weighted_cost_instance(-1)
        # ... and whatever else a batch refuses
        sharded = engine_of(P, K, "pick", scene=X.SCENES["mu"], K_local=32, k_offset=0)
        engs.append(sharded); made.append(sharded)
        refused(flagged, [good, scene, sharded], ERR_STATE, "handle 2: sharded")
        sim = HipEngine(make_config(K=K, T=T, nu=9, env_type="panda_env", sim_only=True, **PK))
        made.append(sim)
        sim.set_panda_scene(X.SCENES["mu"])
        refused(flagged, [good, sim], ERR_STATE, "handle 1: handle was created sim_only")
        big = engine_of(P, 4100, "pick", weights=TABLES[0])
        engs.append(big); made.append(big)
        refused(flagged, [good, big], ERR_UNSUPPORTED, "handle 1: its command does not take the one-launch update \\(nu = 9: K <= 4096")
        point = HipEngine(make_config(K=64, T=10, nu=2, env_type="point_env"))
        made.append(point)
        refused(flagged, [scene, point], ERR_UNSUPPORTED, "handle 1: point_env handle in a batch of panda_env handles")
        refused(flagged, [scene, scene], ERR_BAD_ARG, "handle 1: handle listed twice")
        # unknown flag bits at create
        out = C.c_void_p()
        assert good.lib.m3_batch_create_ex(0, 4, 2, C.byref(out)) == ERR_BAD_ARG and not out
        assert good.lib.m3_batch_create_ex(0, 4, 3, C.byref(out)) == ERR_BAD_ARG and not out
        # after all that the same batch takes the same handles
        flagged.command([good, scene, weights, rows])
        assert flagged.launches()[0] == 3
        torch.cuda.synchronize()
        assert [e.info().calls for e in (good, scene, weights, rows)] == [1, 1, 1, 1]
    finally:
        plain.close()
        close_all(made)


# ------------------------------------------------------------------ 5. no allocation, ring reuse
def test_a_call_allocates_nothing_and_the_ring_is_reused(P):
    lib = L.load()
    torch.cuda.synchronize()
    start = lib.m3_owned_blocks_live()
    engs, twins = build_mixed(P), build_mixed(P)
    batch = HipBatch(len(engs), panda_runtime=True)
    try:
        batch.command(engs)
        for t in twins:
            t.command()
        torch.cuda.synchronize()
        live = lib.m3_owned_blocks_live()
        assert live > start
        for call in range(6):                                 # more calls than the ring has slots (4)
            batch.command(engs if call % 2 == 0 else list(reversed(engs)))
            assert lib.m3_owned_blocks_live() == live, call
            for t in twins:
                t.command()
        assert lib.m3_owned_blocks_live() == live
        for i, (e, t) in enumerate(zip(engs, twins)):
            assert_same(e, t, ("after the ring went round", i))
    finally:
        batch.close()
        close_all(engs + twins)
    assert lib.m3_owned_blocks_live() == start


# ------------------------------------------------------------------ 6. the planner
def test_command_batch_with_panda_runtime_equals_each_planners_own_command(P):
    from m3p2i_aip_amd import planner as planner_mod
    from tests.test_planner_api_panda_gpu import Tamp, make_cfg
    K, TP = 64, 12          # (the planner's own halton-spline sampler needs a horizon of at least 12: three knots)
    goal = torch.tensor(list(X.GOAL))

    def trio():
        ts = [Tamp(make_cfg(K, TP, fused=True)) for _ in range(3)]
        for t in ts:
            t.motion_planner.attach(t.sim, t.objective)
            t.motion_planner.update_gripper_command("pick")
            t.objective.update_objective("pick", goal)
        ts[0].objective.set_panda_cost_weights(pick_ori=25.0, collision=500.0)             # panda_cost_weights
        ts[1].sim.panda_scene = L.panda_scene_dict(L.panda_scene_fields(X.COMBINED))       # a panda_scene the planner follows
        ts[2].motion_planner.set_panda_rollout_scenes(R.cycle_rows("pick", K))
        return ts

    a, b = trio(), trio()
    try:
        states = [t.sim._dof_state[0].clone() for t in a]
        with pytest.raises(ValueError, match="planner 0 has panda cost weights of its own"):
            planner_mod.command_batch([t.motion_planner for t in a], states)               # the default stays as it was
        for tick in range(2):
            got = planner_mod.command_batch([t.motion_planner for t in a], states, panda_runtime=True)
            assert planner_mod._BATCHES_PANDA_RUNTIME[0].flags() == L.BATCH_PANDA_RUNTIME
            want = [t.motion_planner.command(s) for t, s in zip(b, states)]
            torch.cuda.synchronize()
            for i, (x, y) in enumerate(zip(got, want)):
                assert x.shape == y.shape == (TP, 9) and torch.isfinite(x).all()
                assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (tick, i)
                assert_same(a[i].motion_planner._engine, b[i].motion_planner._engine, ("planner", tick, i))
        ea = [t.motion_planner._engine for t in a]
        assert ea[0].panda_weighted_cost_instance_used() and not ea[0].panda_scene_instance_used()
        assert ea[1].panda_scene_instance_used() and not ea[1].panda_weighted_cost_instance_used()
        assert ea[2].panda_rollout_scenes_set() and ea[2].panda_scene_instance_used()
    finally:
        for t in a + b:
            t.motion_planner._engine.close()
            t.sim.stop_sim()
