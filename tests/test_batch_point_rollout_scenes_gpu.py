"""m3_batch_command for point_env handles with an arena per sample (m3_batch_create_sections with
M3_BATCH_SECTION_POINT_ROLLOUT_SCENES).  Handle A_i goes through the batch, its twin B_i through its own
m3_command; after every call every buffer of tests/test_batch_command_gpu.BUFS and every field of m3_info must be the same
BYTES.  Handle i's rows are cycle_rows(K, shift=i), so a handle that read a neighbour's table would differ -- on the oracle
alone the cycle is first shown to be felt for every shift used (at least 0.8 of the samples differ from the next and the
previous row's arena, 0.5 from the default arena: conditions, not tolerances).  One handle is also held to the stitched CPU
oracle, bit for bit.  Refused calls leave every handle as it was."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, make_config  # noqa: E402
from tests import point_scene_fixture as X  # noqa: E402
from tests import rollout_scenes_fixture as R  # noqa: E402
from tests.test_batch_command_gpu import PK, Twin, _noise  # noqa: E402
from tests.test_hip_parity_point import raw_world  # noqa: E402
from tests.test_point_scene_gpu import TASKS, W_TUNED, _assert_rollout_bits  # noqa: E402

T = X.T          # 8
GOAL = X.GOAL
POINT = L.BATCH_SECTION_POINT_ROLLOUT_SCENES


@pytest.fixture(scope="module")
def rows_matter(oracle):
    """once per module, on the oracle alone: every shift of the cycle the cases use (period three) is felt by the samples"""
    w0 = X.start_worlds(oracle)[2]
    for shift in range(3):
        R.assert_rows_matter(oracle, "push", False, 64, w0, f"push K=64 shift {shift}", rows=R.cycle_rows(64, shift))
    R.assert_rows_matter(oracle, "push_pull", True, 100, w0, "push_pull K=100 shift 1", rows=R.cycle_rows(100, 1))
    return True


@pytest.fixture
def twins():
    made = []
    yield made
    for t in made:
        t.close()


def _rows(t, rows):
    for e in t.engs:
        e.set_point_rollout_scenes(rows)


def _twin(made, i, K, task="push", mm=False, shift=None, **kw):
    """twin i with the rows cycle_rows(K, shift) on both handles (shift None: no rows)"""
    kw.setdefault("filter_u", False)
    t = Twin(i, K=K, T=T, task=task, goal=GOAL, multi_modal=mm, **kw)
    made.append(t)
    if shift is not None:
        _rows(t, R.cycle_rows(K, shift))
    return t


def _run(twins, calls=6, before=None, max_handles=None):
    """before(call): what changes ahead of that call.  Returns the launches of every call."""
    batch = HipBatch(max_handles or len(twins), point_runtime=True)
    launches = []
    try:
        assert batch.flags() == POINT
        for c in range(calls):
            if before:
                before(c)
            for t in twins:
                t.set_world(c)
            batch.command([t.A for t in twins])
            for t in twins:
                t.B.command()
            torch.cuda.synchronize()
            for t in twins:
                assert t.assert_same(f"call {c}") == c + 1
            launches.append(batch.launches())
        return launches
    finally:
        batch.close()


# ------------------------------------------------------------------ 1. twin equality
def _case_a(twins):
    for i in range(3):
        _twin(twins, i, 64, shift=i)
    for i in range(3, 5):
        _twin(twins, i, 100, shift=i)      # (100: a half-empty second wavefront)
    return twins


def test_a_two_sizes_in_one_call_give_two_per_sample_groups(rows_matter, twins):
    launches = _run(_case_a(twins))
    assert all(roll == 2 for roll, _ in launches), launches
    assert all(t.A.point_rollout_scenes_set() for t in twins)


def test_b_the_four_tasks_tuned_weights_and_update_cov_share_one_launch(rows_matter, twins):
    for i, (task, mm) in enumerate(TASKS):
        _twin(twins, i, 100, task=task, mm=mm, shift=i)
    tuned = _twin(twins, 4, 100, shift=4)
    for e in tuned.engs:
        e.set_point_cost_weights(W_TUNED)
    _twin(twins, 5, 100, shift=5, update_cov=True)
    _twin(twins, 6, 100, task="push_pull", mm=True, shift=6, dt=0.04, substeps=3)   # (uniform members are per handle)
    launches = _run(twins)
    assert all(roll == 1 for roll, _ in launches), launches


def test_c_one_call_with_all_four_sections(rows_matter, twins):
    _twin(twins, 0, 64)
    weighted = _twin(twins, 1, 64)
    for e in weighted.engs:
        e.set_point_cost_weights(W_TUNED)
    scene = _twin(twins, 2, 64)
    for e in scene.engs:
        e.set_point_scene(X.CUSTOM)
    _twin(twins, 3, 64, shift=1)
    # (call order is not section order: the per-sample handle first)
    twins[:] = [twins[3], twins[0], twins[2], twins[1]]
    launches = _run(twins)
    assert all(roll == 4 for roll, _ in launches), launches


def test_d_rows_replaced_and_cleared_between_calls(rows_matter, twins):
    _twin(twins, 0, 64, shift=0)
    _twin(twins, 1, 64, shift=1)

    def before(c):
        if c == 2:        # between calls 2 and 3: other rows on both twins
            for i, t in enumerate(twins):
                _rows(t, R.cycle_rows(64, i + 1))
        if c == 4:        # before call 5: handle 0 back on its single scene -- another section of the table
            _rows(twins[0], None)

    launches = _run(twins, before=before, max_handles=5)
    assert [roll for roll, _ in launches] == [1, 1, 1, 1, 2, 2]
    assert not twins[0].A.point_rollout_scenes_set() and twins[1].A.point_rollout_scenes_set()


def test_e_wave_order_relabelled_noise_and_bound_views(rows_matter, twins):
    _twin(twins, 0, 100, shift=0, wave_order=False)
    _twin(twins, 1, 100, shift=1, relabel=True)
    _twin(twins, 2, 100, shift=2, bind=True, action_out=True)
    _twin(twins, 3, 100, shift=3)
    launches = _run(twins)
    assert all(roll == 1 for roll, _ in launches), launches


# ------------------------------------------------------------------ 2. the occ builds through the group rule
@pytest.mark.parametrize("n,K,build", [(17, 64, "occ2"), (33, 128, "occ3")])
def test_the_group_wavefront_count_picks_the_occ_builds(twins, n, K, build):
    """one sample per wavefront: 17 * 64 = 1088 wavefronts (> 1024: occ2), 33 * 128 = 4224 (> 4096: occ3) -- no handle reaches the
    threshold on its own, so its twin's m3_command runs the lone build: same bits"""
    for i in range(n):
        t = _twin(twins, i, K, shift=i)
        for e in t.engs:
            e.set_rollout_lanes(1)
    launches = _run(twins, calls=3)
    assert all(roll == 1 for roll, _ in launches), (build, launches)


# ------------------------------------------------------------------ 3. against the reference
def test_a_batched_handle_equals_the_stitched_oracle(oracle, rows_matter, twins):
    """handle 0 of case (a) on the fixture's noise and start world: the first batched command's rollout against the CPU
    oracle rolling each sample out in its own arena, bit for bit"""
    _case_a(twins)
    w0 = X.start_worlds(oracle)[2]
    for e in twins[0].engs:
        e.set_noise(X.actions(64, T))
    opl = R.make_stitched(oracle, oracle.make_cfg(64, T, 2, task="push", goal=GOAL, multi_modal=False, filter_u=False),
                          X.actions(64, T), R.cycle_rows(64, 0))
    batch = HipBatch(5, point_runtime=True)
    try:
        for t in twins:
            t.set_world(0)
        for e in twins[0].engs:
            e.set_world_point_raw(raw_world(w0))
        batch.command([t.A for t in twins])
        twins[0].B.command()
        torch.cuda.synchronize()
        opl.command(w0)
        _assert_rollout_bits(twins[0].A, opl, "batched handle 0 vs the stitched oracle")
        assert twins[0].assert_same("call 0") == 1
    finally:
        batch.close()


# ------------------------------------------------------------------ 4. refusals
def _state(ts):
    torch.cuda.synchronize()
    return [(t.A.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes(), t.A.buffer(L.BUF_MEAN).cpu().numpy().tobytes(), t.A.info().calls)
            for t in ts]


def _refused(batch, engines, code, fragment, ts):
    before = _state(ts)
    with pytest.raises(L.M3Error, match=rf"error {code}: .*{fragment}"):
        batch.command(engines)
    assert _state(ts) == before


def test_batches_without_the_section_refuse_with_todays_message(twins):
    for i in range(3):
        _twin(twins, i, 64, shift=1 if i == 1 else None)
    for t in twins:
        t.set_world(0)
    for batch in (HipBatch(3), HipBatch(3, panda_runtime=True)):
        try:
            assert batch.flags() in (0, L.BATCH_PANDA_RUNTIME)
            _refused(batch, [t.A for t in twins], -5,
                     r"handle 1: it has an arena per sample \(m3_set_point_rollout_scenes\), which only m3_rollout / m3_command run", twins)
        finally:
            batch.close()
    batch = HipBatch(3)
    try:
        batch.command([twins[0].A, twins[2].A])
        twins[0].B.command(); twins[2].B.command()
        torch.cuda.synchronize()
        assert twins[0].assert_same("after the refusal") == 1 and twins[2].assert_same("after the refusal") == 1
    finally:
        batch.close()


def test_unknown_section_bits_are_refused():
    lib = L.load()
    torch.zeros(1, device="cuda:0")
    for bits in (4, 1 | 4, 2 | 8, -1):
        out = C.c_void_p(1)
        assert lib.m3_batch_create_sections(0, 4, bits, C.byref(out)) == -1 and out.value is None
        assert b"unknown section bits" in lib.m3_batch_last_error(None)
    for bits in (0, 1, 2, 3):
        out = C.c_void_p()
        assert lib.m3_batch_create_sections(0, 4, bits, C.byref(out)) == 0
        assert lib.m3_batch_flags(out) == bits
        lib.m3_batch_destroy(out)


def test_the_new_batch_keeps_the_other_refusals(twins):
    K = 64
    good = _twin(twins, 0, K, shift=0)
    other = _twin(twins, 1, K, shift=1)
    for t in twins:
        t.set_world(0)
    rows = R.cycle_rows(K)
    made = []

    def eng(task="push", noise=True, rows=None, **kw):
        e = HipEngine(make_config(T=T, nu=kw.pop("nu", 2), filter_u=False, **{**PK, **kw}))
        made.append(e)
        if noise:
            e.set_noise(_noise(e.cfg.K_local, T, 7))
        if task:
            e.set_objective(task, GOAL)
        if rows is not None:
            e.set_point_rollout_scenes(rows)
        return e

    batch = HipBatch(4, point_runtime=True)
    try:
        sharded = eng(K=128, K_local=64, rows=rows)
        _refused(batch, [good.A, sharded], -4, "handle 1: sharded", twins)
        sim = eng(K=K, sim_only=True, noise=False, task=None)
        _refused(batch, [good.A, sim], -4, "handle 1: handle was created sim_only", twins)
        panda = HipEngine(make_config(K=200, T=20, nu=9, env_type="panda_env", u_min=[-1.2] * 9, u_max=[1.2] * 9,
                                      noise_sigma_diag=[10.0] * 7 + [0.8, 0.8], lambda_=0.05, dt=0.01))
        made.append(panda)
        panda.set_noise(np.zeros((200, 20, 9), np.float32))
        panda.set_objective("reach", [0.2, 0.2, 1.1, 0, 0, 0, 1])
        _refused(batch, [good.A, panda], -5, "handle 1: panda_env handle in a batch of point_env handles", twins)
        other.A.set_point_scene_instance(0)
        _refused(batch, [good.A, other.A], -4, r"handle 1: .*forced off \(m3_set_point_scene_instance 0\).*arena per sample", twins)
        other.A.set_point_scene_instance(-1)
        _refused(batch, [good.A, good.A], -1, "handle 1: handle listed twice", twins)
        # and the same handles run afterwards
        batch.command([good.A, other.A])
        good.B.command(); other.B.command()
        torch.cuda.synchronize()
        assert good.assert_same("after the refusals") == 1 and other.assert_same("after the refusals") == 1
        assert batch.launches()[0] == 1
    finally:
        batch.close()
        for e in made:
            e.close()
