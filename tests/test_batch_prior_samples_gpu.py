"""m3_batch_command for point_env handles with prior samples (m3_batch_create_sections with M3_BATCH_SECTION_POINT_PRIORS;
DESIGN.md section 7k).  Handle A_i goes through the batch, its twin B_i through its own m3_command; after every call every
buffer of tests/test_batch_command_gpu.BUFS and every field of m3_info must be the same BYTES.  Handle i carries its own table
(sequences seeded by i, at indices shifted by i), and after every call the stored actions of its prior samples are its own
clamped rows and not its neighbour's -- a handle that read a neighbour's table or slot map would show.  Refused calls leave every
handle as it was.  K = 64 and K = 100 (a half-empty wavefront), T = 12."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, make_config  # noqa: E402
from tests import point_scene_fixture as X  # noqa: E402
from tests import prior_samples_fixture as P  # noqa: E402
from tests import rollout_scenes_fixture as R  # noqa: E402
from tests.test_batch_command_gpu import PK, Twin, _noise  # noqa: E402
from tests.test_point_scene_gpu import TASKS, W_TUNED  # noqa: E402

F = np.float32
T = 12
GOAL = [-1.0, -1.0]
PRIORS = L.BATCH_SECTION_POINT_PRIORS


@pytest.fixture
def twins():
    made = []
    yield made
    for t in made:
        t.close()


def _idx(i, K, mm):
    """four samples of handle i, shifted by i; multi-modal: two in each half, never 0, K / 2 or K - 1"""
    if mm:
        return [1 + i % 5, 7 + i % 5, K // 2 + 1 + i % 5, K // 2 + 7 + i % 5]
    return [1 + i % 10, 12 + (2 * i) % 10, 24 + i % 5, K - 2 - (i % 3) * 7]      # (disjoint ranges: 1..10, 12..21, 24..28, >= 48)


def _set(t, how, seed=None, idx=None):
    """the priors of twin t on both of its handles: "host" (m3_set_prior_samples), "device" (m3_set_prior_samples_device), "go_to" /
    "push_behind" (a controller), None (cleared).  Remembers what the rows must be (t.seqs: None for a controller)."""
    K, mm = t.A.cfg.K_global, bool(t.A.cfg.multi_modal)
    t.idx = _idx(t.i, K, mm) if idx is None else idx
    t.how, t.seqs = how, None
    for e in t.engs:
        if how is None:
            e.set_prior_samples(None)
        elif how in ("host", "device"):
            t.seqs = P.prior_seqs(len(t.idx), T, seed=(100 + t.i) if seed is None else seed)
            e.set_prior_samples(torch.as_tensor(t.seqs, device=e.device) if how == "device" else t.seqs, t.idx)
        else:
            e.set_prior_controller(how, len(t.idx), t.idx)


def _twin(made, i, K, how="host", task="push", mm=False, shift=None, **kw):
    kw.setdefault("filter_u", False)
    t = Twin(i, K=K, T=T, task=task, goal=GOAL, multi_modal=mm, **kw)
    made.append(t)
    if shift is not None:
        for e in t.engs:
            e.set_point_rollout_scenes(R.cycle_rows(K, shift))
    _set(t, how)
    return t


def _assert_own_rows(twins, label):
    """the actions the rollout stored for each handle's prior samples are ITS rows, clamped -- and no other handle's"""
    for n, t in enumerate(twins):
        if t.how is None:
            continue
        got = t.A.actions.cpu().numpy()[t.idx]
        if t.seqs is None:      # a controller: the handle's own table, as the kernel ahead of the rollout left it
            want = t.A.prior_table().cpu().numpy()
            assert np.abs(want).max() > 0, label
        else:
            want = t.seqs
        lim = np.clip(want, -3, 3).astype(F)
        assert got.view(np.uint32).tobytes() == lim.view(np.uint32).tobytes(), f"{label}: handle {n}: not its own priors"
        for m, o in enumerate(twins):
            if o is not t and o.seqs is not None and o.seqs.shape == want.shape:
                assert np.clip(o.seqs, -3, 3).astype(F).tobytes() != got.tobytes(), (label, n, m)


def _run(twins, calls=6, before=None, max_handles=None, **batch_kw):
    """before(call): what changes ahead of that call.  Returns the launches of every call."""
    batch = HipBatch(max_handles or len(twins), point_priors=True, **batch_kw)
    launches = []
    live = None
    try:
        assert batch.flags() & PRIORS
        for c in range(calls):
            if before:
                before(c)
            for t in twins:
                t.set_world(c)
            if c == 1 and before is None:
                live = L.load().m3_owned_blocks_live()
            batch.command([t.A for t in twins])
            for t in twins:
                t.B.command()
            torch.cuda.synchronize()
            for t in twins:
                assert t.assert_same(f"call {c}") == c + 1
                assert t.how is None or t.A.prior_samples_used() == t.B.prior_samples_used() == 1
            _assert_own_rows(twins, f"call {c}")
            launches.append(batch.launches())
        if live is not None:
            assert L.load().m3_owned_blocks_live() == live      # nothing allocated on the command path
        return launches
    finally:
        batch.close()


# ------------------------------------------------------------------ 1. twin equality
def test_a_two_sizes_in_one_call_give_two_priors_groups(twins):
    for i in range(3):
        _twin(twins, i, 64)
    for i in range(3, 5):
        _twin(twins, i, 100)
    launches = _run(twins)
    assert all(roll == 2 for roll, _ in launches), launches


def test_b_host_device_controller_and_rows_share_one_group(twins):
    _twin(twins, 0, 100, "host")
    _twin(twins, 1, 100, "device")
    _twin(twins, 2, 100, "push_behind")
    _twin(twins, 3, 100, "host", shift=1)            # priors plus an arena per sample
    _twin(twins, 4, 100, "go_to", shift=2, bind=True)
    launches = _run(twins)
    assert all(roll == 1 for roll, _ in launches), launches
    assert twins[3].A.point_rollout_scenes_set() and twins[2].A.prior_controller()["kind"] == 2


def test_c_the_four_tasks_tuned_weights_update_cov_and_another_dt_share_one_launch(twins):
    for i, (task, mm) in enumerate(TASKS):
        _twin(twins, i, 100, "host" if i % 2 else "go_to", task=task, mm=mm)
    tuned = _twin(twins, 4, 100, "push_behind")
    for e in tuned.engs:
        e.set_point_cost_weights(W_TUNED)
    _twin(twins, 5, 100, "host", update_cov=True)
    _twin(twins, 6, 100, "push_behind", task="push_pull", mm=True, dt=0.04, substeps=3)   # (the controller's dt is the handle's)
    launches = _run(twins)
    assert all(roll == 1 for roll, _ in launches), launches


def test_d_one_call_with_all_five_sections(twins):
    _twin(twins, 0, 64, None)
    weighted = _twin(twins, 1, 64, None)
    for e in weighted.engs:
        e.set_point_cost_weights(W_TUNED)
    scene = _twin(twins, 2, 64, None)
    for e in scene.engs:
        e.set_point_scene(X.CUSTOM)
    _twin(twins, 3, 64, None, shift=1)
    _twin(twins, 4, 64, "host")
    _twin(twins, 5, 64, "push_behind", shift=2)
    # (call order is not section order: the handles with priors first)
    twins[:] = [twins[4], twins[3], twins[0], twins[5], twins[2], twins[1]]
    launches = _run(twins, point_runtime=True)
    assert all(roll == 5 for roll, _ in launches), launches


def test_e_priors_replaced_and_cleared_between_calls(twins):
    _twin(twins, 0, 64, "host")
    _twin(twins, 1, 64, "go_to")

    def before(c):
        if c == 2:        # other values and other indices; the controller replaced by a caller's table
            _set(twins[0], "device", seed=300, idx=[5, 6, 50])
            _set(twins[1], "host", seed=301)
        if c == 3:        # ... and a caller's table by a controller
            _set(twins[1], "push_behind")
        if c == 4:        # handle 0 without priors: another section of the table
            _set(twins[0], None)

    launches = _run(twins, before=before, max_handles=5)
    assert [roll for roll, _ in launches] == [1, 1, 1, 1, 2, 2]
    assert twins[0].A.prior_samples_set() == 0 and twins[0].A.prior_samples_used() == 1    # (the record of its last prior build)
    assert twins[1].A.prior_samples_set() == 4


def test_f_wave_order_relabelled_noise_and_bound_views(twins):
    _twin(twins, 0, 256, "host", wave_order=False)
    _twin(twins, 1, 256, "push_behind", relabel=True)
    _twin(twins, 2, 256, "go_to", bind=True, action_out=True)
    _twin(twins, 3, 256, "device")           # (the wavefront order is formed from K_local = 128 on)
    launches = _run(twins)
    assert all(roll == 1 for roll, _ in launches), launches
    assert twins[0].A.wave_order() is None


# ------------------------------------------------------------------ 2. the occ builds through the group rule
@pytest.mark.parametrize("n,K,build", [(17, 64, "occ2"), (33, 128, "occ3")])
def test_the_group_wavefront_count_picks_the_occ_builds(twins, n, K, build):
    """one sample per wavefront: 17 * 64 = 1088 wavefronts (> 1024: occ2), 33 * 128 = 4224 (> 4096: occ3) -- no handle reaches the
    threshold on its own, so its twin's m3_command runs the lone build: same bits"""
    for i in range(n):
        t = _twin(twins, i, K, ("host", "push_behind", "device")[i % 3], shift=i if i % 4 == 0 else None)
        for e in t.engs:
            e.set_rollout_lanes(1)
    launches = _run(twins, calls=3)
    assert all(roll == 1 for roll, _ in launches), (build, launches)


# ------------------------------------------------------------------ 3. refusals
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
    _twin(twins, 0, 64, None)
    _twin(twins, 1, 64, "push_behind")
    _twin(twins, 2, 64, None)
    for t in twins:
        t.set_world(0)
    for batch in (HipBatch(3), HipBatch(3, panda_runtime=True), HipBatch(3, point_runtime=True)):
        try:
            assert not batch.flags() & PRIORS
            _refused(batch, [t.A for t in twins], -5,
                     r"handle 1: it has prior samples \(m3_set_prior_samples\), which only m3_rollout / m3_command run", twins)
        finally:
            batch.close()


def test_section_bits():
    lib = L.load()
    torch.zeros(1, device="cuda:0")
    for bits in (64, 16, 32 | 4, 32 | 8):
        out = C.c_void_p(1)
        assert lib.m3_batch_create_sections(0, 4, bits, C.byref(out)) == -1 and out.value is None
        assert b"unknown section bits" in lib.m3_batch_last_error(None)
    for bits in (32, 33, 34, 35):
        out = C.c_void_p()
        assert lib.m3_batch_create_sections(0, 4, bits, C.byref(out)) == 0
        assert lib.m3_batch_flags(out) == bits
        lib.m3_batch_destroy(out)
    out = C.c_void_p(1)
    assert lib.m3_batch_create_ex(0, 4, 32, C.byref(out)) == -1 and out.value is None


def test_the_new_batch_keeps_the_other_refusals(twins):
    K = 64
    good = _twin(twins, 0, K, "host")
    other = _twin(twins, 1, K, "push_behind")
    for t in twins:
        t.set_world(0)
    made = []

    def eng(task="push", noise=True, **kw):
        e = HipEngine(make_config(T=T, nu=kw.pop("nu", 2), filter_u=False, **{**PK, **kw}))
        made.append(e)
        if noise:
            e.set_noise(_noise(e.cfg.K_local, T, 7))
        if task:
            e.set_objective(task, GOAL)
        return e

    batch = HipBatch(4, point_priors=True)
    try:
        sharded = eng(K=128, K_local=64)
        _refused(batch, [good.A, sharded], -4, "handle 1: sharded", twins)
        sim = eng(K=K, sim_only=True, noise=False, task=None)
        _refused(batch, [good.A, sim], -4, "handle 1: handle was created sim_only", twins)
        rows_only = eng(K=K)
        rows_only.set_point_rollout_scenes(R.cycle_rows(K))       # an arena per sample without priors needs ITS section
        _refused(batch, [good.A, rows_only], -5, r"handle 1: it has an arena per sample \(m3_set_point_rollout_scenes\)", twins)
        panda = HipEngine(make_config(K=200, T=20, nu=9, env_type="panda_env", u_min=[-1.2] * 9, u_max=[1.2] * 9,
                                      noise_sigma_diag=[10.0] * 7 + [0.8, 0.8], lambda_=0.05, dt=0.01))
        made.append(panda)
        panda.set_noise(np.zeros((200, 20, 9), np.float32))
        panda.set_objective("reach", [0.2, 0.2, 1.1, 0, 0, 0, 1])
        _refused(batch, [good.A, panda], -5, "handle 1: panda_env handle in a batch of point_env handles", twins)
        other.A.set_point_scene_instance(0)
        _refused(batch, [good.A, other.A], -4, r"handle 1: .*forced off \(m3_set_point_scene_instance 0\).*prior samples", twins)
        other.A.set_point_scene_instance(-1)
        other.A.set_objective("navigation", GOAL)       # PUSH_BEHIND without a box to go behind: the rollout's own refusal
        _refused(batch, [good.A, other.A], -4, "handle 1: .*PUSH_BEHIND.*navigation", twins)
        other.A.set_objective("push", GOAL)
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
