"""The wavefront order of the point_env samples (sampler.hip: k_order_keys, the radix sort, k_fix_specials, k_gather_noise,
k_gather_rows; m3_api.hip: order_block, refresh_wave_order) against the float64 reference tests/wave_order_ref.py.

Lane placement cannot change a sample's numbers, so no test of the results can see a wrong order; these see the order itself:
as the indirection the rollout went by (m3_wave_order), and after m3_relabel_samples as the permutation of the uploaded noise
rows (recovered by matching row bytes).  The comparison (wave_order_ref.compare): a permutation, the special samples at their own
index, every sample in its mode's half, and position by position a key within tol = 2 (3T + 8) 2^-24 M of the reference's --
two near-tied samples may trade places, nothing else may move.  Inputs: tests/wave_order_cases.py (the smallest shapes at which
the code can go wrong; the order needs K_local >= 128).
"""
import numpy as np
import pytest

from tests import wave_order_cases as W
from tests import wave_order_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PK = dict(nu=2, u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=list(W.SIGMA))
BOX_ACTOR, DYN_ACTOR = 6, 5


def _engine(c, k_offset=0, K_local=None, shard_mix=0, world=True):
    from m3p2i_aip_amd.engine import HipEngine, make_config
    e = HipEngine(make_config(K=c["K"], T=c["T"], multi_modal=c["mm"], K_local=K_local, k_offset=k_offset,
                              shard_mix=shard_mix, **PK))
    e.set_objective(*(("push_pull", (-3.75, -3.75)) if c["mm"] else ("push", (-1.0, -1.0))))
    if world:
        e.set_world_point_raw(W.world_raw(c))
    return e


def _perm_of_rows(block, uploaded):
    """p[i] = index of the uploaded row [T, nu] that row i of the device block [T, Kl, nu] holds"""
    where = {r.tobytes(): i for i, r in enumerate(np.ascontiguousarray(uploaded))}
    assert len(where) == len(uploaded), "the uploaded rows are not pairwise distinct"
    rows = np.ascontiguousarray(block.permute(1, 0, 2).contiguous().cpu().numpy())
    return np.array([where[r.tobytes()] for r in rows])      # (KeyError: a row that was never uploaded)


def _check(tag, p, c, k_offset, K_local, relabel):
    keys, bound = W.block_keys(c, k_offset, K_local)
    worst = R.compare(p, keys, c["K"], k_offset, K_local, c["mm"], relabel, bound)
    print(f"{tag}: largest position-wise key difference {worst:.3g}, bound {bound:.3g}")


def _indirection_then_relabel(name, c, e):
    """the order the rollout went by, then the same handle relabelled: both against the reference"""
    from m3p2i_aip_amd import _lib as L
    K = c["K"]
    assert e.wave_order() is None                       # no rollout yet
    e.set_noise(c["delta"])
    e.command()
    p = e.wave_order()
    assert p is not None and p.dtype == torch.int32 and tuple(p.shape) == (K,)
    _check(f"{name} indirection", p.cpu().numpy(), c, 0, K, relabel=False)
    # (the indirection leaves the noise buffer as uploaded)
    assert np.array_equal(_perm_of_rows(e.buffer(L.BUF_NOISE), c["delta"]), np.arange(K))
    e.relabel_samples()
    e.command()
    assert e.wave_order() is None                       # relabelled: index order is wavefront order
    _check(f"{name} relabelled", _perm_of_rows(e.buffer(L.BUF_NOISE), c["delta"]), c, 0, K, relabel=True)


@pytest.mark.parametrize("name", ["single_K128", "single_K200"])
def test_single_mode_order_equals_the_reference(name):
    c = W.case(name)
    e = _engine(c)
    _indirection_then_relabel(name, c, e)
    e.close()


@pytest.mark.parametrize("name", ["multi_K256", "multi_K512_T30"])
def test_multi_modal_order_equals_the_reference_in_both_modes(name):
    """With the mode carried as an offset of 1e9 in the f32 key (one ulp: 64) the second mode's samples stayed in index order
    inside buckets of 64 key units: measured with that key, 122 of 256 slots off by up to 57.9 (K = 256) and 233 of 512 by up
    to 62.9 (K = 512, T = 30), against bounds of 1.5e-3 and 1.7e-2."""
    c = W.case(name)
    e = _engine(c)
    _indirection_then_relabel(name, c, e)
    e.close()


@pytest.mark.parametrize("name", ["oblique_single_K200", "oblique_multi_K256"])
def test_order_follows_an_oblique_axis(name):
    """box, dyn-obs and obstacle not in a row (tests/wave_order_cases.py states the positions): the axis is neither x nor y"""
    c = W.case(name)
    e = _engine(c)
    _indirection_then_relabel(name, c, e)
    e.close()


@pytest.mark.parametrize("name", ["bound_single_K200", "bound_multi_K256"])
def test_order_follows_the_bound_simulators_root_tensor(name):
    """bind_sim_point: box and dyn-obs are read from the device root tensor; the handle's own world keeps the row scene, whose
    axis (th = 0) gives another order"""
    c = W.case(name)
    e = _engine(c, world=False)
    e.set_world_point_raw(W.world_raw(dict(W.SCENES["row"])))
    dof = torch.tensor([[0.0, 0.0, 1.5, 0.0]], device=e.device)
    root = torch.zeros(1, 11, 13, device=e.device)
    root[0, :, 6] = 1.0
    root[0, BOX_ACTOR, 0:2] = torch.tensor(c["box"], device=e.device)
    root[0, DYN_ACTOR, 0:2] = torch.tensor(c["dyn"], device=e.device)
    e.bind_sim_point(dof, root, BOX_ACTOR, DYN_ACTOR)
    e.set_noise(c["delta"])
    e.command()
    p = e.wave_order()
    assert p is not None
    _check(f"{name} indirection", p.cpu().numpy(), c, 0, c["K"], relabel=False)
    row_keys, _ = R.keys64(c["delta"], W.SIGMA, W.SCENES["row"]["box"], W.SCENES["row"]["dyn"], W.OBSTACLE)
    assert not np.array_equal(p.cpu().numpy(), R.expected_perm(row_keys, c["K"], 0, c["K"], c["mm"], False))
    e.close()


@pytest.mark.parametrize("k_offset", [0, 256])
def test_plain_shards_order_their_own_block(k_offset):
    """K_global = 512 in two shards of 256, multi-modal: the first block lies wholly in the first mode, the second wholly in the
    second (half_local = 0).  Each shard's order equals the reference for its block; special samples outside the block are
    skipped (0 in the first; 256 and 511, local 0 and 255, in the second)."""
    from m3p2i_aip_amd import _lib as L
    c = W.case("shards_K512")
    rows = c["delta"][k_offset:k_offset + 256]
    e = _engine(c, k_offset, 256)
    e.set_noise(rows)
    e.rollout()
    p = e.wave_order()
    assert p is not None
    _check(f"shard at {k_offset} indirection", p.cpu().numpy(), c, k_offset, 256, relabel=False)
    e.relabel_samples()
    e.rollout()
    assert e.wave_order() is None
    _check(f"shard at {k_offset} relabelled", _perm_of_rows(e.buffer(L.BUF_NOISE), rows), c, k_offset, 256, relabel=True)
    e.close()


@pytest.mark.parametrize("level", [1, 2, 3])
def test_one_collective_shards_relabel_every_block_like_its_owner(level):
    """shard_mix with the noise of all K_global samples on both ranks (two ranks on one GPU): after relabelling both hold the
    same M3_BUF_NOISE_ALL bit for bit, and every block in it is in the reference's order for its owner's offset."""
    from m3p2i_aip_amd import _lib as L
    c = W.case("shards_K512")
    shards = [_engine(c, r * 256, 256, shard_mix=level) for r in range(2)]
    for e in shards:
        assert e.needs_global_noise
        e.set_noise(c["delta"])
        e.relabel_samples()
        e.rollout()
    torch.cuda.synchronize()
    tables = [e.buffer(L.BUF_NOISE_ALL) for e in shards]
    assert torch.equal(tables[0], tables[1])
    for rank, e in enumerate(shards):
        assert e.wave_order() is None
        assert torch.equal(e.buffer(L.BUF_NOISE), tables[rank][rank])
        for r in range(2):
            p = _perm_of_rows(tables[rank][r], c["delta"][r * 256:(r + 1) * 256])
            _check(f"level {level} rank {rank} block {r}", p, c, r * 256, 256, relabel=True)
    for e in shards:
        e.close()


def test_pending_forces_follow_their_samples_through_a_mid_stream_relabel(oracle):
    """k_gather_rows.  A pull task with the robot next to the box leaves pending suction forces that differ from sample to sample
    (checked on the CPU oracle too).  Two twins run one command by index; one is then relabelled, both run a second command:
    sample i of the relabelled twin must be sample p[i] of the other, bit for bit, in cost and in every row of the forces."""
    from m3p2i_aip_amd import _lib as L
    c = dict(W.case("multi_K256"), mm=False)
    K, T = c["K"], c["T"]
    robot = (0.0, 1.5)
    twins = []
    for _ in range(2):
        e = _engine(c, world=False)
        e.set_objective("pull", (0.0, 0.0))
        e.set_world_point_raw(W.world_raw(c, robot))
        e.set_wave_order(False)
        e.set_noise(c["delta"])
        e.command()
        assert e.wave_order() is None
        twins.append(e)
    a, b = twins
    pend = a.buffer(L.BUF_PENDING_FORCE).clone()                       # [4, K]
    assert torch.equal(pend, b.buffer(L.BUF_PENDING_FORCE))
    assert (pend != 0).any() and len({col.tobytes() for col in pend.cpu().numpy().T}) >= 8
    w0 = oracle.init_world(1)[0]
    w0[0:2] = robot
    opl = oracle.OraclePointPlanner(oracle.make_cfg(K, T, 2, task="pull", goal=(0.0, 0.0)), c["delta"])
    opl.command(w0)
    assert (opl.pend != 0).any() and len({r.tobytes() for r in opl.pend}) >= 8
    assert np.array_equal(np.ascontiguousarray(opl.pend.T).view(np.uint32), pend.cpu().numpy().view(np.uint32))
    a.set_wave_order(True)
    a.relabel_samples()
    for e in twins:
        e.command()
    torch.cuda.synchronize()
    assert a.wave_order() is None and b.wave_order() is None
    p = _perm_of_rows(a.buffer(L.BUF_NOISE), c["delta"])
    assert not np.array_equal(p, np.arange(K))
    _check("mid-stream relabel", p, c, 0, K, relabel=True)
    pt = torch.as_tensor(p, device=a.device)
    assert not torch.equal(pend[:, pt], pend)           # (forces left in place would be other samples' forces)
    assert torch.equal(a.buffer(L.BUF_TRAJ_COST).view(torch.int32), b.buffer(L.BUF_TRAJ_COST)[pt].view(torch.int32))
    pa, pb = a.buffer(L.BUF_PENDING_FORCE), b.buffer(L.BUF_PENDING_FORCE)
    assert (pb != 0).any()
    for row in range(4):
        assert torch.equal(pa[row].view(torch.int32), pb[row][pt].view(torch.int32)), f"pending force row {row}"
    for e in twins:
        e.close()


@pytest.mark.parametrize("what", ["K127", "mode_simple", "sampling_random", "order_off"])
def test_refusals_stay_by_index(what):
    from m3p2i_aip_amd import sampling
    from m3p2i_aip_amd.engine import HipEngine, make_config
    kw = dict(K127=dict(K=127, T=12), mode_simple=dict(K=128, T=12, mode_simple=True, u_per_command=12, lambda_=0.5),
              sampling_random=dict(K=128, T=12, sampling_random=True), order_off=dict(K=128, T=12))[what]
    e = HipEngine(make_config(**kw, **PK))
    e.set_objective("navigation", (-3.0, 3.0))
    if not kw.get("sampling_random"):
        e.set_noise(sampling.halton_spline_delta(kw["K"], 12, 2, workers=1).numpy())
    if what == "order_off":
        e.set_wave_order(False)
    e.command()
    assert e.wave_order() is None
    e.close()
