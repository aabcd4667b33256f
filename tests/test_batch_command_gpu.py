"""m3_batch_command (include/m3p2i_hip.h): one rollout launch and one update launch per group of point_env handles that run
the same kernel instance.  Every handle A_i is commanded through the batch and its twin B_i (same config, noise, world,
objective and settings) through its own m3_command; after every call every per-handle output and every field of m3_info
must be the same BITS.  Refused calls must leave every handle as it was."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, make_config  # noqa: E402

PK = dict(u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3])
BUFS = [L.BUF_ACTION_OUT, L.BUF_MEAN, L.BUF_MEAN_1, L.BUF_MEAN_2, L.BUF_BEST, L.BUF_BEST_1, L.BUF_BEST_2, L.BUF_WEIGHTS,
        L.BUF_WEIGHTS_1, L.BUF_WEIGHTS_2, L.BUF_TRAJ_COST, L.BUF_COST_HORIZON, L.BUF_STATES, L.BUF_ACTIONS, L.BUF_TOP_IDX,
        L.BUF_TOP_TRAJS, L.BUF_PENDING_FORCE, L.BUF_COV]
BOX_ACTOR, DYN_ACTOR, N_ACTORS = 6, 5, 11


def _noise(K, T, seed):
    g = torch.Generator().manual_seed(seed)
    knots = torch.randn(K, 2, max(T // 4, 2), generator=g)
    return torch.nn.functional.interpolate(knots, size=T, mode="linear", align_corners=True).permute(0, 2, 1).contiguous().numpy()


def _world(i, call):
    """raw layout: robot x y vx vy | box x y c s vx vy w | dyn-obs x y c s vx vy w -- moved a little every call"""
    r = np.random.default_rng([i, call])
    w = np.zeros(18, np.float32)
    w[0:2] = (0.2 * math.sin(i) + 0.05 * call, 0.5 + 0.1 * math.cos(i) - 0.04 * call)
    w[2:4] = r.uniform(-0.3, 0.3, 2)
    w[4:7] = (0.1 * math.cos(3 * i), 2.0 - 0.03 * call, 1.0)
    w[11:14] = (-2.0 + 0.1 * call, 2.0 - 0.05 * i, 1.0)
    w[15] = -0.2
    return w


class Twin:
    """Two handles made the same way; A is commanded through the batch, B by m3_command."""

    def __init__(self, i, K, T, task, goal, avoid=False, wave_order=True, relabel=False, bind=False, action_out=False,
                 spins=None, **cfg_kw):
        kw = dict(PK)
        kw.update(cfg_kw)
        self.i, self.bind = i, bind
        self.engs = []
        if bind:
            self.dof = torch.zeros(1, 4, device="cuda:0")
            self.root = torch.zeros(1, N_ACTORS, 13, device="cuda:0")
            self.root[..., 6] = 1.0
        for _ in range(2):
            e = HipEngine(make_config(K=K, T=T, nu=2, **kw))
            if not (e.cfg.sampling_random or e.cfg.mode_simple):
                e.set_noise(_noise(K, T, 100 + i))
            e.set_objective(task, goal)
            if avoid:
                e.set_avoid_dyn_obs(True)
            if not wave_order:
                e.set_wave_order(False)
            if relabel:
                e.relabel_samples()
            if spins is not None:
                e.set_ladder_spins(spins)
            if bind:
                e.bind_sim_point(self.dof, self.root, BOX_ACTOR, DYN_ACTOR)
            if action_out:
                rows = e.cfg.u_per_command if e.cfg.mode_simple else e.cfg.T
                e.set_action_out(torch.zeros(rows, 2, device="cuda:0"))
            self.engs.append(e)
        self.A, self.B = self.engs

    def set_world(self, call):
        w = _world(self.i, call)
        if self.bind:
            self.dof[0] = torch.tensor([w[0], w[2], w[1], w[3]])
            for actor, o in ((BOX_ACTOR, 4), (DYN_ACTOR, 11)):
                c, s = float(w[o + 2]), float(w[o + 3])
                half = math.atan2(s, c) / 2
                self.root[0, actor, 0:2] = torch.tensor(w[o:o + 2])
                self.root[0, actor, 3:7] = torch.tensor([0.0, 0.0, math.sin(half), math.cos(half)])
                self.root[0, actor, 7:9] = torch.tensor(w[o + 4:o + 6])
                self.root[0, actor, 12] = float(w[o + 6])
        else:
            for e in self.engs:
                e.set_world_point_raw(w)

    def out(self, e, which):
        if which == L.BUF_ACTION_OUT and e._action_out is not None:
            return e._action_out
        try:
            return e.buffer(which)
        except L.M3Error:
            return None

    def assert_same(self, label):
        for which in BUFS:
            a, b = self.out(self.A, which), self.out(self.B, which)
            assert (a is None) == (b is None), (label, self.i, which)
            if a is not None:
                assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), f"{label}: handle {self.i}: buffer {which} differs"
        ia, ib = self.A.info(), self.B.info()
        assert bytes(ia) == bytes(ib), f"{label}: handle {self.i}: m3_info differs"
        return ia.calls

    def close(self):
        for e in self.engs:
            e.close()


def _run(twins, calls=6, order=None):
    """order(call) -> the indices of the twins commanded in that call (default: all, in order)"""
    batch = HipBatch(len(twins))
    expect = [0] * len(twins)
    try:
        for c in range(calls):
            for t in twins:
                t.set_world(c)
            sel = list(range(len(twins))) if order is None else order(c)
            batch.command([twins[i].A for i in sel])
            for i in sel:
                twins[i].B.command()
                expect[i] += 1
            torch.cuda.synchronize()
            for i, t in enumerate(twins):
                assert t.assert_same(f"call {c}") == expect[i]
        return batch.launches()
    finally:
        batch.close()


@pytest.fixture
def twins():
    made = []
    yield made
    for t in made:
        t.close()


def test_mixed_tasks_and_sizes(twins):
    specs = [dict(K=200, T=15, task="navigation", goal=(2.0, -2.0)),
             dict(K=2000, T=30, task="push", goal=(-1.0, -1.0)),
             dict(K=2000, T=15, task="pull", goal=(0.0, 0.0)),
             dict(K=4000, T=30, task="push_pull", goal=(-3.75, -3.75), multi_modal=True),
             dict(K=2000, T=30, task="push_pull", goal=(-3.75, -3.75), multi_modal=True),
             dict(K=4000, T=30, task="push", goal=(-1.0, -1.0)),
             dict(K=2000, T=30, task="push", goal=(1.0, -1.0), action_out=True),
             dict(K=200, T=15, task="push", goal=(-1.0, 1.0))]
    twins += [Twin(i, **s) for i, s in enumerate(specs)]
    n = len(twins)
    # in order, reversed, alternating halves, everything again
    order = {0: list(range(n)), 1: list(range(n))[::-1], 2: list(range(0, n, 2)), 3: list(range(1, n, 2))[::-1],
             4: list(range(n)), 5: [3, 0, 7, 5]}
    # the last call: rollouts push_pull 4000 / navigation 200 / push 200 / push 4000; updates multi-modal / K <= 2048 with
    # T = 15 (navigation + push) / single mode with 16 register rows
    assert _run(twins, calls=6, order=order.get) == (4, 3)


def test_general_instances_and_bound_views(twins):
    specs = [dict(K=2000, T=30, task="push", goal=(-1.0, -1.0), sampling_random=True),
             dict(K=2000, T=30, task="push", goal=(-1.0, -1.0), mode_simple=True, sampling_random=True, u_per_command=10),
             dict(K=2000, T=30, task="push", goal=(-1.0, -1.0), update_cov=True),
             dict(K=2000, T=30, task="pull", goal=(0.0, 0.0), noise_sigma=[[3.0, 0.5], [0.5, 3.0]], sampling_random=True),
             dict(K=2000, T=30, task="push", goal=(-1.0, -1.0), avoid=True),
             dict(K=2000, T=30, task="push", goal=(-1.0, -1.0), bind=True),
             dict(K=2000, T=30, task="navigation", goal=(2.0, -2.0), bind=True),
             dict(K=4000, T=30, task="push_pull", goal=(-3.75, -3.75), multi_modal=True, bind=True),
             dict(K=2000, T=30, task="push", goal=(-1.0, -1.0))]
    twins += [Twin(i, **s) for i, s in enumerate(specs)]
    _run(twins, calls=6)


def test_wave_order_relabel_and_lanes(twins):
    specs = [dict(K=2000, T=30, task="push", goal=(-1.0, -1.0), wave_order=False),
             dict(K=2000, T=30, task="push", goal=(-1.0, -1.0), relabel=True),
             dict(K=4000, T=30, task="push_pull", goal=(-3.75, -3.75), multi_modal=True, relabel=True),
             dict(K=4000, T=30, task="push_pull", goal=(-3.75, -3.75), multi_modal=True, wave_order=False),
             dict(K=2000, T=30, task="push", goal=(-1.0, -1.0))]
    twins += [Twin(i, **s) for i, s in enumerate(specs)]
    for t in twins[:2]:
        for e in t.engs:
            e.set_rollout_lanes(32)
    _run(twins, calls=6)


def test_batch_of_one(twins):
    twins.append(Twin(0, K=2000, T=30, task="push", goal=(-1.0, -1.0)))
    assert _run(twins, calls=6) == (1, 1)


@pytest.mark.parametrize("spins", [None, 0])
def test_multi_modal_group_larger_than_one_residency_chunk(twins, spins):
    n = 40
    twins += [Twin(i, K=4000, T=30, task="push_pull", goal=(-3.75, -3.75), multi_modal=True, spins=spins) for i in range(n)]
    rl, ul = _run(twins, calls=3)
    # kb_update_small<true, 8, 512>: one resident workgroup per CU (update_small.hip; tests/test_batch_cpu.py checks the
    # number against the code object), 31 workgroups per handle -> 8 handles per launch
    assert rl == 1 and ul == math.ceil(n / (256 // 31))


@pytest.mark.parametrize("counts", [(1, 1, 1), (3, 1, 2)])
def test_all_three_variants_in_one_call(twins, counts):
    """plain / tuned cost weights in the default arena / custom arena in ONE m3_batch_command: the table then holds all three
    kinds of entry, with both alignment gaps between its sections (584-byte plain and 616-byte weighted entries: an odd number
    of either leaves the next section 8 bytes further).  K = 128: two workgroups per handle.  Every handle's states, actions,
    costs and plan (all of BUFS, m3_info) are the bits of its own twin's m3_command; one rollout launch per variant."""
    from tests.point_scene_fixture import CUSTOM
    kinds = [k for k, c in enumerate(counts) for _ in range(c)]
    kinds = kinds[::-1][1:] + kinds[::-1][:1]   # (not in the order of the table's sections)
    for i, kind in enumerate(kinds):
        t = Twin(i, K=128, T=5, task="push", goal=(-1.0, -1.0), filter_u=False)   # (T = 5 is below the filter's window)
        twins.append(t)
        for e in t.engs:
            if kind == 1:
                e.set_point_cost_weights(dict(push_align=2.5, push_dist=1.5))
            if kind == 2:
                e.set_point_scene(CUSTOM)
    assert _run(twins, calls=2)[0] == 3


def _calls_and_mean(e):
    return e.info().calls, e.buffer(L.BUF_MEAN).cpu().numpy().tobytes()


def test_refusals_leave_every_handle_untouched():
    lib = L.load()
    made = []

    def eng(K=2000, T=30, task="push", noise=True, **kw):
        e = HipEngine(make_config(K=K, T=T, nu=kw.pop("nu", 2), **{**PK, **kw}))
        if noise:
            e.set_noise(_noise(e.cfg.K_local, T, 7) if e.cfg.nu == 2 else
                        np.zeros((e.cfg.K_local, T, e.cfg.nu), np.float32))
        if task:
            e.set_objective(task, (-1.0, -1.0) if e.cfg.nu == 2 else [0.2, 0.2, 1.1, 0, 0, 0, 1])
        if e.cfg.nu == 2:
            e.set_world_point_raw(_world(0, 0))
        made.append(e)
        return e

    good = eng()
    good.command()           # (a warm start that a refused call must not touch)
    batch = HipBatch(4)
    before = _calls_and_mean(good)

    def refused(engines, status, text, n=None, handles=None):
        arr = (C.c_void_p * max(len(engines), 1))(*[e._h.value if e is not None else None for e in engines])
        rc = lib.m3_batch_command(batch._b, arr if handles is None else handles, len(engines) if n is None else n, None)
        msg = lib.m3_batch_last_error(batch._b).decode()
        assert rc == status, (rc, msg)
        assert text in msg, msg
        assert _calls_and_mean(good) == before

    try:
        assert lib.m3_batch_command(None, None, 1, None) < 0
        refused([good], L_ERR["BAD_ARG"], "handle list", handles=C.POINTER(C.c_void_p)())
        refused([good], L_ERR["BAD_ARG"], "max_handles", n=0)
        refused([good] * 5, L_ERR["BAD_ARG"], "max_handles")
        refused([good, None], L_ERR["BAD_ARG"], "handle 1")
        refused([good, good], L_ERR["BAD_ARG"], "handle 1: handle listed twice")
        refused([good, eng(K=2000, K_local=1000)], L_ERR["STATE"], "handle 1: sharded")
        refused([good, eng(K=2000, sim_only=True, noise=False, task=None)], L_ERR["STATE"], "handle 1")
        other = eng()
        stream = torch.cuda.Stream()
        other.use_torch_stream(stream)
        refused([good, other], L_ERR["STATE"], "handle 1: its stream differs")
        refused([good, eng(noise=False)], L_ERR["STATE"], "handle 1: m3_rollout: no noise set")
        # (push_pull without multi_modal, m3_rollout's other refusal, is already refused by m3_set_objective)
        panda = eng(K=200, T=20, nu=9, env_type="panda_env", u_min=[-1.2] * 9, u_max=[1.2] * 9,
                    noise_sigma_diag=[10.0] * 7 + [0.8, 0.8], lambda_=0.05, dt=0.01, task="reach")
        refused([good, panda], L_ERR["UNSUPPORTED"], "handle 1: panda_env")
        refused([good, eng(K=20000)], L_ERR["UNSUPPORTED"], "handle 1: its command does not take the one-launch update")
        refused([good, eng(K=10000, multi_modal=True, task="push_pull")], L_ERR["UNSUPPORTED"], "handle 1")
        if torch.cuda.device_count() > 1:
            far = HipEngine(make_config(K=2000, T=30, nu=2, device=1, **PK))
            made.append(far)
            refused([good, far], L_ERR["BAD_ARG"], "handle 1: handle on another device")
            torch.cuda.set_device(0)
        # ... and the same batch still works afterwards
        batch.command([good])
        assert good.info().calls == before[0] + 1
    finally:
        batch.close()
        for e in made:
            e.close()


L_ERR = {"BAD_ARG": -1, "HIP": -2, "SHAPE": -3, "STATE": -4, "UNSUPPORTED": -5}
