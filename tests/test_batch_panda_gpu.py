"""m3_batch_command on panda_env handles (include/m3p2i_hip.h): one kb_rollout_panda launch (+ one kb_panda_reach_cost launch
when the group keeps the reach-cost record) and one update launch per group of handles whose own command would take the same
kernel form.  Every handle A_i is commanded through the batch and its twin B_i (same config, noise, world, objective and
settings) through its own m3_command; after every call every buffer, every field of m3_info, the kernel form the handle ran
(m3_panda_lanes_per_sample_used) and its busy report (m3_panda_near_share) must be the same.  Refused calls must leave every
handle as it was."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, make_config  # noqa: E402
from tests.panda_worlds import grasp_world  # noqa: E402

PK = dict(u_min=[-2.0] * 7 + [-1.5] * 2, u_max=[2.0] * 7 + [1.5] * 2, noise_sigma_diag=[10.0] * 7 + [0.8] * 2,
          lambda_=0.05, pre_height_diff=0.05, dt=0.01)
BUFS = [L.BUF_ACTION_OUT, L.BUF_MEAN, L.BUF_MEAN_1, L.BUF_MEAN_2, L.BUF_BEST, L.BUF_BEST_1, L.BUF_BEST_2, L.BUF_WEIGHTS,
        L.BUF_WEIGHTS_1, L.BUF_WEIGHTS_2, L.BUF_TRAJ_COST, L.BUF_COST_HORIZON, L.BUF_STATES, L.BUF_ACTIONS, L.BUF_TOP_IDX,
        L.BUF_TOP_TRAJS, L.BUF_PENDING_FORCE, L.BUF_COV]
GOALS = {"reach": [0.2, 0.2, 1.115, 0, 0, 0, 1], "pick": [0.5, 0.2, 0.7, 0, 0, 0, 1], "place": [0.5, 0.2, 0.7, 0, 0, 0, 1]}
CUBEA, CUBEB, OBS, N_ACTORS = 1, 2, 3, 4
_WORLDS = {}


def _worlds():
    """base scenes (57 floats each): cubes at rest with the arm up, the configured initial scene (cubes landing), the open
    gripper 3 cm above cubeA, cubeA held"""
    if not _WORLDS:
        import oracle
        oracle.load()
        import oracle.panda as P
        sc = P.default_scene()
        rest = P.init_world(1)
        for _ in range(30):
            P.step_batch(sc, rest, np.zeros((1, 9), np.float32))
        _WORLDS.update(rest=P.raw57(rest[0]), init=P.raw57(P.init_world(1)[0]),
                       near=P.raw57(grasp_world(P, sc, close_gripper=False, lift=0.03)), held=P.raw57(grasp_world(P, sc)))
    return _WORLDS


def _noise(K, T, seed):
    return np.random.default_rng(seed).standard_normal((K, T, 9)).astype(np.float32)


class Twin:
    """Two handles made the same way; A is commanded through the batch, B by m3_command.  scenes: the base scene of each call
    (the last one repeats); the arm and cubeA move a little every call."""

    def __init__(self, i, K, T, task, grip=1, scenes=("near",), lps=None, cost_kernel=True, bind=False, action_out=False,
                 spins=None, **cfg_kw):
        kw = dict(PK)
        kw.update(cfg_kw)
        self.i, self.bind, self.scenes = i, bind, list(scenes)
        self.engs = []
        if bind:
            self.dof = torch.zeros(1, 18, device="cuda:0")
            self.root = torch.zeros(1, N_ACTORS, 13, device="cuda:0")
        for _ in range(2):
            e = HipEngine(make_config(K=K, T=T, nu=9, env_type="panda_env", **kw))
            if not (e.cfg.sampling_random or e.cfg.mode_simple):
                e.set_noise(_noise(K, T, 300 + i))
            e.set_objective(task, GOALS[task], gripper_cmd=grip)
            if lps is not None:
                e.set_panda_lanes_per_sample(lps)
            if not cost_kernel:
                e.set_panda_reach_cost_kernel(False)
            if spins is not None:
                e.set_ladder_spins(spins)
            if bind:
                e.bind_sim_panda(self.dof, self.root, CUBEA, CUBEB, OBS)
            if action_out:
                rows = e.cfg.u_per_command if e.cfg.mode_simple else e.cfg.T
                e.set_action_out(torch.zeros(rows, 9, device="cuda:0"))
            self.engs.append(e)
        self.A, self.B = self.engs

    def set_world(self, call):
        w = _worlds()[self.scenes[min(call, len(self.scenes) - 1)]].copy()
        r = np.random.default_rng([self.i, call])
        w[0:7] += r.uniform(-0.01, 0.01, 7).astype(np.float32)           # arm
        w[18:20] += r.uniform(-0.004, 0.004, 2).astype(np.float32)       # cubeA x, y
        if self.bind:
            dof = np.zeros(18, np.float32)
            dof[0::2], dof[1::2] = w[0:9], w[9:18]
            self.dof[0] = torch.from_numpy(dof)
            for actor, o in ((CUBEA, 18), (CUBEB, 31), (OBS, 44)):
                self.root[0, actor] = torch.from_numpy(w[o:o + 13])
        else:
            for e in self.engs:
                e.set_world_panda_raw(w)

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
        fa = (self.A.panda_lanes_per_sample_used(), self.A.panda_near_share())
        fb = (self.B.panda_lanes_per_sample_used(), self.B.panda_near_share())
        assert fa == fb, f"{label}: handle {self.i}: kernel form / busy report {fa} != {fb}"
        return ia.calls, fa[0]

    def close(self):
        for e in self.engs:
            e.close()


def _run(twins, calls=6, order=None):
    """order(call) -> the indices of the twins commanded in that call (default: all, in order).  Returns the last call's
    (rollout launches, update launches) and every twin's forms, call by call."""
    batch = HipBatch(len(twins))
    expect = [0] * len(twins)
    forms = [[] for _ in twins]
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
                calls_i, lps = t.assert_same(f"call {c}")
                assert calls_i == expect[i]
                forms[i].append(lps)
        return batch.launches(), forms
    finally:
        batch.close()


@pytest.fixture
def twins():
    made = []
    yield made
    for t in made:
        t.close()


def test_tasks_grippers_and_sizes(twins):
    specs = [dict(K=4000, T=20, task="reach", grip=1, scenes=("rest", "near")),
             dict(K=4000, T=20, task="pick", grip=2, scenes=("near",)),
             dict(K=200, T=12, task="pick", grip=2, scenes=("near", "held")),
             dict(K=4000, T=20, task="place", grip=1, scenes=("held",)),
             dict(K=200, T=12, task="place", grip=2, scenes=("held",)),
             dict(K=200, T=12, task="reach", grip=2, scenes=("init", "rest")),
             dict(K=4000, T=20, task="reach", grip=1, multi_modal=True, scenes=("near",)),
             dict(K=200, T=12, task="reach", grip=1, multi_modal=True, scenes=("rest",), action_out=True),
             dict(K=4000, T=20, task="pick", grip=2, scenes=("near",))]
    twins += [Twin(i, **s) for i, s in enumerate(specs)]
    n = len(twins)
    # in order, reversed, alternating halves, everything again
    order = {0: list(range(n)), 1: list(range(n))[::-1], 2: list(range(0, n, 2)), 3: list(range(1, n, 2))[::-1],
             4: list(range(n)), 5: [8, 0, 4, 1]}
    (rl, ul), _ = _run(twins, calls=6, order=order.get)
    # the last call: rollouts reach 4000 / pick 4000 (handles 1 and 8: one group) / place 200; updates single mode with
    # 16 register rows (K = 4000) / 8 (K = 200, T = 12)
    assert (rl, ul) == (3, 2)


def test_forced_and_automatic_forms_and_the_busy_hysteresis(twins):
    flip = ("rest", "rest", "near", "near", "rest", "rest")
    specs = [dict(K=512, T=20, task="reach", lps=1, scenes=flip),
             dict(K=512, T=20, task="reach", lps=8, scenes=flip),
             dict(K=512, T=20, task="reach", lps=16, scenes=flip),
             dict(K=512, T=20, task="reach", scenes=flip),                       # cost kernel: sixteen lanes throughout
             dict(K=512, T=20, task="reach", cost_kernel=False, scenes=flip),    # one lane <-> eight lanes by the busy report
             dict(K=512, T=20, task="reach", cost_kernel=False, lps=16, scenes=flip),
             dict(K=512, T=20, task="pick", grip=2, lps=1, scenes=("near",)),
             dict(K=512, T=20, task="pick", grip=2, lps=8, scenes=("near",)),
             dict(K=512, T=20, task="pick", grip=2, scenes=("near",))]
    twins += [Twin(i, **s) for i, s in enumerate(specs)]
    _, forms = _run(twins, calls=6)
    assert forms[0] == [1] * 6 and forms[1] == [8] * 6 and forms[2] == [16] * 6 and forms[3] == [16] * 6
    # (the form follows the previous command's report: quiet until the report of the first command next to the cube)
    assert forms[4][:3] == [1, 1, 1] and forms[4][3] == 8, forms[4]
    assert forms[5] == [16] * 6 and forms[6] == [1] * 6 and forms[7] == [8] * 6 and forms[8] == [16] * 6


def test_general_instance_cov_and_bound_views(twins):
    specs = [dict(K=1000, T=20, task="pick", grip=2, sampling_random=True),
             dict(K=1000, T=20, task="reach", grip=1, mode_simple=True, sampling_random=True, u_per_command=10),
             dict(K=1000, T=20, task="reach", grip=1, sampling_random=True, scenes=("rest", "near")),
             dict(K=1000, T=20, task="pick", grip=2, update_cov=True),
             dict(K=1000, T=20, task="reach", grip=1, update_cov=True, scenes=("rest", "near")),
             dict(K=1000, T=20, task="pick", grip=2, bind=True),
             dict(K=1000, T=20, task="reach", grip=1, bind=True, scenes=("rest", "near")),
             dict(K=1000, T=20, task="reach", grip=1, bind=True, multi_modal=True),
             dict(K=1000, T=20, task="place", grip=1, bind=True, scenes=("held",))]
    twins += [Twin(i, **s) for i, s in enumerate(specs)]
    _run(twins, calls=6)


def test_batch_of_one_is_one_rollout_and_one_update_launch(twins):
    twins.append(Twin(0, K=4000, T=20, task="pick", grip=2))
    (rl, ul), _ = _run(twins, calls=6)
    assert (rl, ul) == (1, 1)


def test_homogeneous_group_is_one_rollout_and_one_update_launch(twins):
    twins += [Twin(i, K=200, T=12, task="pick", grip=2) for i in range(8)]
    (rl, ul), _ = _run(twins, calls=6)
    assert (rl, ul) == (1, 1)


@pytest.mark.parametrize("spins", [None, 0])
def test_multi_modal_group_larger_than_one_residency_chunk(twins, spins):
    # kb_update_small9<true, 8>: 4 resident workgroups per CU (update_small.hip; tests/test_batch_panda_cpu.py checks the
    # number against the code object); T = 200 -> 201 workgroups per handle -> 5 handles per launch
    n, T = 12, 200
    twins += [Twin(i, K=64, T=T, task="reach", grip=1, multi_modal=True, spins=spins) for i in range(n)]
    (rl, ul), _ = _run(twins, calls=3)
    assert rl == 1 and ul == math.ceil(n / (256 * 4 // (T + 1)))


def _state(e):
    return (e.info().calls, e.buffer(L.BUF_MEAN).cpu().numpy().tobytes(), e.buffer(L.BUF_TRAJ_COST).cpu().numpy().tobytes(),
            e.panda_lanes_per_sample_used(), e.panda_near_share())


L_ERR = {"BAD_ARG": -1, "HIP": -2, "SHAPE": -3, "STATE": -4, "UNSUPPORTED": -5}


def test_refusals_leave_every_handle_untouched():
    lib = L.load()
    made = []

    def eng(K=512, T=20, env="panda_env", **kw):
        if env == "panda_env":
            e = HipEngine(make_config(K=K, T=T, nu=9, env_type=env, **{**PK, **kw}))
            e.set_noise(_noise(e.cfg.K_local, T, 7))
            e.set_objective("reach", GOALS["reach"], gripper_cmd=1)
            e.set_world_panda_raw(_worlds()["near"])
        else:
            e = HipEngine(make_config(K=K, T=T, nu=2, u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3]))
            e.set_noise(np.random.default_rng(3).standard_normal((K, T, 2)).astype(np.float32))
            e.set_objective("push", (-1.0, -1.0))
        made.append(e)
        return e

    good, good2 = eng(), eng(K=200, T=12)
    good.command()           # (warm starts that a refused call must not touch: its busy report included)
    good2.command()
    torch.cuda.synchronize()
    batch = HipBatch(4)
    before = [_state(good), _state(good2)]

    def refused(engines, status, text):
        arr = (C.c_void_p * len(engines))(*[e._h.value for e in engines])
        rc = lib.m3_batch_command(batch._b, arr, len(engines), None)
        msg = lib.m3_batch_last_error(batch._b).decode()
        assert rc == status, (rc, msg)
        assert text in msg, msg
        torch.cuda.synchronize()
        assert [_state(good), _state(good2)] == before

    try:
        point = eng(K=2000, T=30, env="point_env")
        refused([good, good2, point], L_ERR["UNSUPPORTED"],
                "handle 2: point_env handle in a batch of panda_env handles (one environment per call)")
        refused([point, good], L_ERR["UNSUPPORTED"], "handle 1: panda_env handle in a batch of point_env handles")
        refused([good, eng(K=8192)], L_ERR["UNSUPPORTED"], "handle 1: its command does not take the one-launch update")
        refused([good, eng(K=100, T=240)], L_ERR["UNSUPPORTED"], "handle 1: its command does not take the one-launch update")
        refused([good2, good, eng(K=1024, K_local=512)], L_ERR["STATE"], "handle 2: sharded")
        sim = HipEngine(make_config(K=512, T=20, nu=9, env_type="panda_env", sim_only=True, **PK))
        made.append(sim)
        refused([good, sim], L_ERR["STATE"], "handle 1: handle was created sim_only")
        other = eng()
        stream = torch.cuda.Stream()
        other.use_torch_stream(stream)
        refused([good, good2, other], L_ERR["STATE"], "handle 2: its stream differs")
        no_noise = HipEngine(make_config(K=512, T=20, nu=9, env_type="panda_env", **PK))
        made.append(no_noise)
        refused([good, no_noise], L_ERR["STATE"], "handle 1: m3_rollout: no noise set")
        # ... and the same batch still works afterwards
        batch.command([good2, good])
        torch.cuda.synchronize()
        assert good.info().calls == before[0][0] + 1 and good2.info().calls == before[1][0] + 1
    finally:
        batch.close()
        for e in made:
            e.close()
