"""Prior controllers on the device (m3_set_prior_controller) on the GPU: the table k_prior_controllers
fills against the host build of the same header (tests/native/prior_controllers_host.cpp), bit for bit, with the world set and
with bound views; a handle with a controller against a twin that gets that same table through m3_set_prior_samples_device,
byte for byte over six warm-started commands with the world moved between them; fused against the step probe; the life cycle
and every refusal.  K = 64 and K = 100 (a half-empty wavefront), T = 12 (the shortest horizon the spline sampler takes)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipEngine, make_config  # noqa: E402
from tests import prior_controllers_fixture as PC  # noqa: E402
from tests import prior_samples_fixture as P  # noqa: E402
from tests.test_batch_command_gpu import PK, Twin, _world  # noqa: E402

F = np.float32
BAD_ARG, STATE, UNSUPPORTED = -1, -4, -5
T = 12


@pytest.fixture(scope="module")
def host_prog(tmp_path_factory):
    return PC.build(tmp_path_factory.mktemp("prior_controllers_gpu"))


def _table(eng):
    eng.prior_controller_fill()
    torch.cuda.synchronize()
    return eng.prior_table().cpu().numpy()


def _host_case(eng, kind, w, goal):
    pc = eng.prior_controller()
    return PC.case(kind, eng.cfg.T, [eng.cfg.u_max[0], eng.cfg.u_max[1]], w[0:2], w[4:6], goal, factors=pc["speeds"],
                   dt=eng.cfg.dt, standoff=pc["standoff"], reach=pc["reach"])


# ------------------------------------------------------------------ 1: the table against the host build
@pytest.mark.parametrize("bind", [False, True])
def test_filled_table_equals_the_host_build_bit_for_bit(host_prog, bind):
    """the inputs of tests/test_prior_controllers_cpu.py, both kinds, both limits, T = 12 and 30, through one handle per
    (T, u_max): world0 (m3_set_world_point_raw) or row 0 of bound views"""
    kinds = {PC.GO_TO: ("go_to", "navigation"), PC.PUSH_BEHIND: ("push_behind", "push")}
    cases, got = [], []
    for Th in PC.HORIZONS:
        for um in PC.U_MAX:
            t = Twin(0, K=64, T=Th, task="push", goal=[0.0, 0.0], bind=bind, filter_u=False,
                     **{**PK, "u_max": [abs(um[0]), abs(um[1])], "u_min": [-abs(um[0]), -abs(um[1])]})
            eng = t.A
            try:
                assert abs(eng.cfg.dt - 0.05) < 1e-6
                for kind, (name, task) in kinds.items():
                    eng.set_prior_controller(name, 4, [3, 17, 40, 62])
                    for robot, box, goal in PC.INPUTS:
                        w = np.zeros(18, F)
                        w[0:2], w[4:6], w[6], w[11:13], w[13] = robot, box, 1.0, (3.0, -3.0), 1.0
                        eng.set_objective(task, list(goal))
                        if bind:
                            t.dof[0] = torch.tensor([w[0], 0.0, w[1], 0.0])
                            t.root[0, 6, 0:2] = torch.tensor(w[4:6])      # (BOX_ACTOR of tests/test_batch_command_gpu.py)
                        else:
                            eng.set_world_point_raw(w)
                        got.append(_table(eng).copy())
                        cases.append(_host_case(eng, kind, w, PC.f32(goal)))
            finally:
                t.close()
    want = PC.run(host_prog, cases)
    bad = 0
    for c, g, h in zip(cases, got, want):
        assert g.shape == h.shape == (4, c["T"], 2)
        bad += int((g.view(np.uint32) != h.view(np.uint32)).sum())
        np.testing.assert_array_equal(g.view(np.uint32), h.view(np.uint32), err_msg=str(c))
    print(f"{len(cases)} tables, {sum(g.size for g in got)} words, {bad} differ from the host build")
    assert len(cases) == 2 * 2 * 2 * len(PC.INPUTS) and any((g != 0).any() for g in got)


# ------------------------------------------------------------------ 2: a controller is its table through the device setter
CASES = [("push", False, "push_behind", 64, False), ("push", False, "push_behind", 100, True),
         ("navigation", False, "go_to", 100, False), ("push_pull", True, "push_behind", 64, True),
         ("pull", False, "go_to", 100, False)]


@pytest.mark.parametrize("task,mm,kind,K,bind", CASES)
def test_controller_handle_equals_a_twin_with_that_table(host_prog, task, mm, kind, K, bind):
    """A: the controller.  B: before each command, A's table (filled for this call's world, read back) through
    m3_set_prior_samples_device.  Every buffer and m3_info byte for byte over six warm-started commands; each call's table
    differs from the last call's (the world moved) and equals the host build's."""
    idx = [1, 2, K // 2 + 1, K // 2 + 2] if mm else P.prior_indices(K)[:4]
    goal = [-1.0, -1.0]
    t = Twin(1, K=K, T=T, task=task, goal=goal, multi_modal=mm, bind=bind)
    live = None
    try:
        t.A.set_prior_controller(kind, len(idx), idx)
        last = None
        for c in range(6):
            t.set_world(c)
            tab = _table(t.A)
            want = PC.run(host_prog, [_host_case(t.A, L.PRIOR_CONTROLLER_KINDS[kind], _world(1, c), PC.f32(goal))])[0]
            np.testing.assert_array_equal(tab.view(np.uint32), want.view(np.uint32), err_msg=f"call {c}")
            assert last is None or tab.tobytes() != last
            last = tab.tobytes()
            t.B.set_prior_samples(torch.as_tensor(tab, device=t.B.device), idx)
            if c == 1:
                live = L.load().m3_owned_blocks_live()
            t.A.command()
            t.B.command()
            torch.cuda.synchronize()
            assert t.assert_same(f"{task} {kind} call {c}") == c + 1
            assert t.A.prior_samples_used() == 1 and t.B.prior_samples_used() == 1
            # the rollout took the rows: the stored actions of the prior samples are the clamped table
            np.testing.assert_array_equal(t.A.actions.cpu().numpy()[idx].view(np.uint32), np.clip(tab, -3, 3).astype(F).view(np.uint32))
        assert L.load().m3_owned_blocks_live() == live        # nothing allocated on the command path
        assert t.A.prior_controller()["kind"] == L.PRIOR_CONTROLLER_KINDS[kind] and t.B.prior_controller() is None
    finally:
        t.close()


# ------------------------------------------------------------------ 3: fused versus step
def test_fused_path_is_the_step_path_with_a_controller():
    from tests.test_prior_samples_gpu import _side
    t = _side()
    try:
        p = t.motion_planner
        assert p._fused is None
        p.set_prior_controller("push_behind", 4)
        assert p._engine.prior_samples_set() == 4
        t.first_plan(t.sim._dof_state[0:1].clone(), t.sim._root_state[0:1].clone())
        print(f"probe {p.probe_result}")
        assert p.probe_result == dict(fused=True, max_abs_diff=0.0)
        tab = p._engine.prior_table().cpu().numpy()
        assert np.abs(tab).max() > 0.5
        lim = np.maximum(np.minimum(tab, F(p.u_max.cpu().numpy())), F(p.u_min.cpu().numpy()))
        np.testing.assert_array_equal(p.perturbed_action[:4].cpu().numpy().view(np.uint32), lim.view(np.uint32))   # the step leg's rows
        assert p._engine.prior_samples_used() == 1
    finally:
        t.close()


# ------------------------------------------------------------------ 4: life cycle and refusals
def _pc(kind=1, n=4, **kw):
    pc = L.PriorController()
    L.load().m3_default_prior_controller(C.byref(pc), kind, n)
    pc.kind, pc.n = kind, n
    for k, v in kw.items():
        if k == "speed":
            pc.speed[v[0]] = v[1]
        else:
            setattr(pc, k, v)
    return pc


def _refused(eng, code, match, pc, idx):
    arr = (C.c_int * max(len(idx), 1))(*idx) if idx is not None else None
    rc = eng.lib.m3_set_prior_controller(eng._h, C.byref(pc), arr)
    msg = eng.lib.m3_last_error(eng._h).decode()
    assert rc == code, (rc, msg)
    assert "m3_set_prior_controller" in msg and match in msg, msg


def test_life_cycle_and_refusals():
    K = 64
    lib = L.load()
    idx = [3, 17, 40, 62]
    for mm, task in ((False, "push"), (True, "push_pull")):
        t = Twin(2, K=K, T=T, task=task, goal=[-1.0, -1.0], multi_modal=mm)
        eng, ref = t.A, t.B
        try:
            p, n = C.c_void_p(), C.c_int()
            assert lib.m3_prior_table(eng._h, C.byref(p), C.byref(n)) == STATE and eng.prior_controller() is None
            assert lib.m3_prior_controller_fill(eng._h) == STATE and b"no prior controller" in lib.m3_last_error(eng._h)
            # the first call allocates what the first m3_set_prior_samples call allocates, and nothing more
            b0 = lib.m3_owned_blocks_live()
            eng.set_prior_controller("push_behind", 4, idx)
            b1 = lib.m3_owned_blocks_live()
            ref.set_prior_samples(P.prior_seqs(4, T), idx)
            assert lib.m3_owned_blocks_live() - b1 == b1 - b0 > 0
            eng.set_prior_controller("go_to", 2, idx[:2]); eng.set_prior_controller("push_behind", 4, idx)
            eng.set_prior_samples(P.prior_seqs(4, T), idx); eng.set_prior_controller("push_behind", 4, idx)
            assert lib.m3_owned_blocks_live() == b1 + (b1 - b0)
            assert eng.prior_samples_set() == 4 and eng.prior_controller() == dict(
                kind=2, n=4, speeds=[1.0, 0.75, 0.5, 0.25], standoff=float(F(0.45)), reach=float(F(0.05)))
            # every refusal, every check before any state changes
            _refused(eng, BAD_ARG, "unknown kind 0", _pc(0), idx)
            _refused(eng, BAD_ARG, "unknown kind 3", _pc(3), idx)
            _refused(eng, BAD_ARG, "n is 0, must be in 1 .. 16", _pc(1, 0), idx)
            _refused(eng, BAD_ARG, "n is 17, must be in 1 .. 16", _pc(1, 17), list(range(1, 18)))
            _refused(eng, BAD_ARG, "speed factor 2 is not a finite positive", _pc(speed=(2, float("nan"))), idx)
            _refused(eng, BAD_ARG, "speed factor 0 is not a finite positive", _pc(speed=(0, 0.0)), idx)
            _refused(eng, BAD_ARG, "speed factor 3 is not a finite positive", _pc(speed=(3, float("inf"))), idx)
            _refused(eng, BAD_ARG, "standoff is not a finite positive", _pc(2, standoff=-0.45), idx)
            _refused(eng, BAD_ARG, "reach is not a finite positive", _pc(2, reach=0.0), idx)
            _refused(eng, BAD_ARG, "null sample_idx", _pc(), None)
            _refused(eng, BAD_ARG, "prior 1: sample 64 is outside", _pc(), [5, K, 6, 7])
            _refused(eng, BAD_ARG, "prior 0: sample -1 is outside", _pc(), [-1, 5, 6, 7])
            _refused(eng, BAD_ARG, "prior 2: sample 63 is the zero-noise", _pc(), [5, 6, K - 1, 7])
            _refused(eng, BAD_ARG, "prior 3: sample 17 listed twice", _pc(), [17, 5, 6, 17])
            if mm:
                _refused(eng, BAD_ARG, "prior 0: sample 0 is a best-trajectory sample", _pc(), [0, 5, 6, 7])
                _refused(eng, BAD_ARG, "prior 1: sample 32 is a best-trajectory sample", _pc(), [5, K // 2, 6, 7])
            assert eng.prior_samples_set() == 4 and eng.prior_controller()["kind"] == 2
            # the values of a controller's priors are the device's
            k = C.c_int()
            assert lib.m3_get_prior_sample(eng._h, 1, C.byref(k), None) == 0 and k.value == idx[1]
            with pytest.raises(L.M3Error):
                eng.prior_sample(0)
            # survives m3_reset; the next command runs it
            eng.reset()
            assert eng.prior_controller()["kind"] == 2 and eng.prior_samples_set() == 4
            t.set_world(0)
            eng.command(sync_host=True)
            assert eng.prior_samples_used() == 1
            # PUSH_BEHIND on a navigation task: refused before any launch, not downgraded
            calls = eng.info().calls
            before = eng.buffer(L.BUF_TRAJ_COST).clone()
            eng.set_objective("navigation", [-1.0, -1.0])
            with pytest.raises(L.M3Error, match=r"error -4: .*PUSH_BEHIND.*navigation"):
                eng.command()
            assert lib.m3_prior_controller_fill(eng._h) == STATE
            torch.cuda.synchronize()
            assert eng.info().calls == calls and torch.equal(before, eng.buffer(L.BUF_TRAJ_COST))
            eng.set_objective(task, [-1.0, -1.0])
            # the run-time-scene instance forced off: refused as for any handle with priors
            eng.set_point_scene_instance(0)
            with pytest.raises(L.M3Error, match=r"forced off.*m3_set_prior_samples"):
                eng.command()
            eng.set_point_scene_instance(-1)
            # against m3_set_prior_samples the last call wins
            eng.set_prior_samples(P.prior_seqs(2, T), idx[:2])
            assert eng.prior_controller() is None and eng.prior_samples_set() == 2 and eng.prior_sample(0)[0] == idx[0]
            assert lib.m3_prior_controller_fill(eng._h) == STATE
            eng.set_prior_controller("go_to", 3, idx[:3])
            assert eng.prior_controller()["kind"] == 1 and eng.prior_samples_set() == 3
            # pc == NULL clears controller and priors: byte for byte the handle without priors
            eng.set_prior_controller(None)
            ref.set_prior_samples(None)
            assert eng.prior_samples_set() == 0 and eng.prior_controller() is None
            eng.reset(); ref.reset()
            for c in range(2):
                t.set_world(c)
                eng.command(); ref.command()
                torch.cuda.synchronize()
                assert t.assert_same(f"{task} cleared, call {c}") == c + 1
                assert eng.prior_samples_used() == 0
            # m3_set_prior_samples(NULL) clears a controller as well
            eng.set_prior_controller("go_to", 3, idx[:3])
            eng.set_prior_samples(None)
            assert eng.prior_samples_set() == 0 and eng.prior_controller() is None
        finally:
            t.close()


def test_refusals_by_the_kind_of_handle():
    lib = L.load()
    pc, arr = _pc(1, 2), (C.c_int * 2)(3, 4)
    sim = HipEngine(make_config(K=64, T=12, nu=2, sim_only=True, filter_u=False, **PK))
    try:
        assert lib.m3_set_prior_controller(sim._h, C.byref(pc), arr) == STATE
        assert b"m3_set_prior_controller: planner handles only" in lib.m3_last_error(sim._h)
    finally:
        sim.close()
    p = HipEngine(make_config(K=64, T=12, nu=9, env_type="panda_env", u_min=[-2] * 9, u_max=[2] * 9, noise_sigma_diag=[1] * 9))
    try:
        assert lib.m3_set_prior_controller(p._h, C.byref(pc), arr) == UNSUPPORTED
        assert b"m3_set_prior_controller: point_env only" in lib.m3_last_error(p._h)
        assert lib.m3_set_prior_controller(p._h, None, None) == UNSUPPORTED
        assert lib.m3_get_prior_controller(p._h, C.byref(pc)) == UNSUPPORTED and lib.m3_prior_controller_fill(p._h) == UNSUPPORTED
        assert lib.m3_prior_table(p._h, None, None) == UNSUPPORTED
    finally:
        p.close()
    sh = HipEngine(make_config(K=128, K_local=64, k_offset=64, T=12, nu=2, **PK))
    try:
        assert lib.m3_set_prior_controller(sh._h, C.byref(_pc(1, 2)), arr) == UNSUPPORTED
        assert b"m3_set_prior_controller: sharded handle (K_local != K_global)" in lib.m3_last_error(sh._h)
        assert lib.m3_prior_samples_set(sh._h) == 0
    finally:
        sh.close()
