"""Prior samples (m3_set_prior_samples), the parts that need no GPU: the guard of the GPU tests on the oracle, the oracle planner
with priors equal to what it would assemble anyway, the host-side ancillary controllers of m3p2i_aip_amd/priors.py, the rollout
plan, the planner's Python-side rules, and the header / ctypes layout of the entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from m3p2i_aip_amd import _lib as L
from m3p2i_aip_amd import priors
from tests import point_scene_fixture as X
from tests import prior_samples_fixture as P
from tests import rollout_scenes_fixture as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TASKS = [("navigation", False), ("push", False), ("pull", False), ("push_pull", True)]


# ------------------------------------------------------------------ 1. the fixture
def test_prior_indices():
    assert P.prior_indices(64) == [0, 62] and P.prior_indices(100) == [0, 63, 64, 98]
    assert P.prior_indices(64, True) == [1, 62, 31, 33] and P.prior_indices(100, True) == [1, 63, 64, 98, 49, 51]
    assert P.prior_indices(4097) == [0, 63, 64, 4095]
    s = P.prior_seqs(4)
    assert s.shape == (4, X.T, 2) and s.dtype == F and (np.abs(s) > P.U_LIM).any(axis=(1, 2)).all()


@pytest.mark.parametrize("K", [64, 100])
@pytest.mark.parametrize("task,mm", TASKS)
def test_the_priors_are_felt_by_their_samples(oracle, task, mm, K):
    for wi, w0 in enumerate(X.start_worlds(oracle)):
        P.assert_priors_matter(oracle, task, mm, K, w0, f"{task} K={K} world {X.WORLD_NAMES[wi]}")


def test_the_priors_are_felt_on_top_of_an_arena_per_sample(oracle):
    P.assert_priors_matter(oracle, "push", False, 100, X.start_worlds(oracle)[2], "push K=100 rows", rows=R.cycle_rows(100))


# ------------------------------------------------------------------ 2. priors that repeat the planner's own rows
@pytest.mark.parametrize("task,mm", [("push", False), ("push_pull", True)])
def test_priors_equal_to_the_assembled_rows_reproduce_the_plain_planner(oracle, task, mm):
    K = 64
    idx = P.prior_indices(K, mm)
    mk = lambda: oracle.make_cfg(K, X.T, 2, task=task, goal=X.GOAL, multi_modal=mm, filter_u=False)
    plain = oracle.OraclePointPlanner(mk(), X.actions(K, X.T))
    pri = P.make_prior_planner(oracle, mk(), X.actions(K, X.T), idx, np.zeros((len(idx), X.T, 2), F))
    w0 = X.start_worlds(oracle)[2].copy()
    for call in range(3):
        w0[0] += 0.02 * call
        # what the planner is about to assemble for those samples: its state shifted as command() shifts it
        sh = oracle.shift
        act = oracle.assemble_actions(pri.cfg, pri.delta, sh(pri.mean), sh(pri.mean1), sh(pri.mean2), sh(pri.best1), sh(pri.best2))
        pri.set_priors(idx, act[idx])
        ua, ub = plain.command(w0), pri.command(w0)
        assert ua.tobytes() == ub.tobytes(), call
        for name in ("states", "actions", "cost_h", "J", "w"):
            assert plain.last[name].tobytes() == pri.last[name].tobytes(), (call, name)
        assert plain.pend.tobytes() == pri.pend.tobytes()


# ------------------------------------------------------------------ 3. the ancillary controllers
def _end(start, u, dt):
    return np.asarray(start, np.float64) + (u.astype(np.float64) * dt).sum(axis=0)


def test_go_to_shapes_saturation_and_end_point():
    T, dt, u_max = 30, 0.05, [3.0, 3.0]
    start, target = (-1.0, 0.5), (1.0, 1.25)
    speeds = (1.0, 0.75, 0.5)
    u = priors.go_to(start, target, T, dt, u_max, speeds)
    assert u.shape == (3, T, 2) and u.dtype == np.float32
    d = np.subtract(target, start); d = d / np.hypot(*d)
    for j, f in enumerate(speeds):
        sp = np.hypot(u[j, :, 0], u[j, :, 1])
        assert sp.max() <= f * 3.0 * (1 + 1e-6) and abs(sp[0] - f * 3.0) <= 1e-5, (j, sp)   # saturated from the first step
        np.testing.assert_allclose(u[j, 0] / sp[0], d, atol=1e-6)
        assert (np.abs(u[j]) <= 3.0).all()
        # 30 steps of 0.05 s at 1.5 .. 3 m/s cover 2.25 .. 4.5 m; the target is 2.136 m away: reached, then at rest
        assert np.abs(_end(start, u[j], dt) - target).max() <= 1e-6, j
        assert (u[j, -1] == 0.0).all()
    # a target out of reach: saturated all the way, on the line
    far = priors.go_to(start, (100.0, 0.5), 8, dt, u_max, (1.0,))
    np.testing.assert_allclose(far[0], [[3.0, 0.0]] * 8, atol=1e-6)
    # asymmetric limits: the smaller one bounds the speed
    assert np.hypot(*priors.go_to(start, target, 4, dt, [3.0, 1.0], (1.0,))[0, 0]) <= 1.0 + 1e-6


def test_push_behind_goes_behind_the_box_first():
    T, dt = 40, 0.05
    robot, box, goal = (0.0, -1.0), (0.0, 0.0), (1.5, 0.0)
    u = priors.push_behind(robot, box, goal, T, dt, [3.0, 3.0], speeds=(1.0, 0.5), standoff=0.45)
    assert u.shape == (2, T, 2) and u.dtype == np.float32 and (np.hypot(u[..., 0], u[..., 1]) <= 3.0 + 1e-5).all()
    behind = np.array([-0.45, 0.0])
    d0 = behind - np.array(robot); d0 /= np.hypot(*d0)
    np.testing.assert_allclose(u[0, 0] / np.hypot(*u[0, 0]), d0, atol=1e-6)     # first toward the stand-off point ...
    pos = np.array(robot, np.float64)
    reached = None
    for t in range(T):
        pos = pos + u[0, t].astype(np.float64) * dt
        if reached is None and np.hypot(*(pos - behind)) <= 0.05 + 1e-6:
            reached = t
    assert reached is not None and reached < T - 2
    assert u[0, reached + 1, 0] > 0 and abs(u[0, reached + 1, 1]) < 0.2 * u[0, reached + 1, 0]   # ... then toward the goal
    assert set(priors.CONTROLLERS) == {"go_to", "push_behind"}


# ------------------------------------------------------------------ 4. the rollout plan (host only)
def _plan(task, mm, scene, K, priors_on, lanes=64, form_request=0, minima=0):
    out = (C.c_int * 9)()
    rc = L.load().m3_point_rollout_plan_ex(task, int(mm), 0, 0, 0, K, 30, lanes, 0.05, 2, 6, 0, scene, form_request, minima, priors_on, out)
    return rc, dict(zip(("instance", "ref", "form", "weighted", "scene", "blocks", "rows", "lanes", "priors"), out))


@pytest.mark.parametrize("task,mm", [(0, False), (1, False), (2, False), (3, True)])
def test_the_plan_of_a_handle_with_priors(task, mm):
    for K, blocks in ((64, 1), (65, 2), (65537, 1025)):
        for scene in (1, 2):
            for form_request in (0, 1, -1):
                rc, p = _plan(task, mm, scene, K, 1, form_request=form_request)
                assert rc == 0 and p == dict(instance=-1, ref=0, form=0, weighted=1, scene=scene, blocks=blocks, rows=0, lanes=64,
                                             priors=1), (K, p)
            rc, p = _plan(task, mm, scene, K, 0)
            assert rc == 0 and p["priors"] == 0 and p["scene"] == scene
        # without priors the answers of m3_point_rollout_plan
        old = (C.c_int * 8)()
        assert L.load().m3_point_rollout_plan(task, int(mm), 0, 0, 0, K, 30, 64, 0.05, 2, 6, 0, 0, 0, 0, old) == 0
        rc, p = _plan(task, mm, 0, K, 0)
        assert rc == 0 and list(old) == list(p.values())[:8]
    assert _plan(task, mm, 0, 64, 1)[0] == -1        # a handle with priors never runs a compiled-in scene
    assert _plan(task, mm, 1, 64, 2)[0] == -1
    assert _plan(task, mm, 1, 2000, 1, minima=1)[1]["rows"] == 32


# ------------------------------------------------------------------ 5. the planner's Python-side rules
class _Engine:
    def __init__(self):
        self.calls = []

    def set_prior_samples(self, seqs=None, indices=None):
        self.calls.append(None if seqs is None else (np.asarray(seqs).shape, list(indices)))


def _planner(mm=False, env="point_env", world_size=1):
    import torch
    from m3p2i_aip_amd import planner
    p = object.__new__(planner.MPPI)
    p.env_type, p.K, p.K_local, p.k_offset, p.T, p.nu = env, 8, 8, 0, 4, 2
    p.multi_modal, p.mppi_mode, p.world_size, p.collective, p.device = mm, "halton-spline", world_size, None, "cpu"
    p.u_max, p.u_min = torch.tensor([3.0, 3.0]), torch.tensor([-3.0, -3.0])
    p._engine, p._fused, p._sim, p._bound_sim = _Engine(), True, None, None
    return p


def test_planner_default_indices_and_refusals():
    import torch
    from m3p2i_aip_amd import planner
    seqs = np.full((2, 4, 2), 5.0, F)
    p = _planner()
    p.set_prior_samples(seqs)
    assert p._engine.calls == [((2, 4, 2), [0, 1])] and p.has_prior_samples
    # the step path writes the clamped rows
    act = torch.zeros(8, 4, 2)
    out = p._write_priors(act, torch.arange(8))
    assert (out[:2] == 3.0).all() and (out[2:] == 0.0).all()
    with pytest.raises(ValueError, match="prior samples"):
        planner.command_batch([p], [np.zeros(4, F)])
    p.set_prior_samples(None)
    assert p._engine.calls[-1] is None and not p.has_prior_samples
    assert (p._write_priors(torch.zeros(8, 4, 2), torch.arange(8)) == 0.0).all()
    q = _planner(mm=True)
    for mode in ("halton-spline", "simple"):        # (the library refuses 0 and K/2 whenever multi_modal is set)
        q.mppi_mode = mode
        with pytest.raises(ValueError, match="needs indices"):
            q.set_prior_samples(seqs)
    q.mppi_mode = "halton-spline"
    assert q._engine.calls == []
    q.set_prior_samples(seqs, [1, 5])
    assert q._engine.calls == [((2, 4, 2), [1, 5])]
    with pytest.raises(ValueError, match="point_env only"):
        _planner(env="panda_env").set_prior_samples(seqs)
    with pytest.raises(ValueError, match="unsharded"):
        _planner(world_size=2).set_prior_samples(seqs)


def test_prior_samples_config_key():
    from m3p2i_aip_amd import compat
    assert compat.make_config("config_point").prior_samples is None
    cfg = compat.make_config("config_point", ["task=push", "prior_samples={controller: push_behind, n: 4}"])
    assert cfg.prior_samples == dict(controller="push_behind", n=4) and compat.check_prior_samples(cfg) == ("push_behind", 4)
    assert compat.prior_sample_indices(200, 4, False) == [0, 1, 2, 3]
    assert compat.prior_sample_indices(200, 5, True) == [1, 2, 3, 101, 102]       # never 0, K / 2 or K - 1
    for bad in ("prior_samples={controller: straight}", "prior_samples={n: 4}", "prior_samples={controller: go_to, m: 1}",
                "prior_samples={controller: go_to, n: 0}", "prior_samples={controller: go_to, n: 99}"):
        with pytest.raises(ValueError, match="prior_samples"):
            compat.make_config("config_point", ["mppi.num_samples=64", bad])
    with pytest.raises(ValueError, match="point_env only"):
        compat.make_config("config_panda", ["prior_samples={controller: go_to}"])


def test_the_dead_config_switches_stay_ignored():
    from m3p2i_aip_amd import planner
    assert planner.MPPIConfig.sample_other_priors is False and planner.MPPIConfig.use_priors is False
    src = open(os.path.join(ROOT, "m3p2i_aip_amd", "planner.py")).read()
    assert not re.search(r"(_get\(m, |m\.|cfg\.)(sample_other_priors|use_priors)", src)


# ------------------------------------------------------------------ 6. symbols
def test_the_entry_points_exist_with_their_prototypes():
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    assert "#define M3_ABI_VERSION 4" in hdr and "#define M3_MAX_PRIOR_SAMPLES 256" in hdr
    assert L.MAX_PRIOR_SAMPLES == 256
    bound = {s[0]: (s[1], list(s[2])) for s in L.SYMBOLS}
    IP = C.POINTER(C.c_int)
    assert bound["m3_set_prior_samples"] == (C.c_int, [L._H, C.c_void_p, IP, C.c_int])
    assert bound["m3_set_prior_samples_device"] == (C.c_int, [L._H, C.c_void_p, IP, C.c_int])
    assert bound["m3_prior_samples_set"] == (C.c_int, [L._H])
    assert bound["m3_get_prior_sample"] == (C.c_int, [L._H, C.c_int, IP, L._FP])
    assert bound["m3_prior_samples_used"] == (C.c_int, [L._H])
    assert re.search(r"^int m3_set_prior_samples\(m3_handle\* h, const float\* seqs, const int\* sample_idx, int n\);", hdr, re.M)
    assert re.search(r"^int m3_set_prior_samples_device\(m3_handle\* h, const float\* seqs_dev, const int\* sample_idx, int n\);", hdr, re.M)
    assert re.search(r"^int m3_prior_samples_set\(const m3_handle\* h\);", hdr, re.M)
    assert re.search(r"^int m3_get_prior_sample\(const m3_handle\* h, int j, int\* sample_idx, float\* seq\);", hdr, re.M)
    assert re.search(r"^int m3_prior_samples_used\(m3_handle\* h\);", hdr, re.M)
    lib = L.load()
    k = C.c_int()
    # (no handle can be created without a device -- the handle's answers are checked in tests/test_prior_samples_gpu.py)
    assert lib.m3_set_prior_samples(None, None, None, 0) == -1 and lib.m3_set_prior_samples_device(None, None, None, 0) == -1
    assert lib.m3_prior_samples_set(None) == -1 and lib.m3_prior_samples_used(None) == -1
    assert lib.m3_get_prior_sample(None, 0, C.byref(k), None) == -1
