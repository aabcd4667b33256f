"""panda_env prior samples (m3_set_panda_prior_samples), the parts that need no GPU: the guards of the GPU
tests on the oracle alone, the oracle planner with priors equal to what it would assemble anyway, the arm's host-side
controllers of m3p2i_aip_amd/priors.py, the config key, the planner's Python-side rules on a recording engine stub, the header /
ctypes layout of the entry points, and the native walk of the variant decision with priors_on over every other input."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from m3p2i_aip_amd import _lib as L
from m3p2i_aip_amd import priors
from tests import panda_prior_samples_fixture as PF
from tests import panda_rollout_scenes_ref as R
from tests import panda_scene_fixture as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def P(oracle):
    import oracle.panda as P
    P.lib()
    return P


# ------------------------------------------------------------------ 1. the fixture
def test_prior_indices_and_sequences():
    assert PF.prior_indices(64) == [0, 5, 10, 15, 20, 25, 30, 35, 40, 45, 50, 55, 60, 62]
    assert PF.prior_indices(61) == [0, 5, 10, 15, 20, 25, 30, 35, 40, 45, 50, 55, 59]                 # (60 = K - 1 is refused)
    assert PF.prior_indices(64, True) == [5, 10, 15, 20, 25, 30, 35, 40, 45, 50, 55, 60, 31, 33, 62]
    assert PF.prior_indices(61, True) == [5, 10, 15, 20, 25, 35, 40, 45, 50, 55, 29, 31, 59]          # (30 = K / 2 is refused)
    for K in (61, 64):
        for mm in (False, True):
            idx = PF.prior_indices(K, mm)
            assert len(set(idx)) == len(idx) and K - 1 not in idx and all(0 <= k < K for k in idx)
            assert not mm or (0 not in idx and K // 2 not in idx)
            # first and last sample slots of wavefronts in every form, with and without shadow slots
            for spw in (3, 4, 8, 62, 63, 64):
                slots = {k % spw for k in idx}
                assert (0 in slots or mm) and len(slots) >= min(spw, 3), (K, mm, spw)
    s = PF.prior_seqs(14)
    assert s.shape == (14, X.T, 9) and s.dtype == F
    assert ((s < np.array(X.UMIN, F)) | (s > np.array(X.UMAX, F))).mean() > 0.1                        # more than a tenth is clamped


# ------------------------------------------------------------------ 2. the guards, on the oracle alone
@pytest.mark.parametrize("case,mm,K", [("reach", False, 64), ("reach", True, 64), ("pick", False, 64), ("pick", True, 64),
                                       ("reach", False, 61), ("pick", False, 61)])
def test_the_priors_are_felt_by_their_samples(P, case, mm, K):
    PF.assert_priors_matter(P, case, mm, K, f"{case} mm {mm} K {K}")


def test_the_priors_are_felt_on_top_of_a_workspace_per_sample(P):
    PF.assert_priors_matter(P, "reach", False, X.K, "reach cycle", rows=R.cycle_rows("reach", X.K))


def test_the_gripper_command_stays_the_tasks(P):
    """gripper_cmd 2: a prior's columns 7 and 8 leave the stored actions at -1.5 * u_scale; gripper_cmd 0: they are the prior's"""
    K = X.K
    idx = PF.prior_indices(K)
    seqs = PF.prior_seqs(len(idx))
    for grip in (2, 1, 0):
        cfg = PF.make_cfg(P, "pick", K, grip=grip)
        p = PF.make_panda_prior_planner(P, cfg, X.delta_of(K), idx, seqs)
        p.command(X.world_of(40))
        a = p.last["actions"][idx]
        want = PF.clip(cfg, seqs) * F(cfg.u_scale)
        assert a[:, :, :7].tobytes() == want[:, :, :7].tobytes(), grip
        if grip:
            assert (a[:, :, 7:] == F(1.5 if grip == 1 else -1.5) * F(cfg.u_scale)).all(), grip
            assert (want[:, :, 7:] != a[:, :, 7:]).mean() > 0.5                    # ... which is not what the prior asked for
        else:
            assert a[:, :, 7:].tobytes() == want[:, :, 7:].tobytes()


# ------------------------------------------------------------------ 3. priors that repeat the planner's own rows
@pytest.mark.parametrize("case,mm", [("reach", False), ("pick", True)])
def test_priors_equal_to_the_assembled_rows_reproduce_the_plain_planner(P, oracle, case, mm):
    K = X.K
    world = X.world_of(PF.CASES[case][0])
    idx = PF.prior_indices(K, mm)
    plain = P.OraclePandaPlanner(PF.make_cfg(P, case, K, mm), X.delta_of(K))
    pri = PF.make_panda_prior_planner(P, PF.make_cfg(P, case, K, mm), X.delta_of(K), idx, np.zeros((len(idx), X.T, 9), F))
    for call in range(2):
        # what the planner is about to assemble for those samples: its state shifted as command() shifts it
        sh = oracle.shift
        act = oracle.assemble_actions(pri.cfg, pri.delta, sh(pri.mean), sh(pri.mean1), sh(pri.mean2), sh(pri.best1), sh(pri.best2))
        pri.set_priors(idx, act[idx])
        ua, ub = plain.command(world), pri.command(world)
        assert ua.tobytes() == ub.tobytes(), call
        for name in ("states", "actions", "cost_h", "J", "w"):
            assert plain.last[name].tobytes() == pri.last[name].tobytes(), (call, name)


# ------------------------------------------------------------------ 4. the arm's controllers
def test_hold_and_joint_go_to():
    assert set(priors.PANDA_CONTROLLERS) == {"hold", "joint_go_to"} and set(priors.CONTROLLERS) == {"go_to", "push_behind"}
    h = priors.hold(12)
    assert h.shape == (1, 12, 9) and h.dtype == F and not h.any()
    assert priors.hold(12, 4).shape == (4, 12, 9)
    T, dt = 40, 0.01
    u_max = [2.0] * 7 + [1.5] * 2
    q = np.array([0.0, -0.5, 0.1, -2.0, 0.0, 1.5, 0.7, 0.04, 0.04])
    # joint 0: 0.3 rad away -- out of reach in 0.4 s at 0.5 rad/s, reached at 2 rad/s after 15 steps; joint 1: 0.05 rad, reached
    # by every speed; joint 2: at the target already; joint 3: the other direction
    tgt7 = np.array([0.3, -0.45, 0.1, -2.2, 0.0, 1.5, 0.7])
    speeds = (1.0, 0.75, 0.5, 0.25)
    u = priors.joint_go_to(q, tgt7, T, dt, u_max, speeds)
    assert u.shape == (4, T, 9) and u.dtype == F
    assert not u[:, :, 7:].any() and not u[:, :, 2].any() and not u[:, :, 4:7].any()       # seven targets: the fingers stay zero
    for s, f in enumerate(speeds):
        assert np.abs(u[s, :, :7]).max() <= f * 2.0 * (1 + 1e-6)
        assert u[s, 0, 0] == F(f * 2.0) and u[s, 0, 3] == F(-f * 2.0)                      # saturated from the first step
        end = q[:7] + (u[s, :, :7].astype(np.float64) * dt).sum(axis=0)
        reached = np.abs(end - tgt7) <= 1e-6
        assert reached[1] and reached[2], s                                                 # arrival ...
        assert reached[0] == (f * 2.0 * T * dt >= 0.3 - 1e-9), (s, end[0])
        for j in np.flatnonzero(reached):
            nz = np.flatnonzero(u[s, :, j])
            assert nz.size == 0 or (u[s, nz[-1] + 1:, j] == 0.0).all()                      # ... and zeros after it
        if f == 1.0:
            assert (u[s, 15:, 0] == 0.0).all() and u[s, 14, 0] != 0.0
    # nine targets: the fingers follow theirs at factor * |u_max[7:]|
    u9 = priors.joint_go_to(q, np.concatenate([tgt7, [0.0, 0.0]]), T, dt, u_max, (1.0,))
    assert u9.shape == (1, T, 9) and u9[0, 0, 7] == F(-1.5) and u9[0, 0, 8] == F(-1.5)
    end = q[7:] + (u9[0, :, 7:].astype(np.float64) * dt).sum(axis=0)
    assert np.abs(end).max() <= 1e-6 and (u9[0, -1, 7:] == 0.0).all()
    assert (u9[:, :, :7] == u[:1, :, :7]).all()
    with pytest.raises(ValueError, match="joint_go_to"):
        priors.joint_go_to(q, tgt7[:5], T, dt, u_max)


# ------------------------------------------------------------------ 5. the config key
def test_panda_prior_samples_config_key():
    from m3p2i_aip_amd import compat
    assert compat.make_config("config_panda").panda_prior_samples is None
    cfg = compat.make_config("config_panda", ["panda_prior_samples={controller: hold, n: 4}"])
    assert cfg.panda_prior_samples == dict(controller="hold", n=4) and compat.check_panda_prior_samples(cfg) == ("hold", 4, None)
    seqs, idx = compat.panda_prior_sequences(cfg, np.zeros(9))
    assert seqs.shape == (4, 12, 9) and not seqs.any() and idx == compat.prior_sample_indices(200, 4, False) == [0, 1, 2, 3]
    tgt = [0.0, -0.5, 0.0, -2.0, 0.0, 1.5, 0.7]
    cfg = compat.make_config("config_panda", ["multi_modal=true", "panda_prior_samples={controller: joint_go_to, n: 3, q: %s}" % tgt])
    assert compat.check_panda_prior_samples(cfg) == ("joint_go_to", 3, tgt)
    seqs, idx = compat.panda_prior_sequences(cfg, np.zeros(9))
    assert seqs.shape == (3, 12, 9) and idx == [1, 2, 101]                                  # never 0, K / 2 or K - 1
    want = priors.joint_go_to(np.zeros(9), tgt, 12, 0.01, [2.0] * 7 + [1.5] * 2, [1.0, 2 / 3, 1 / 3])
    assert seqs.tobytes() == want.tobytes() and seqs[:, 0, 1].tolist() == [F(-2.0), F(-4 / 3), F(-2 / 3)]
    for bad in ("panda_prior_samples={controller: go_to}", "panda_prior_samples={n: 4}", "panda_prior_samples={controller: hold, m: 1}",
                "panda_prior_samples={controller: hold, n: 0}", "panda_prior_samples={controller: hold, n: 31}",
                "panda_prior_samples={controller: hold, q: [0, 0, 0, 0, 0, 0, 0]}", "panda_prior_samples={controller: joint_go_to}",
                "panda_prior_samples={controller: joint_go_to, q: [0, 0, 0]}"):
        with pytest.raises(ValueError, match="panda_prior_samples"):
            compat.make_config("config_panda", ["mppi.num_samples=64", bad])
    with pytest.raises(ValueError, match="panda_prior_samples: panda_env only"):
        compat.make_config("config_point", ["panda_prior_samples={controller: hold}"])
    with pytest.raises(ValueError, match="prior_samples: point_env only"):                  # (the point key keeps refusing the arm)
        compat.make_config("config_panda", ["prior_samples={controller: go_to}"])
    # the lockstep episodes refuse the key, with and without the run-time section
    from m3p2i_aip_amd import episodes
    for rt in (False, True):
        with pytest.raises(ValueError, match="run_panda_episodes: episode 0: `panda_prior_samples`.*m3_set_panda_prior_samples"):
            episodes.run_panda_episodes([("config_panda", ["panda_prior_samples={controller: hold}"], None)], panda_runtime=rt)


# ------------------------------------------------------------------ 6. the planner's Python-side rules
class _Engine:
    def __init__(self):
        self.calls = []

    def set_panda_prior_samples(self, seqs=None, indices=None):
        self.calls.append(None if seqs is None else (np.asarray(seqs).shape, list(indices)))

    def set_prior_samples(self, seqs=None, indices=None):
        raise AssertionError("the point entry point on a panda planner")


def _planner(mm=False, env="panda_env", world_size=1, grip="none"):
    import torch
    from m3p2i_aip_amd import planner
    p = object.__new__(planner.MPPI)
    p.env_type, p.K, p.K_local, p.k_offset, p.T, p.nu = env, 8, 8, 0, 4, 9
    p.multi_modal, p.mppi_mode, p.world_size, p.collective, p.device = mm, "halton-spline", world_size, None, "cpu"
    p.u_max, p.u_min = torch.tensor([2.0] * 7 + [1.5] * 2), torch.tensor([-2.0] * 7 + [-1.5] * 2)
    p._engine, p._fused, p._sim, p._bound_sim = _Engine(), True, None, None
    p.gripper_command = grip
    return p


def test_planner_default_indices_and_refusals():
    import torch
    from m3p2i_aip_amd import planner
    seqs = np.full((2, 4, 9), 5.0, F)
    p = _planner()
    assert not p.has_prior_samples
    p.set_panda_prior_samples(seqs)
    assert p._engine.calls == [((2, 4, 9), [0, 1])] and p.has_prior_samples
    # the step path writes the clamped rows (the gripper override comes behind it: _assemble_torch)
    out = p._write_priors(torch.zeros(8, 4, 9), torch.arange(8))
    assert (out[:2, :, :7] == 2.0).all() and (out[:2, :, 7:] == 1.5).all() and (out[2:] == 0.0).all()
    with pytest.raises(ValueError, match=r"planner 0 has prior samples \(set_panda_prior_samples\)"):
        planner.command_batch([p], [np.zeros(18, F)])
    with pytest.raises(ValueError, match=r"planner 0 has prior samples \(set_panda_prior_samples\)"):
        planner.command_batch([p], [np.zeros(18, F)], panda_runtime=True, point_priors=True)
    with pytest.raises(ValueError, match="point_env only"):                                 # (the pinned refusal stays)
        p.set_prior_samples(seqs)
    p.set_panda_prior_samples(None)
    assert p._engine.calls[-1] is None and not p.has_prior_samples
    assert (p._write_priors(torch.zeros(8, 4, 9), torch.arange(8)) == 0.0).all()
    q = _planner(mm=True)
    for mode in ("halton-spline", "simple"):
        q.mppi_mode = mode
        with pytest.raises(ValueError, match="set_panda_prior_samples: a multi-modal planner needs indices"):
            q.set_panda_prior_samples(seqs)
    assert q._engine.calls == []
    q.set_panda_prior_samples(seqs, [1, 5])
    assert q._engine.calls == [((2, 4, 9), [1, 5])]
    with pytest.raises(ValueError, match="set_panda_prior_samples: panda_env only"):
        _planner(env="point_env").set_panda_prior_samples(seqs)
    with pytest.raises(ValueError, match="set_panda_prior_samples: unsharded"):
        _planner(world_size=2).set_panda_prior_samples(seqs)


def test_the_step_path_clamps_then_overrides_the_gripper_in_the_kernels_order():
    """_assemble_torch of a panda planner with priors: clamp(seqs), then the gripper command on columns 7 and 8"""
    import torch
    src = open(os.path.join(ROOT, "m3p2i_aip_amd", "planner.py")).read()
    body = src[src.index("def _assemble_torch"):src.index("def set_prior_samples")]
    for part in body.split("return act")[:2]:                  # (the simple branch and the halton-spline branch)
        assert 0 < part.rindex("self._write_priors(act, ks)") < part.rindex("act[:, :, 7:] =")
    p = _planner(grip="close")
    p.set_panda_prior_samples(np.full((1, 4, 9), 5.0, F), [3])
    act = p._write_priors(torch.zeros(8, 4, 9), torch.arange(8))
    act[:, :, 7:] = -1.5                                        # (what _assemble_torch does next)
    assert (act[3, :, :7] == 2.0).all() and (act[3, :, 7:] == -1.5).all()


# ------------------------------------------------------------------ 7. symbols
def test_the_entry_points_exist_with_their_prototypes():
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    assert "#define M3_ABI_VERSION 4" in hdr and "#define M3_MAX_PRIOR_SAMPLES 256" in hdr
    bound = {s[0]: (s[1], list(s[2])) for s in L.SYMBOLS}
    IP = C.POINTER(C.c_int)
    assert bound["m3_set_panda_prior_samples"] == (C.c_int, [L._H, C.c_void_p, IP, C.c_int])
    assert bound["m3_set_panda_prior_samples_device"] == (C.c_int, [L._H, C.c_void_p, IP, C.c_int])
    assert bound["m3_panda_prior_samples_set"] == (C.c_int, [L._H])
    assert bound["m3_get_panda_prior_sample"] == (C.c_int, [L._H, C.c_int, IP, L._FP])
    assert bound["m3_panda_prior_samples_used"] == (C.c_int, [L._H])
    assert re.search(r"^int m3_set_panda_prior_samples\(m3_handle\* h, const float\* seqs /\* \[n\]\[T\]\[9\] \*/, const int\* sample_idx, int n\);", hdr, re.M)
    assert re.search(r"^int m3_set_panda_prior_samples_device\(m3_handle\* h, const float\* seqs_dev, const int\* sample_idx, int n\);", hdr, re.M)
    assert re.search(r"^int m3_panda_prior_samples_set\(const m3_handle\* h\);", hdr, re.M)
    assert re.search(r"^int m3_get_panda_prior_sample\(const m3_handle\* h, int j, int\* sample_idx, float\* seq\);", hdr, re.M)
    assert re.search(r"^int m3_panda_prior_samples_used\(m3_handle\* h\);", hdr, re.M)
    lib = L.load()
    k = C.c_int()
    # (no handle can be created without a device -- the handle's answers are checked in tests/test_panda_prior_samples_gpu.py)
    assert lib.m3_set_panda_prior_samples(None, None, None, 0) == -1 and lib.m3_set_panda_prior_samples_device(None, None, None, 0) == -1
    assert lib.m3_panda_prior_samples_set(None) == -1 and lib.m3_panda_prior_samples_used(None) == -1
    assert lib.m3_get_panda_prior_sample(None, 0, C.byref(k), None) == -1


def test_the_new_kernels_are_one_translation_unit_of_the_build():
    from m3p2i_aip_amd import build
    assert "rollout_panda_priors.hip" in build.SOURCES
    assert build.PER_SOURCE["rollout_panda_priors.hip"] == build.PER_SOURCE["rollout_panda_rows.hip"]   # (its twin's flags)


# ------------------------------------------------------------------ 8. the variant decision with priors_on, natively
def test_the_variant_decision_with_prior_samples(tmp_path):
    out = str(tmp_path / "panda_variant_priors_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2",
                           os.path.join(ROOT, "tests", "native", "panda_variant_priors_host.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    m = re.fullmatch(r"(\d+) checks, 0 failures\n", r.stdout)
    # 288 inputs; per input 5 + 6 without priors, 7 + 2 + 3 + 6 with: 29
    assert m and int(m.group(1)) >= 288 * 29, r.stdout
