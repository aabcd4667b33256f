"""Prior controllers on the device (m3_set_prior_controller), the parts that need no GPU: the host build
of csrc/prior_controllers.hpp (tests/native/prior_controllers_host.cpp) against priors.go_to / priors.push_behind in float64
within the bound derived in tests/prior_controllers_fixture.py, the same program under -fsanitize=address,undefined, the symbols
and the ABI, the `device: true` config key and the planner's Python-side rules on a stub engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from m3p2i_aip_amd import _lib as L
from tests import prior_controllers_fixture as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def host_prog(tmp_path_factory):
    return PC.build(tmp_path_factory.mktemp("prior_controllers"))


# ------------------------------------------------------------------ 1. the header against priors.py
def test_the_replay_is_priors_py():
    """the fixture's float64 restatement (which also returns the switch margins) gives priors.py's float32 output exactly"""
    for c in PC.all_cases():
        np.testing.assert_array_equal(PC.replay(c)[0].astype(F).view(np.uint32), PC.reference(c).view(np.uint32))


def test_the_switch_guard_holds_on_every_input():
    """the switch is a discontinuity: the float64 reference stays GUARD away from the threshold at every test it makes, and the
    derived error of the binary32 side at such a test is below GUARD -- both sides take the same decisions.  No case is skipped."""
    worst, tests, switches = np.inf, 0, 0
    for c in PC.all_cases():
        if c["kind"] != PC.PUSH_BEHIND:
            continue
        _, margins, sw = PC.replay(c)
        assert margins, c
        worst = min(worst, min(margins))
        tests += len(margins)
        switches += int((sw[:, 0]).sum()) + int((sw[:, 1:] & ~sw[:, :-1]).sum())
        assert PC.bounds(c)[1] < PC.GUARD, (PC.bounds(c), c)
    print(f"switch guard: {tests} tests, {switches} switches, smallest margin {worst:.3e} (guard {PC.GUARD:g}), "
          f"largest decision error bound {max(PC.bounds(c)[1] for c in PC.all_cases()):.3e}")
    assert worst >= PC.GUARD
    assert switches > 0
    # the inputs named for it: a switch mid-horizon and one at step 0
    mid = PC.replay(PC.case(PC.PUSH_BEHIND, 30, (2.0, 2.0), *PC.INPUTS[3]))[2]
    assert not mid[0, 0] and mid[0, -1]
    assert PC.replay(PC.case(PC.PUSH_BEHIND, 12, (2.0, 2.0), *PC.INPUTS[4]))[2][:, 0].all()


def test_host_build_equals_priors_py_within_the_derived_bound(host_prog):
    """Measured on the host build (g++, x86-64): max |binary32 - float64| 1.40e-6 (23.5 eps) on the five inputs the feature
    was specified with -- what a numpy float32 emulation had given -- and 3.93e-6 (66 eps) over all 56 cases (push_behind at
    T = 30 with the robot starting at the goal), against derived bounds of 1.3e-4 (go_to, T = 12) to 5.7e-4 (push_behind,
    T = 30).  The bound is loose by two orders: it lets the stand-off point's error and every step's rounding add up linearly
    and divides the sum by dt."""
    cases = PC.all_cases()
    got = PC.run(host_prog, cases)
    worst = 0.0
    for c, g in zip(cases, got):
        ref = PC.reference(c)
        assert g.shape == ref.shape and np.isfinite(g).all()
        err = float(np.abs(g.astype(np.float64) - ref.astype(np.float64)).max())
        bound = PC.bounds(c)[0]
        worst = max(worst, err)
        print(f"kind {c['kind']} T {c['T']} u_max {c['u_max']} robot {c['robot']} box {c['box']} goal {c['goal']}: "
              f"max |f32 - f64| {err:.3e} ({err / PC.EPS:.1f} eps), bound {bound:.3e}")
        assert err <= bound, (err, bound, c)
    print(f"measured maximum over {len(cases)} cases: {worst:.3e} ({worst / PC.EPS:.1f} eps)")
    assert worst > 0.0      # (binary32 is not float64: a comparison that sees nothing would give 0)


def test_host_program_under_the_sanitizers(tmp_path):
    prog = PC.build(tmp_path, extra=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    cases = PC.all_cases()
    got = PC.run(prog, cases)
    plain = PC.run(PC.build(tmp_path), cases)
    for a, b in zip(got, plain):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------ 2. symbols, defines, null handles
def test_the_entry_points_are_declared_and_bound():
    main = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    ext = open(os.path.join(ROOT, "include", "m3p2i_hip_ext.h")).read()
    assert "#define M3_ABI_VERSION 4" in main
    for define, value in (("M3_PRIOR_CONTROLLER_GO_TO", 1), ("M3_PRIOR_CONTROLLER_PUSH_BEHIND", 2), ("M3_MAX_PRIOR_CONTROLLER_SEQS", 16)):
        assert re.search(rf"^#define {define} {value}$", ext, re.M), define
    assert (L.PRIOR_CONTROLLER_GO_TO, L.PRIOR_CONTROLLER_PUSH_BEHIND, L.MAX_PRIOR_CONTROLLER_SEQS) == (1, 2, 16)
    assert L.PRIOR_CONTROLLER_KINDS == dict(go_to=1, push_behind=2)
    assert C.sizeof(L.PriorController) == 4 * (2 + 16 + 2)
    assert [f[0] for f in L.PriorController._fields_] == ["kind", "n", "speed", "standoff", "reach"]
    assert re.search(r"int   kind;.*\n\s+int   n;.*\n\s+float speed\[16\];.*\n\s+float standoff;\n\s+float reach;\n\} m3_prior_controller;", ext)
    for proto in (r"void m3_default_prior_controller\(m3_prior_controller\* pc, int kind, int n\);",
                  r"int m3_set_prior_controller\(m3_handle\* h, const m3_prior_controller\* pc, const int\* sample_idx\);",
                  r"int m3_get_prior_controller\(const m3_handle\* h, m3_prior_controller\* out\);",
                  r"int m3_prior_controller_fill\(m3_handle\* h\);",
                  r"int m3_prior_table\(const m3_handle\* h, const float\*\* tab_dev, int\* n\);"):
        assert re.search("^" + proto, ext, re.M), proto
    names = {"m3_default_prior_controller", "m3_set_prior_controller", "m3_get_prior_controller", "m3_prior_controller_fill",
             "m3_prior_table"}
    assert names <= {s[0] for s in L.SYMBOLS_EXT} and not names & {s[0] for s in L.SYMBOLS}
    lib = L.load()
    # (no handle can be created without a device -- the handle's answers are checked in tests/test_prior_controllers_gpu.py)
    pc = L.PriorController()
    for kind, n in ((1, 4), (2, 16), (2, 1)):
        lib.m3_default_prior_controller(C.byref(pc), kind, n)
        assert (pc.kind, pc.n) == (kind, n) and pc.standoff == F(0.45) and pc.reach == F(0.05)
        assert [pc.speed[j] for j in range(16)] == [float(F(1.0) - F(j) / F(n)) if j < n else 0.0 for j in range(16)]
    lib.m3_default_prior_controller(None, 1, 4)
    assert lib.m3_set_prior_controller(None, C.byref(pc), None) == -1 and lib.m3_set_prior_controller(None, None, None) == -1
    assert lib.m3_get_prior_controller(None, C.byref(pc)) == -1 and lib.m3_prior_controller_fill(None) == -1
    p, n = C.c_void_p(), C.c_int()
    assert lib.m3_prior_table(None, C.byref(p), C.byref(n)) == -1


# ------------------------------------------------------------------ 3. the config key
def test_the_device_flag_of_the_config_key():
    from m3p2i_aip_amd import compat
    cfg = compat.make_config("config_point", ["task=push", "prior_samples={controller: push_behind, n: 4}"])
    assert compat.check_prior_samples(cfg) == ("push_behind", 4) and compat.prior_samples_on_device(cfg) is False
    assert compat.prior_samples_on_device(compat.make_config("config_point")) is False
    cfg = compat.make_config("config_point", ["task=push", "prior_samples={controller: push_behind, n: 4, device: true}"])
    assert cfg.prior_samples == dict(controller="push_behind", n=4, device=True)
    assert compat.check_prior_samples(cfg) == ("push_behind", 4) and compat.prior_samples_on_device(cfg) is True
    cfg = compat.make_config("config_point", ["prior_samples={controller: go_to, device: false}"])
    assert compat.check_prior_samples(cfg) == ("go_to", 4) and compat.prior_samples_on_device(cfg) is False
    for bad in ("prior_samples={controller: go_to, device: 2}", "prior_samples={controller: go_to, n: 17, device: true}"):
        with pytest.raises(ValueError, match="prior_samples: device"):
            compat.make_config("config_point", ["mppi.num_samples=200", bad])
    compat.make_config("config_point", ["mppi.num_samples=200", "prior_samples={controller: go_to, n: 17}"])   # the host's limit stays


# ------------------------------------------------------------------ 4. the planner's Python-side rules
class _Engine:
    """records the calls; prior_table() returns what a fill would have written"""

    def __init__(self):
        self.calls = []
        self.table = None

    def set_prior_samples(self, seqs=None, indices=None):
        self.calls.append(("samples", None if seqs is None else list(indices)))

    def set_prior_controller(self, kind=None, n=4, indices=None, speeds=None, standoff=None, reach=None):
        self.calls.append(("controller", kind) if kind is None else ("controller", kind, n, list(indices), speeds, standoff, reach))

    def prior_controller_fill(self):
        self.calls.append(("fill",))

    def prior_table(self):
        self.calls.append(("table",))
        return self.table


def _planner(mm=False, env="point_env", world_size=1):
    import torch
    from m3p2i_aip_amd import planner
    p = object.__new__(planner.MPPI)
    p.env_type, p.K, p.K_local, p.k_offset, p.T, p.nu = env, 8, 8, 0, 4, 2
    p.multi_modal, p.mppi_mode, p.world_size, p.collective, p.device = mm, "halton-spline", world_size, None, "cpu"
    p.u_max, p.u_min = torch.tensor([3.0, 3.0]), torch.tensor([-3.0, -3.0])
    p._engine, p._fused, p._sim, p._bound_sim = _Engine(), True, None, None
    p._push_objective = lambda: p._engine.calls.append(("objective",))
    p._bind_world = lambda: p._engine.calls.append(("bind",))
    return p


def test_planner_rules_and_the_step_path_reads_the_filled_table():
    import torch
    from m3p2i_aip_amd import planner
    p = _planner()
    p.set_prior_controller("go_to", 2)
    assert p._engine.calls == [("controller", "go_to", 2, [0, 1], None, None, None)] and p.has_prior_samples
    # the step path: objective and world as the fused path pushes them, the fill, then the rows of the table, clamped
    p._engine.table = torch.full((2, 4, 2), 5.0)
    out = p._write_priors(torch.zeros(8, 4, 2), torch.arange(8))
    assert p._engine.calls[1:] == [("objective",), ("bind",), ("fill",), ("table",)]
    assert (out[:2] == 3.0).all() and (out[2:] == 0.0).all()
    with pytest.raises(ValueError, match="prior samples"):
        planner.command_batch([p], [np.zeros(4, F)])
    # against set_prior_samples the last call wins, both ways
    p.set_prior_samples(np.full((1, 4, 2), -5.0, F), [6])
    out = p._write_priors(torch.zeros(8, 4, 2), torch.arange(8))
    assert (out[6] == -3.0).all() and (out[:6] == 0.0).all() and p._engine.calls[-1] == ("samples", [6])
    p.set_prior_controller("push_behind", 3, indices=[1, 2, 5], speeds=[1.0, 0.5, 0.25], standoff=0.6, reach=0.1)
    assert p._engine.calls[-1] == ("controller", "push_behind", 3, [1, 2, 5], [1.0, 0.5, 0.25], 0.6, 0.1)
    p._engine.table = torch.full((3, 4, 2), 1.5)
    out = p._write_priors(torch.zeros(8, 4, 2), torch.arange(8))
    assert (out[[1, 2, 5]] == 1.5).all() and (out[[0, 3, 4, 6, 7]] == 0.0).all()
    p.set_prior_controller(None)
    assert p._engine.calls[-1] == ("controller", None) and not p.has_prior_samples
    assert (p._write_priors(torch.zeros(8, 4, 2), torch.arange(8)) == 0.0).all()
    # the rules of set_prior_samples
    q = _planner(mm=True)
    with pytest.raises(ValueError, match="needs indices"):
        q.set_prior_controller("go_to", 2)
    with pytest.raises(ValueError, match="kind is one of"):
        q.set_prior_controller("straight", 2, indices=[1, 5])
    assert q._engine.calls == []
    q.set_prior_controller("go_to", 2, indices=[1, 5])
    assert q._engine.calls == [("controller", "go_to", 2, [1, 5], None, None, None)]
    with pytest.raises(ValueError, match="point_env only"):
        _planner(env="panda_env").set_prior_controller("go_to", 2)
    with pytest.raises(ValueError, match="unsharded"):
        _planner(world_size=2).set_prior_controller("go_to", 2)
