"""The lean instances of point_substep (m3p2i_aip_amd/csrc/planar_dyn.hpp: no pair / robot-box / + robot-dyn-obs) run their
contact and friction rows for ALL lanes and merge by a select on the row's per-lane flag.  What that form could get wrong --
and what a world whose rows are all on, or all off, does not show -- is a lane whose flag CHANGES: the robot-box contact
switching on and off within one sequence of calls, with the box at rest or still sliding when it does.

The host build of the header (tests/native/planar_substep_host.cpp, g++) runs scripted worlds of that kind through each
lean instance directly, in lockstep with the oracle (oracle/_build/libm3oracle.so), and every state, pending force and
contact impulse must be the oracle's bit for bit after every step.  Each sequence runs six times: with the leanest
instance that covers the lane's broad-phase mask and with a wider lean instance forced (rows that exist in the code but
are off for the lane), each as a one-lane wavefront and as one lane of a wavefront whose other lanes have every row --
there the wave-uniform pass version has all rows and only the per-lane selects keep this lane's state.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.native_flags import host_flags
from tests.test_device_dynamics_on_host import HOST_FLAGS, fma_flag

HERE = os.path.dirname(os.path.abspath(__file__))
G_RB, G_RD = 1, 2
STEPS = 70
DT, SUBSTEPS, ITERS = 0.05, 2, 6
# what is compared: everything the rollout's path writes (the robot's c, s, w do not exist on the device; of the contact
# forces it forms the dyn-obs' only), as in tests/test_device_dynamics_on_host.py
COLS = [c for c in range(25) if c not in (2, 3, 6)] + [29, 30]


@pytest.fixture(scope="module")
def substep_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("planar_substep") / "libplanar_substep_host.so")
    subprocess.check_call(["g++"] + host_flags(HOST_FLAGS) + fma_flag() + ["-I" + os.path.join(HERE, "native", "shim"),
                           os.path.join(HERE, "native", "planar_substep_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.pss_step.argtypes = [C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p]
    lib.pss_step.restype = C.c_int
    return lib


def scene(O):
    sc = O.default_scene()
    sc.dt, sc.substeps, sc.iters = DT, SUBSTEPS, ITERS
    return sc


def moving(w, base):
    """The device's (and the spec's) rest test: a velocity below the smallest normal number is zero."""
    return bool(((w[base + 4:base + 7].view(np.uint32) & 0x7f800000) != 0).any())


class Script:
    """A world and the controller that drives its robot, from the ORACLE's state: approach a target box until it has been
    pushed for `push` steps, back off until `clear` away from it, turn to the next target -- so the robot-box row comes
    on, goes off while the box still slides, stays off while it comes to rest, and comes on again."""

    def __init__(self, O, kind, seed):
        rng = np.random.default_rng(1000 * (1 + ["push_release", "between"].index(kind)) + seed)
        self.rng, self.O, self.kind = rng, O, kind
        w = O.init_world(1)[0]
        yaw = rng.uniform(-np.pi, np.pi, 2)
        if kind == "push_release":
            # the box in the open, pushed towards -y (away from the obstacle at (2, 2) and every wall); the dyn-obs far off
            b = np.array([rng.uniform(-1.5, -0.5), rng.uniform(-0.3, 0.7)])
            a = np.deg2rad(rng.uniform(230.0, 310.0))
            r = b - 0.8 * np.array([np.cos(a), np.sin(a)])
            d = np.array([2.8, -0.5])
            self.targets = [O.W_B]
        else:
            # the robot between the box (pushed towards +x) and the dyn-obs (towards -x), touching them in turn
            b = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-1.2, -0.8)])
            d = b + np.array([-1.45, rng.uniform(-0.05, 0.05)])
            r = b + np.array([-0.72, rng.uniform(-0.05, 0.05)])
            self.targets = [O.W_B, O.W_D]
            if seed % 2:    # (a dyn-obs that already drifts and turns: its friction row runs while its contact row is off)
                w[O.W_D + 4:O.W_D + 7] = (rng.uniform(-0.3, 0.0), rng.uniform(-0.1, 0.1), rng.uniform(-1.0, 1.0))
        w[0:2] = r
        w[O.W_B:O.W_B + 4] = (b[0], b[1], np.cos(yaw[0]), np.sin(yaw[0]))
        w[O.W_D:O.W_D + 4] = (d[0], d[1], np.cos(yaw[1]), np.sin(yaw[1]))
        self.world0 = w.astype(np.float32)
        self.phase, self.count, self.target = "in", 0, 0
        self.push, self.clear = int(rng.integers(2, 5)), rng.uniform(0.75, 0.95)
        self.speed = rng.uniform(1.5, 3.0)

    def control(self, w):
        base = self.targets[self.target]
        to = w[base:base + 2].astype(np.float64) - w[0:2].astype(np.float64)
        dist = float(np.hypot(*to))
        to /= dist
        if self.phase == "in":
            if moving(w, base) and dist < 0.5:
                self.count += 1
            if self.count >= self.push:
                self.phase, self.count = "out", 0
        elif dist > self.clear or (self.kind == "between" and dist > 0.6):
            self.phase = "in"
            self.target = (self.target + 1) % len(self.targets)
            base = self.targets[self.target]
            to = w[base:base + 2].astype(np.float64) - w[0:2].astype(np.float64)
            to /= np.hypot(*to)
        u = (self.speed if self.phase == "in" else -self.speed) * to + self.rng.normal(0, 0.15, 2)
        return np.clip(u, -3, 3).astype(np.float32)


CASES = [(kind, seed) for kind in ("push_release", "between") for seed in range(6)]


def oracle_run(O, kind, seed):
    """The oracle's trajectory of a case: worlds before every step (STEPS + 1 rows) and the controls."""
    s = Script(O, kind, seed)
    w = s.world0.copy()[None]
    worlds, us = [w[0].copy()], []
    sc = scene(O)
    for _ in range(STEPS):
        u = s.control(w[0])
        O.step_batch(sc, w, u[None])
        worlds.append(w[0].copy()); us.append(u)
    return np.array(worlds), np.array(us)


def test_the_oracle_agrees_with_itself_on_every_case(oracle):
    """Every case's controls replayed on the oracle with ALL cases stepped as one batch: the same bits as one world at a
    time (the reference these tests compare against is a function of the world and the control alone)."""
    runs = [oracle_run(oracle, kind, seed) for kind, seed in CASES]
    w = np.array([r[0][0] for r in runs])
    sc = scene(oracle)
    for t in range(STEPS):
        oracle.step_batch(sc, w, np.array([r[1][t] for r in runs]))
        for i, r in enumerate(runs):
            assert np.array_equal(w[i].view(np.uint32), r[0][t + 1].view(np.uint32)), (CASES[i], t)


def run_case(O, lib, kind, seed, min_instance, other_lanes):
    """One case on the host build, in lockstep with the oracle; returns per substep (mask, instance, box moves, dyn-obs moves)."""
    worlds, us = oracle_run(O, kind, seed)
    b = worlds[0].copy()
    info = (C.c_int * (2 * SUBSTEPS))()
    seen = []
    for t in range(STEPS):
        before = b.copy()
        rc = lib.pss_step(DT, SUBSTEPS, ITERS, b.ctypes.data, float(us[t][0]), float(us[t][1]), min_instance, other_lanes, info)
        assert rc == 0, f"{kind} seed {seed} step {t}: the world left the lean instances' range (mask {info[0]} / {info[2]})"
        a = worlds[t + 1]
        neq = a[COLS].view(np.uint32) != b[COLS].view(np.uint32)
        if neq.any():
            c = COLS[int(np.argwhere(neq)[0][0])]
            raise AssertionError(f"{kind} seed {seed} min_instance {min_instance} other_lanes {other_lanes} step {t} column {c}: "
                                 f"oracle {a[c]!r} device-source {b[c]!r} ({int(neq.sum())} values differ)")
        for sub in range(SUBSTEPS):
            seen.append((info[2 * sub], info[2 * sub + 1], moving(before, O.W_B), moving(before, O.W_D)))
    return seen


@pytest.mark.parametrize("other_lanes", [0, 1], ids=["one_lane_wave", "lane_of_a_wave_with_every_row"])
@pytest.mark.parametrize("min_instance", [0, 1, 2], ids=["leanest", "at_least_robot_box", "robot_box_and_dyn_obs"])
@pytest.mark.parametrize("kind,seed", CASES)
def test_lean_instances_equal_the_oracle_while_rows_switch(oracle, substep_lib, kind, seed, min_instance, other_lanes):
    seen = run_case(oracle, substep_lib, kind, seed, min_instance, other_lanes)
    rb = [bool(m & G_RB) for m, _, _, _ in seen]
    switches = sum(1 for x, y in zip(rb, rb[1:]) if x != y)
    assert switches >= 3, "the robot-box row must come on, go off and come on again within the sequence"
    # (step-start states: the box at rest / moving) x (the robot-box pair in / out of range), all four in one sequence
    combos = {(bool(m & G_RB), mb) for m, _, mb, _ in seen}
    assert combos == {(False, False), (False, True), (True, False), (True, True)}, combos
    if kind == "between":
        rd = [bool(m & G_RD) for m, _, _, _ in seen]
        assert sum(1 for x, y in zip(rd, rd[1:]) if x != y) >= 2, "the robot-dyn-obs row must switch as well"
        if seed % 2:
            assert any(md and not (m & G_RD) for m, _, _, md in seen), "the dyn-obs must move while out of the robot's range"


def test_all_three_lean_instances_are_hit(oracle, substep_lib):
    used = set()
    for kind, seed in CASES:
        used |= {inst for _, inst, _, _ in run_case(oracle, substep_lib, kind, seed, 0, 0)}
    assert used == {0, 1, 2}
