"""Batched closed-loop episodes (m3_episodes_*) without a GPU: the episode structs of include/m3p2i_hip.h
against their ctypes mirror, the per-lane decisions of k_episodes_pre / k_episodes_post (csrc/episode_lane.hpp, built for
the host) against the Python expressions of tools/closed_loop.run on their edge cases, and the Fisher exact test of
tests/test_behaviour_band_n60_gpu.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from m3p2i_aip_amd import _lib as L  # noqa: E402


@pytest.fixture(scope="module")
def lane(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("episode_lane") / "libepisode_lane_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                           os.path.join(HERE, "native", "episode_lane_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    for name, args in (("ep_walk_forth_h", [C.c_int]), ("ep_success_h", [C.c_int] + [C.c_float] * 4),
                       ("ep_collision_h", [C.c_float] * 2), ("ep_gate_h", [C.c_int, C.c_int])):
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = C.c_int
    lib.ep_norm2_h.argtypes = [C.c_float, C.c_float]
    lib.ep_norm2_h.restype = C.c_float
    lib.ep_layout_h.argtypes = [C.c_void_p]
    return lib


def test_episode_structs_match_the_ctypes_layout(lane):
    out = (C.c_long * 17)()
    lane.ep_layout_h(out)
    S, T = L.EpisodeSpec, L.EpisodeStatus
    assert list(out[:6]) == [C.sizeof(S), S.task.offset, S.goal.offset, S.dyn_phase.offset, S.suction.offset, S.kp_suction.offset]
    assert list(out[6:11]) == [C.sizeof(T), T.done_tick.offset, T.success.offset, T.collision_ticks.offset, T.final_pos.offset]
    assert list(out[11:14]) == [L.SUCTION_OFF, L.SUCTION_ON, L.SUCTION_PULL_PREFERENCE] == list(out[14:17])


def test_new_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    names = [s[0] for s in L.SYMBOLS if s[0].startswith("m3_episodes_")]
    assert sorted(names) == sorted(["m3_episodes_create", "m3_episodes_tick", "m3_episodes_begin", "m3_episodes_end",
                                    "m3_episodes_status", "m3_episodes_ticks_done", "m3_episodes_running",
                                    "m3_episodes_destroy", "m3_episodes_last_error"])
    for n in names:
        assert n + "(" in hdr, n


@pytest.mark.parametrize("phase", [0, 24, 25, 26, 74, 75, 76, 99, 100, 124, 125, 126, 175])
@pytest.mark.parametrize("tick", [0, 1, 49, 50, 51, 799])
def test_dyn_obs_walk_direction(lane, tick, phase):
    i, period = tick + phase, 100
    forth = period / 4 < i % period < period / 4 * 3        # isaacgym_wrapper.update_dyn_obs
    assert bool(lane.ep_walk_forth_h(i)) == forth


def _torch_success(task, p, goal):
    """PLANNER_SIMPLE.check_task_success on an f32 position and the goal tensor the task planner makes."""
    pos = torch.tensor(p, dtype=torch.float32)
    g = torch.tensor(goal)
    d = torch.norm(pos - g)
    return bool(d < 0.1) if task == 0 else bool(d <= 0.1)


def _f(x):
    return float(np.float32(x))


def test_success_test_on_its_edges(lane):
    f01 = _f(0.1)
    nxt, prv = float(np.nextafter(np.float32(f01), np.float32(1))), float(np.nextafter(np.float32(f01), np.float32(0)))
    cases = []
    for goal in ([-3, 3], [-3.75, -3.75], [0.0, 0.0], [2.0, -2.0]):
        for task in (0, 1, 2, 3):
            for off in (f01, nxt, prv, 0.0, -f01, 0.05, _f(0.0707107), _f(0.07071068)):
                for dy in (0.0, off, -off, _f(0.06), _f(0.08)):
                    cases.append((task, (_f(goal[0] + off), _f(goal[1] + dy)), goal))
    cases.append((1, (f01, 0.0), [0.0, 0.0]))      # distance exactly 0.1f: push succeeds, navigation does not
    cases.append((0, (f01, 0.0), [0.0, 0.0]))
    agree = 0
    for task, p, goal in cases:
        ours = bool(lane.ep_success_h(task, p[0], p[1], float(goal[0]), float(goal[1])))
        assert ours == _torch_success(task, p, goal), (task, p, goal)
        agree += 1
    assert lane.ep_success_h(1, f01, 0.0, 0.0, 0.0) == 1 and lane.ep_success_h(0, f01, 0.0, 0.0, 0.0) == 0
    assert lane.ep_success_h(4, 0.0, 0.0, 0.0, 0.0) == 0      # (a panda task never succeeds here)
    assert agree == len(cases)


def test_norm_rounds_each_square_then_the_sum(lane):
    """The device's torch.norm of a 2-vector: x*x and y*y rounded to f32, their f32 sum, a correctly rounded sqrt -- no fma
    (which torch's CPU kernel may use: the device's own decisions are checked against the serial loop on the GPU,
    tests/test_episodes_gpu.py)."""
    rng = np.random.default_rng(3)
    v = rng.uniform(-0.2, 0.2, (4000, 2)).astype(np.float32)
    ours = np.array([lane.ep_norm2_h(float(a), float(b)) for a, b in v], np.float32)
    ref = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1])      # numpy f32: each product and the sum rounded
    assert ref.dtype == np.float32 and np.array_equal(ours, ref)


def test_collision_test_compares_the_f32_sum_in_double(lane):
    f01 = _f(0.1)
    cases = [(f01, 0.0), (0.0, -f01), (_f(0.05), _f(0.05)), (_f(0.06), _f(0.04)), (0.0, 0.0), (-0.0, 0.0),
             (float(np.nextafter(np.float32(f01), np.float32(0))), 0.0), (_f(1e-9), f01), (-3.0, 2.0), (_f(0.03), _f(0.07))]
    for fx, fy in cases:
        f = torch.tensor([fx, fy], dtype=torch.float32)
        ref = float(f[0].abs() + f[1].abs()) > 0.1               # closed_loop.run
        assert bool(lane.ep_collision_h(fx, fy)) == ref, (fx, fy)
    assert lane.ep_collision_h(f01, 0.0) == 1                     # 0.1f > 0.1 in double: a collision


def test_gate_is_the_previous_commands_pull_preference(lane):
    """closed_loop.run: tamp.run_tamp reads get_pull_preference() BEFORE its command, the world applies suction with it AFTER
    the command; so the gate of tick i is the preference the command of tick i - 1 left (0 at tick 0)."""
    prefs = [0, 1, 1, 0, 1, 0, 0, 1]        # m3_info.pull_preference after the command of tick i
    serial, batched, info = [], [], 0
    for i, p in enumerate(prefs):
        serial.append(int(bool(info)))     # suction_active = get_pull_preference() (before command i) ... applied after it
        batched.append(lane.ep_gate_h(L.SUCTION_PULL_PREFERENCE, info))   # k_episodes_pre snapshots before the command
        info = p                           # command i
    assert serial == batched == [0, 0, 1, 1, 0, 1, 0, 0]
    assert [lane.ep_gate_h(L.SUCTION_ON, p) for p in (0, 1)] == [1, 1]
    assert [lane.ep_gate_h(L.SUCTION_OFF, p) for p in (0, 1)] == [0, 0]


def test_fisher_exact_one_sided():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import band_stats
    f = band_stats.fisher_one_sided
    # the committed N = 60 numbers against the logged counts: corner2_push 8/60 successes vs 3/20, 1/60 collided vs 0/20
    assert f(8, 52, 3, 17, "less") > 0.01 and f(1, 59, 0, 20, "greater") > 0.01
    assert f(0, 60, 20, 0, "less") < 1e-10 and f(30, 30, 0, 20, "greater") < 0.01
    try:
        from scipy.stats import fisher_exact
    except Exception:
        fisher_exact = None
    for t in [(8, 52, 3, 17), (1, 59, 0, 20), (50, 10, 45, 15), (40, 20, 11, 9), (60, 0, 20, 0), (0, 60, 0, 60), (3, 57, 3, 57)]:
        for alt in ("less", "greater"):
            p = f(*t, alt)
            assert 0.0 <= p <= 1.0 + 1e-12
            if fisher_exact is not None:
                assert abs(p - fisher_exact([[t[0], t[1]], [t[2], t[3]]], alternative=alt)[1]) < 1e-9, (t, alt)
