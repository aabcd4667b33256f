"""Batched panda_env episodes (m3_panda_episodes_*) without a GPU: the status struct of include/m3p2i_hip.h
against its ctypes mirror, the per-lane decisions of k_panda_episodes_post (csrc/panda_episode_lane.hpp, built for the
host) against the loops of tools/closed_loop.run written out in Python, the trace row's layout against what closed_loop.run
puts into its `trace` / `full` rows, and the simulator adapter of m3p2i_aip_amd/episodes.py against the wrapper's
env0_link_states_host on PLANNER_AIF_PANDA."""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd import scenes  # noqa: E402

OP_STEP, OP_ZERO, OP_TRACE, OP_FREEZE = 1, 2, 4, 8


@pytest.fixture(scope="module")
def lane(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("panda_episode_lane") / "libpanda_episode_lane_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                           os.path.join(HERE, "native", "panda_episode_lane_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.pe_advance_h.argtypes = [C.POINTER(L.PandaEpisodeStatus)] + [C.c_int] * 4
    lib.pe_advance_h.restype = C.c_int
    lib.pe_target_h.argtypes = [C.c_int, C.POINTER(C.c_float), C.c_int]
    lib.pe_target_h.restype = C.c_float
    lib.pe_layout_h.argtypes = [C.c_void_p]
    return lib


def test_status_struct_and_constants_match_the_ctypes_mirror(lane):
    out = (C.c_long * 21)()
    lane.pe_layout_h(out)
    S = L.PandaEpisodeStatus
    assert list(out[:7]) == [C.sizeof(S), S.phase.offset, S.done_tick.offset, S.success.offset, S.settle_left.offset,
                             S.cubeA.offset, S.cubeB.offset]
    assert list(out[7:10]) == [L.PE_RUNNING, L.PE_SETTLING, L.PE_FROZEN]
    assert list(out[10:15]) == [L.PE_TR_DOF, L.PE_TR_ROOT, L.PE_TR_ACTION, L.PE_TR_HAND, L.PE_TR_CUBE]
    assert out[15] == out[16] == L.PANDA_EPISODE_TRACE_FLOATS
    assert list(out[17:21]) == [OP_STEP, OP_ZERO, OP_TRACE, OP_FREEZE]


def test_new_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    names = [s[0] for s in L.SYMBOLS if s[0].startswith("m3_panda_episodes_")]
    assert sorted(names) == sorted("m3_panda_episodes_" + x for x in (
        "create", "observe", "act", "act_first", "status", "ticks_done", "running", "active", "destroy", "last_error"))
    for n in names:
        assert n + "(" in hdr, n
    assert "#define M3_ABI_VERSION 4" in hdr          # (additive)


def _serial_world_ops(success_tick, ticks, settle_ticks):
    """What tools/closed_loop.run does to its 1-env world, as a list of ("step", tick, zero targets?, trace row?) in order,
    and (ticks reported, success)."""
    ops, success, i = [], False, 0
    for i in range(ticks):
        if success_tick is not None and i == success_tick:      # tamp.task_success: break BEFORE the trace row and the step
            success = True
            break
        ops.append(("step", i, False, True))
    for _ in range(settle_ticks if success else 0):
        ops.append(("step", None, True, False))
    return ops, (i + 1, success)


def _lockstep_world_ops(lane, success_tick, max_ticks, settle_ticks):
    """The same from pe_advance, one call per tick of the set, until the lane is frozen (+ a few ticks more: nothing)."""
    st = L.PandaEpisodeStatus(phase=L.PE_RUNNING, done_tick=-1)
    ops, tick, frozen_at = [], 0, None
    while tick < max_ticks + settle_ticks + 3:
        ended = int(st.phase == L.PE_RUNNING and success_tick is not None and tick == success_tick)
        was = st.phase
        op = lane.pe_advance_h(C.byref(st), ended, tick, max_ticks - 1, settle_ticks)
        if op & OP_STEP:
            ops.append(("step", tick if op & OP_TRACE else None, bool(op & OP_ZERO), bool(op & OP_TRACE)))
        assert bool(op & OP_TRACE) == (was == L.PE_RUNNING and not ended)      # a row per tick the episode steps while running
        assert not (op & OP_TRACE and op & OP_ZERO)
        if op & OP_FREEZE:
            assert frozen_at is None and st.phase == L.PE_FROZEN
            frozen_at = tick
        elif frozen_at is not None:
            assert op == 0                                                    # nothing after the freeze
        tick += 1
    assert st.phase == L.PE_FROZEN and st.settle_left == 0
    return ops, (st.done_tick + 1, bool(st.success)), frozen_at


@pytest.mark.parametrize("settle", [0, 1, 2, 20])
@pytest.mark.parametrize("success_tick", [None, 0, 1, 5, 10, 11, 12])
def test_lane_decisions_equal_the_serial_loops(lane, success_tick, settle):
    max_ticks = 12                       # success ticks 11 (the last tick) and 12 (never reached) included
    serial, rep = _serial_world_ops(success_tick, max_ticks, settle)
    ours, rep2, frozen_at = _lockstep_world_ops(lane, success_tick, max_ticks, settle)
    assert ours == serial and rep2 == rep
    if rep[1]:       # frozen at the tick of its last settle step (settle 0: at the success tick itself, without a step)
        assert frozen_at == success_tick + max(settle - 1, 0)
    else:            # out of ticks: after the step of the last tick, no settling
        assert frozen_at == max_ticks - 1 and rep == (max_ticks, False)


def test_targets_are_plan_row_0_or_the_zero_action(lane):
    plan = (C.c_float * 9)(*[0.25 * (j - 4) for j in range(9)])
    zero = torch.zeros(1, 9)                                  # closed_loop.run's settle action
    for j in range(9):
        assert lane.pe_target_h(OP_STEP | OP_TRACE, plan, j) == plan[j]
        z = lane.pe_target_h(OP_STEP | OP_ZERO, plan, j)
        assert z == float(zero[0, j]) and np.signbit(np.float32(z)) == np.signbit(zero[0, j].numpy())


def test_trace_row_layout_gives_closed_loops_rows():
    """A row as k_panda_episodes_post lays it out, cut as PandaEpisodeSet.reports cuts it, against closed_loop.run's own
    expressions on the tensors the row was made from."""
    rng = np.random.default_rng(5)
    nb, na = scenes.num_bodies("panda_env"), len(scenes.ENVS["panda_env"])
    assert (nb, na) == (17, 7) and L.PE_TR_ACTION - L.PE_TR_ROOT == na * 13
    dof = torch.from_numpy(rng.standard_normal((1, 18)).astype(np.float32))
    root = torch.from_numpy(rng.standard_normal((1, na, 13)).astype(np.float32))
    rb = torch.from_numpy(rng.standard_normal((1, nb, 13)).astype(np.float32))
    action = torch.from_numpy(rng.standard_normal(9).astype(np.float32))
    hand_row, cube_row = scenes.body_index("panda_env", "panda", "panda_hand"), scenes.body_index("panda_env", "cubeA", "box")
    robot_body = scenes.body_index("panda_env", "panda", "panda_link0")
    assert hand_row == robot_body + 8                       # (the kernel's index of the hand among the robot's 11 links)
    # closed_loop.run, trace=True, panda_env
    hand = rb[:, hand_row][0, :7].tolist()
    cube = rb[:, cube_row][0, :7].tolist()
    want_path = ["pick"] + hand + cube + dof[0, [14, 16]].tolist() + action[7:9].tolist()
    want_full = dict(tick=3, task="pick", dof_state=dof[0].tolist(), root_state=root[0].tolist(), action=action.reshape(-1).tolist())
    # the kernel's row
    row = np.zeros(L.PANDA_EPISODE_TRACE_FLOATS, np.float32)
    row[L.PE_TR_DOF:L.PE_TR_DOF + 18] = dof[0].numpy()
    row[L.PE_TR_ROOT:L.PE_TR_ACTION] = root[0].numpy().reshape(-1)
    row[L.PE_TR_ACTION:L.PE_TR_ACTION + 9] = action.numpy()
    row[L.PE_TR_HAND:L.PE_TR_HAND + 7] = rb[0, hand_row, :7].numpy()
    row[L.PE_TR_CUBE:L.PE_TR_CUBE + 7] = rb[0, cube_row, :7].numpy()
    d, a = row[L.PE_TR_DOF:L.PE_TR_ROOT], row[L.PE_TR_ACTION:L.PE_TR_HAND]
    path = ["pick"] + row[L.PE_TR_HAND:L.PE_TR_CUBE].tolist() + row[L.PE_TR_CUBE:L.PE_TR_CUBE + 7].tolist() + d[[14, 16]].tolist() + a[7:9].tolist()
    full = dict(tick=3, task="pick", dof_state=d.tolist(), root_state=row[L.PE_TR_ROOT:L.PE_TR_ACTION].reshape(-1, 13).tolist(), action=a.tolist())
    assert path == want_path and full == want_full


# ---- the simulator adapter: PLANNER_AIF_PANDA on recorded rows, through the wrapper's method and through RowSim ----
class _WrapperLike:
    """IsaacGymWrapper's env0_link_states_host / link_row / step on a recorded sequence of rigid-body states (the wrapper
    itself needs a HIP device): step() moves to the next recorded state, the host copy is cached per state version."""
    env_type = "panda_env"
    env0_link_states_host = None     # (bound below: the wrapper's own function)
    link_row = None

    def __init__(self, states):
        self.states, self.k = states, -1
        self._rb_host, self._state_version = None, 0

    @property
    def _rigid_body_state(self):
        return torch.from_numpy(self.states[self.k])[None]

    def step(self):
        self.k += 1
        self._state_version += 1


def _recorded_states(n=120):
    """A scripted pick-and-place as rigid-body states [17, 13] f32: the gripper approaches cubeA, carries it above cubeB,
    lowers it -- with f32 noise, so that the stage tests see thresholds crossed at arbitrary values."""
    rng = np.random.default_rng(11)
    row = lambda a, l: scenes.body_index("panda_env", a, l)
    iA, iB, iL, iR = row("cubeA", "box"), row("cubeB", "box"), row("panda", "panda_leftfinger"), row("panda", "panda_rightfinger")
    B = np.array([0.55, 0.25, 0.42], np.float32)
    A0 = np.array([0.45, -0.10, 0.42], np.float32)
    ee0 = np.array([0.30, 0.00, 0.80], np.float32)
    out = []
    for k in range(n):
        s = rng.standard_normal((17, 13)).astype(np.float32) * np.float32(1e-3)
        t = k / (n - 1)
        if t < 0.35:                     # reach
            ee, A = ee0 + (A0 + np.float32([0, 0, 0.02]) - ee0) * np.float32(t / 0.35), A0
        elif t < 0.8:                    # pick: carry towards the pre-place pose above cubeB
            u = np.float32((t - 0.35) / 0.45)
            A = A0 + (B + np.float32([0, 0, 0.055]) - A0) * u
            ee = A + np.float32([0, 0, 0.02])
        else:                            # place: lower
            u = np.float32((t - 0.8) / 0.2)
            A = B + np.float32([0, 0, 0.055 - 0.005 * u])
            ee = A + np.float32([0, 0, 0.02])
        for i, p in ((iA, A), (iB, B), (iL, ee + np.float32([0, 0.02, 0])), (iR, ee - np.float32([0, 0.02, 0]))):
            s[i, :3] += p
            s[i, 3:7] = np.float32([0, 0, 0, 1]) + s[i, 3:7] * np.float32(0.1)
        out.append(s)
    return out


def _drive(planner, sim, feed):
    seq = []
    for k in range(len(feed)):
        if sim is None:
            adapter.rows = feed[k]
            s = adapter
        else:
            s = sim
        planner.update_plan(s)
        ok = bool(planner.check_task_success(s))
        seq.append((planner.stage, planner.task, tuple(np.float32(planner.curr_goal.cpu().numpy()).tolist()), ok))
    return seq


def test_row_adapter_feeds_the_task_planner_what_the_wrapper_would():
    global adapter
    from m3p2i_aip_amd.episodes import RowSim
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymWrapper
    from m3p2i_aip_amd.task_planner import PLANNER_AIF_PANDA
    _WrapperLike.env0_link_states_host = IsaacGymWrapper.env0_link_states_host
    _WrapperLike.link_row = IsaacGymWrapper.link_row
    states = _recorded_states()
    cfg = types.SimpleNamespace(mppi=types.SimpleNamespace(device="cpu"), pre_height_diff=0.05)
    a, b = PLANNER_AIF_PANDA(cfg), PLANNER_AIF_PANDA(cfg)
    through_wrapper = _drive(a, _WrapperLike(states), states)
    adapter = RowSim("panda_env")
    through_adapter = _drive(b, None, states)
    assert through_wrapper == through_adapter
    assert [s[0] for s in through_wrapper][0] == 0 and {s[0] for s in through_wrapper} == {0, 1, 2}   # all three stages
    assert {s[1] for s in through_wrapper} >= {"reach", "pick", "place"}
    assert adapter.link_row("panda", "panda_hand") == scenes.body_index("panda_env", "panda", "panda_hand")
    adapter.step()        # (a no-op: the pre kernel took the step)
    assert adapter.env0_link_states_host() is states[-1]
