"""Lockstep panda episodes with run-time workspaces, weights and rows on the GPU (m3_panda_episodes_create_ex with
M3_PANDA_EPISODES_RUNTIME; include/m3p2i_hip.h).

Kernel level (no task planner): 65 episodes -- one more than a wavefront -- whose world rows and planner workspaces lie in two
different 5-cycles; the planning view after every observe and the world after every act are compared, as bytes, with twin
sim_only handles on the existing step-mode path (m3_sim_step_with_target with a workspace per environment, which
tests/test_panda_scene_rows_gpu.py pins to the oracle).  End to end: run_panda_episodes(..., panda_runtime=True) against
tools/closed_loop.run, episode by episode and bit for bit."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, HipPandaEpisodes, make_config  # noqa: E402
from tests import panda_rollout_scenes_ref as R  # noqa: E402
from tests import panda_scene_fixture as X  # noqa: E402

F = np.float32
DEV = "cuda:0"
PK = dict(u_min=X.UMIN, u_max=X.UMAX, noise_sigma_diag=X.SIG, lambda_=0.05, pre_height_diff=0.05, dt=0.01)
GOAL = np.array(X.GOAL, F)
CYCLE = (None, "table_z", "mu", "base", "COMBINED")
ERR_BAD_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5     # (include/m3p2i_hip.h)
SHIPPED = ["mppi.num_samples=200", "mppi.horizon=12"]
C4 = ["mppi.num_samples=4000", "mppi.horizon=20"]


@pytest.fixture(scope="module")
def P(oracle):
    import oracle.panda as P
    P.lib()
    return P


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


# ------------------------------------------------------------------ 1. kernel level: the set against twin step-mode handles
class Rig:
    """n episodes on engines made by hand.  World row e steps in CYCLE[e % 5], planner e plans in CYCLE[(e + 2) % 5] -- its single
    scene, or (every tenth planner) row 0 of per-sample rows whose other rows are the default; every sixth planner has tuned
    weights.  tick() runs one tick of the set and compares both kernels' results with the twins'."""

    def __init__(self, P, n=65, K=64, T=4, settle=1, max_ticks=8, world_rows=None, seed=5):
        from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
        from tests.test_device_dynamics_on_host import random_panda_worlds
        self.P, self.n, self.K, self.T, self.settle = P, n, K, T, settle
        rng = self.rng = np.random.default_rng(seed)
        self.world_rows = world_rows if world_rows is not None else [R.fields_of(CYCLE[e % 5]) for e in range(n)]
        self.plan_rows = [R.fields_of(CYCLE[(e + 2) % 5]) for e in range(n)]
        mk = lambda rows, envs=n: IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=envs, device=DEV, panda_scenes=rows)  # noqa: E731
        self.world, self.twin_w, self.twin_p = mk(self.world_rows), mk(self.world_rows), mk(self.plan_rows)
        # three K-env simulators whose row 0 keeps known targets: sims[e] = one of them, episode e's kept targets from tick 1 on
        self.kept_u = rng.uniform(-1, 1, (3, 9)).astype(F)
        self.sims = []
        for k in range(3):
            s = mk(None, K)
            s.set_dof_velocity_target_tensor(torch.from_numpy(np.tile(self.kept_u[k], (K, 1))).to(DEV))
            s.step()
            self.sims.append(s)
        self.planners, self.outs = [], []
        for e in range(n):
            eng = HipEngine(make_config(K=K, T=T, nu=9, env_type="panda_env", filter_u=False, **PK))      # (T = 4: below the filter's window)
            eng.set_objective("reach", GOAL, gripper_cmd=1)
            eng.set_noise(rng.standard_normal((K, T, 9)).astype(F))
            if e % 10 == 7:
                eng.set_panda_rollout_scenes([self.plan_rows[e]] + [None] * (K - 1))
            else:
                eng.set_panda_scene(self.plan_rows[e])
            if e % 6 == 0:
                eng.set_panda_cost_weights(dict(pick_ori=25.0))
            out = torch.from_numpy(rng.uniform(-1, 1, (T, 9)).astype(F)).to(DEV)      # (tick 0's plan: no command runs there)
            eng.set_action_out(out)
            eng.command()                     # (a planner's first command is its own, as in the episodes' tick 0: its lazy blocks)
            self.planners.append(eng)
            self.outs.append(out)
        w = random_panda_worlds(P, P.default_scene(), n, rng)
        for s in (self.world, self.twin_w):
            self._load(s, w)
        torch.cuda.synchronize()
        self.eps = HipPandaEpisodes(self.world._engine, self.planners, max_ticks=max_ticks, settle_ticks=settle, panda_runtime=True)
        self.batch = HipBatch(n, panda_runtime=True)
        self.dyn = [int(self.world._get_actor_index_by_name(x)) for x in ("cubeA", "cubeB", "dyn-obs")]
        self.ended = np.zeros(n, bool)
        self.settle_left = np.full(n, -1)         # -1 running; else settle steps still to take; 0: frozen
        self.frozen_world = {}                    # episode -> its row of the world when it froze
        self.last_rb = self.before = None

    def _load(self, sim, w):
        P = self.P
        ia, ib, io = (int(sim._get_actor_index_by_name(x)) for x in ("cubeA", "cubeB", "dyn-obs"))
        dof = torch.zeros(len(w), 18)
        dof[:, 0::2] = torch.from_numpy(w[:, P.W_Q:P.W_Q + 9])
        dof[:, 1::2] = torch.from_numpy(w[:, P.W_QD:P.W_QD + 9])
        root = sim._root_state.clone().cpu()
        root[:, ia, :] = torch.from_numpy(w[:, P.W_CUBEA:P.W_CUBEA + 13])
        root[:, ib, :] = torch.from_numpy(w[:, P.W_CUBEB:P.W_CUBEB + 13])
        root[:, io, :] = torch.from_numpy(w[:, P.W_OBS:P.W_OBS + 13])
        sim._dof_state[:] = dof.to(DEV)
        sim._root_state[:] = root.to(DEV)
        sim.set_dof_state_tensor(sim._dof_state)
        sim.set_actor_root_state_tensor(sim._root_state)

    def _world_rows_of(self, sim):
        """per environment: its column of the SoA world and its rows of the three views, as bytes"""
        soa = sim._engine.buffer(L.BUF_SIM_WORLD).cpu().numpy().reshape(77, self.n)
        views = [t.cpu().numpy().reshape(self.n, -1) for t in (sim._dof_state, sim._root_state, sim._rigid_body_state)]
        return [soa[:, e].tobytes() + b"".join(v[e].tobytes() for v in views) for e in range(self.n)]

    def tick(self, end=()):
        """one tick; `end`: the episodes the host ends at this tick"""
        n, eps = self.n, self.eps
        tick = eps.ticks_done
        running = self.settle_left < 0
        # ---- observe: the pre kernel of the running episodes against the twin in the planners' workspaces ----
        rb = eps.observe().copy()
        tp, w = self.twin_p, self.world
        tp._dof_state[:] = w._dof_state
        tp._root_state[:, self.dyn] = w._root_state[:, self.dyn]
        tp.set_dof_state_tensor(tp._dof_state)
        tp.set_actor_root_state_tensor(tp._root_state)
        kept = np.zeros((n, 9), F) if tick == 0 else np.stack([self.kept_u[e % 3] for e in range(n)])
        tp.set_dof_velocity_target_tensor(torch.from_numpy(kept).to(DEV))
        tp.step()
        want = tp._rigid_body_state.cpu().numpy()
        for e in range(n):
            if running[e]:
                assert rb[e].tobytes() == want[e].tobytes(), ("planning view", tick, e)
            else:
                assert rb[e].tobytes() == self.last_rb[e].tobytes(), ("planning view of an ended episode", tick, e)
        self.last_rb = rb
        # ---- act: the post kernel against the twin in the world's workspaces ----
        for e in end:
            assert running[e]
            self.ended[e] = True
            self.settle_left[e] = self.settle
        flags = list(self.ended)
        if tick == 0:
            eps.act_first([self.sims[e % 3]._engine for e in range(n)], flags)
        else:
            eps.act(self.batch, flags)
        torch.cuda.synchronize()
        targets = np.stack([np.zeros(9, F) if self.ended[e] else self.outs[e][0].cpu().numpy() for e in range(n)])
        tw = self.twin_w
        tw.set_dof_velocity_target_tensor(torch.from_numpy(targets).to(DEV))
        tw.step()
        got, ref = self._world_rows_of(self.world), self._world_rows_of(tw)
        for e in range(n):
            if e in self.frozen_world:
                assert got[e] == self.frozen_world[e], ("a frozen episode's row moved", tick, e)
                continue
            if self.settle_left[e] == 0:            # (ended with no settle step left: it froze before this tick's step)
                self.frozen_world[e] = self.before[e]
                assert got[e] == self.before[e], ("an episode stepped after its settle steps", tick, e)
                continue
            assert got[e] == ref[e], ("world", tick, e)
            if self.settle_left[e] > 0:
                self.settle_left[e] -= 1
                if self.settle_left[e] == 0:
                    self.frozen_world[e] = got[e]
        self.before = got
        return got

    def close(self):
        for x in (getattr(self, "eps", None), getattr(self, "batch", None)):
            if x is not None:
                x.close()
        for s in [self.world, self.twin_w, self.twin_p] + self.sims:
            s.stop_sim()
        for e in self.planners:
            e.close()


def test_65_episodes_in_two_cycles_of_workspaces_equal_the_step_mode_twins(P):
    rig = Rig(P)
    try:
        assert rig.eps.flags() == L.PANDA_EPISODES_RUNTIME and rig.batch.flags() == L.BATCH_PANDA_RUNTIME
        # the guard: the two sides of every episode differ, and each side shows all five workspaces
        full = lambda f: L.panda_scene_dict(L.panda_scene_fields(f))      # noqa: E731
        assert all(full(a) != full(b) for a, b in zip(rig.world_rows, rig.plan_rows))
        first = rig.tick()                                  # tick 0: observe, act_first
        rig.tick(end=[e for e in range(rig.n) if e % 4 == 1])       # tick 1: the first batched command; a quarter ends
        rig.tick()                                          # tick 2: the ended have had their one settle step and stay
        last = rig.tick()
        moved = [first[e] != last[e] for e in range(rig.n)]
        assert all(moved)                                   # (every row was stepped at all)
        assert len(rig.frozen_world) == len([e for e in range(rig.n) if e % 4 == 1])
        st = rig.eps.status()
        assert [s["phase"] for s in st] == [L.PE_FROZEN if e % 4 == 1 else L.PE_RUNNING for e in range(rig.n)]
        # what each planner's batched command launched: its own record, as m3_command would leave it
        for e, eng in enumerate(rig.planners):
            if e % 4 == 1:
                continue
            assert eng.panda_scene_instance_used() == (e % 10 == 7 or rig.plan_rows[e] not in (None,)), e
            assert eng.panda_weighted_cost_instance_used() == (e % 6 == 0), e
    finally:
        rig.close()


# ------------------------------------------------------------------ 5. between ticks
def test_rows_set_on_the_world_between_ticks_apply_from_the_next_tick(P):
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    n = 9
    rig = Rig(P, n=n, max_ticks=10, seed=6)
    old = IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=n, device=DEV, panda_scenes=rig.world_rows)
    try:
        for _ in range(4):                                  # ticks 0 .. 3 in the rows the world was built with
            rig.tick()
        # a twin that stays in the old rows, from the world's state after tick 3
        for name in ("_dof_state", "_root_state"):
            getattr(old, name)[:] = getattr(rig.world, name)
        old._engine.buffer(L.BUF_SIM_WORLD).copy_(rig.world._engine.buffer(L.BUF_SIM_WORLD))
        new_rows = [R.fields_of(CYCLE[(e + 1) % 5]) for e in range(n)]
        rig.world._engine.set_panda_scene_rows(new_rows)
        rig.twin_w._engine.set_panda_scene_rows(new_rows)
        got = rig.tick()                                    # tick 4: compared with the twin in the NEW rows inside
        torch.cuda.synchronize()
        targets = np.stack([rig.outs[e][0].cpu().numpy() for e in range(n)])
        old.set_dof_velocity_target_tensor(torch.from_numpy(targets).to(DEV))
        old.step()
        soa = lambda s: s._engine.buffer(L.BUF_SIM_WORLD).cpu().numpy().reshape(77, n)      # noqa: E731
        differ = (soa(old).view(np.uint32) != soa(rig.world).view(np.uint32)).any(axis=0)
        assert differ.mean() >= 0.5, differ                 # the guard: the old rows would have shown
        rig.tick()
        assert got is not None
    finally:
        old.stop_sim()
        rig.close()


def test_a_switch_forced_off_between_ticks_refuses_the_tick_and_launches_nothing(P):
    rig = Rig(P, n=5, seed=7)
    try:
        rig.tick()
        rig.tick()
        torch.cuda.synchronize()
        before = rig._world_rows_of(rig.world)
        calls = [e.info().calls for e in rig.planners]
        culprit = rig.planners[1]                           # plans in CYCLE[3]: a geometry of its own
        culprit.set_panda_scene_instance(0)
        rc = rig.eps.lib.m3_panda_episodes_observe(rig.eps._eps, rig.eps._rb)
        assert rc == ERR_STATE
        with pytest.raises(L.M3Error, match="m3_panda_episodes_observe: planner 1: .*forced off .*m3_set_panda_scene"):
            rig.eps.observe()
        torch.cuda.synchronize()
        assert rig._world_rows_of(rig.world) == before and rig.eps.ticks_done == 2
        assert [e.info().calls for e in rig.planners] == calls
        culprit.set_panda_scene_instance(-1)
        rig.tick()                                          # the tick goes on as if nothing had happened: the twins agree
        # ... and between observe and act: act is refused with the same code, the world stays
        rig.eps.observe()
        rig.planners[0].set_panda_weighted_cost_instance(0)     # planner 0 has tuned weights
        before = rig._world_rows_of(rig.world)
        with pytest.raises(L.M3Error, match="m3_panda_episodes_act: planner 0: .*forced off .*m3_set_panda_cost_weights"):
            rig.eps.act(rig.batch, [False] * rig.n)
        torch.cuda.synchronize()
        assert rig._world_rows_of(rig.world) == before and rig.eps.ticks_done == 3
    finally:
        rig.close()


# ------------------------------------------------------------------ 6. refusals and memory
def test_refusals_and_the_ledger(P):
    lib = L.load()
    live0 = lib.m3_owned_blocks_live()
    rig = Rig(P, n=4, max_ticks=40, seed=8)
    plain = HipBatch(4)
    try:
        import ctypes as C
        eps, arr = rig.eps, (C.c_void_p * 4)(*[e._h.value for e in rig.planners])
        out = C.c_void_p()
        # unknown bits; flags == 0 refuses what m3_panda_episodes_create refuses, in its words
        assert lib.m3_panda_episodes_create_ex(rig.world._engine._h, arr, 4, 8, 0, 0, 6, C.byref(out)) == ERR_BAD_ARG and not out.value
        assert lib.m3_panda_episodes_last_error(None) == b"m3_panda_episodes_create_ex: unknown flag bits"
        texts = []
        for call in (lambda: lib.m3_panda_episodes_create(rig.world._engine._h, arr, 4, 8, 0, 0, C.byref(out)),
                     lambda: lib.m3_panda_episodes_create_ex(rig.world._engine._h, arr, 4, 8, 0, 0, 0, C.byref(out))):
            assert call() == ERR_UNSUPPORTED and not out.value
            texts.append(lib.m3_panda_episodes_last_error(None))
        assert texts[0] == texts[1] and texts[0].startswith(b"m3_panda_episodes_create: the world: ") and b"m3_set_panda_scene_rows" in texts[0]
        rig.world._engine.set_panda_scene_rows(None)        # the world on the default scene: now the first planner is what is refused
        for call in (lambda: lib.m3_panda_episodes_create(rig.world._engine._h, arr, 4, 8, 0, 0, C.byref(out)),
                     lambda: lib.m3_panda_episodes_create_ex(rig.world._engine._h, arr, 4, 8, 0, 0, 0, C.byref(out))):
            assert call() == ERR_UNSUPPORTED and not out.value
            text = lib.m3_panda_episodes_last_error(None)
            assert text.startswith(b"m3_panda_episodes_create: planner 0: ") and b"m3_set_panda_scene" in text
        rig.world._engine.set_panda_scene_rows(rig.world_rows)
        # every other refusal stays under the flag: a sim_only planner, a handle listed twice, a forced-off switch
        twice = (C.c_void_p * 4)(*[rig.planners[i]._h.value for i in (0, 1, 1, 3)])
        assert lib.m3_panda_episodes_create_ex(rig.world._engine._h, twice, 4, 8, 0, 0, 1, C.byref(out)) == ERR_BAD_ARG
        assert b"planner 2: handle listed twice" in lib.m3_panda_episodes_last_error(None)
        simonly = (C.c_void_p * 4)(*([rig.planners[i]._h.value for i in (0, 1, 2)] + [rig.sims[0]._engine._h.value]))
        assert lib.m3_panda_episodes_create_ex(rig.world._engine._h, simonly, 4, 8, 0, 0, 1, C.byref(out)) == ERR_STATE
        assert b"planner 3: handle was created sim_only" in lib.m3_panda_episodes_last_error(None)
        rig.planners[1].set_panda_scene_instance(0)
        assert lib.m3_panda_episodes_create_ex(rig.world._engine._h, arr, 4, 8, 0, 0, 1, C.byref(out)) == ERR_STATE
        assert b"planner 1: " in lib.m3_panda_episodes_last_error(None) and b"forced off" in lib.m3_panda_episodes_last_error(None)
        rig.planners[1].set_panda_scene_instance(-1)
        rig.world._engine.set_panda_scene_instance(0)
        assert lib.m3_panda_episodes_create_ex(rig.world._engine._h, arr, 4, 8, 0, 0, 1, C.byref(out)) == ERR_STATE
        assert b"the world: " in lib.m3_panda_episodes_last_error(None) and b"forced off" in lib.m3_panda_episodes_last_error(None)
        rig.world._engine.set_panda_scene_instance(-1)
        # a plain batch handed to the run-time set's act: the batch's own refusal, nothing launched
        live_first = lib.m3_owned_blocks_live()             # (before the first tick)
        rig.tick()
        rig.eps.observe()
        torch.cuda.synchronize()
        before = rig._world_rows_of(rig.world)
        calls = [e.info().calls for e in rig.planners]
        rc = lib.m3_panda_episodes_act(eps._eps, plain._b, eps._flags([False] * 4))
        assert rc == ERR_UNSUPPORTED
        err = lib.m3_panda_episodes_last_error(eps._eps)
        assert err.startswith(b"m3_panda_episodes_act: m3_batch_command: handle 0: ") and b"m3_set_panda_" in err
        torch.cuda.synchronize()
        assert rig._world_rows_of(rig.world) == before and [e.info().calls for e in rig.planners] == calls and eps.ticks_done == 1
        eps.act(rig.batch, [False] * 4)                     # the same tick with the right batch
        torch.cuda.synchronize()
        # no block comes to life in a tick: the ledger's count before the first tick and after the twentieth
        for _ in range(18):
            eps.observe()
            eps.act(rig.batch, [False] * 4)
        torch.cuda.synchronize()
        assert eps.ticks_done == 20 and lib.m3_owned_blocks_live() == live_first
    finally:
        plain.close()
        rig.close()
    assert lib.m3_owned_blocks_live() == live0


# ------------------------------------------------------------------ 2 .. 4. end to end against the serial loop
def _tools():
    import band_stats
    import closed_loop
    return band_stats, closed_loop


JITTER = dict(cube=(0.011, -0.007))
_SERIAL = {}


def _serial(ov, ticks, settle):
    """closed_loop.run of one episode + what its planner's last command launched (read before Tamp.close)."""
    _, closed_loop = _tools()
    key = (tuple(ov), ticks, settle)
    if key not in _SERIAL:
        used, close = [], closed_loop.Tamp.close

        def closing(self):
            e = self.motion_planner._engine
            used.append((e.panda_lanes_per_sample_used(), e.panda_scene_instance_used(), e.panda_weighted_cost_instance_used()))
            close(self)

        closed_loop.Tamp.close = closing
        try:
            r = closed_loop.run("config_panda", list(ov), ticks=ticks, jitter=JITTER, settle_ticks=settle, trace=True)
        finally:
            closed_loop.Tamp.close = close
        r["lanes_per_sample_used"], r["m3_panda_scene_instance_used"], r["m3_panda_weighted_cost_instance_used"] = used[-1]
        _SERIAL[key] = r
    return _SERIAL[key]


def _same(a, b, what):
    from tests.test_panda_episodes_gpu import _same as same
    same(a, b, what)
    for k in ("lanes_per_sample_used", "m3_panda_scene_instance_used", "m3_panda_weighted_cost_instance_used"):
        assert a[k] == b[k], (what, k, a[k], b[k])


def test_default_workspaces_under_the_flag_give_the_plain_sets_reports():
    from m3p2i_aip_amd.episodes import run_panda_episodes
    from tests.test_panda_episodes_gpu import _jitter
    eps = [("config_panda", SHIPPED, _jitter(e)) for e in range(3)]
    plain = run_panda_episodes(eps, max_ticks=150, settle_ticks=0, trace=True)
    rt = run_panda_episodes(eps, max_ticks=150, settle_ticks=0, trace=True, panda_runtime=True)
    timing = ("tick_ms_p50", "tick_ms_p99", "observe_ms_p50", "host_ms_p50", "act_ms_p50", "build_s", "first_s", "loop_s")
    for e, (a, b) in enumerate(zip(rt, plain)):
        assert not a.pop("m3_panda_scene_instance_used") and not a.pop("m3_panda_weighted_cost_instance_used")
        for k in timing:
            a.pop(k), b.pop(k)
        assert a.keys() == b.keys() and len(a["trace"]) >= 100
        from tests.test_panda_episodes_gpu import _same as same
        same(a, b, f"default workspaces, episode {e}")        # ticks, success, timeline, both cube metrics, every trace and full row
        for k in a:
            if k not in ("trace", "full"):
                assert a[k] == b[k], (e, k, a[k], b[k])


MIXED = [["panda_scene={table: [0, 0, 0.99, 0.6, 0.6, 0.025], mu: 0.5}"],
         ["world_panda_scene={cube_m: 0.2}"],
         ["panda_cost_weights={pick_ori: 25.0}"],
         ["world_panda_scene={cube_m: 0.2}", "rollout_workspace_spread={spread: 0.3, seed: 1}"]]


def test_a_mixed_set_equals_the_serial_loop_episode_by_episode():
    from m3p2i_aip_amd.episodes import run_panda_episodes
    ticks = 150
    serial = [_serial(SHIPPED + ov, ticks, 0) for ov in MIXED]
    # the guard: within these ticks the four serial traces differ pairwise -- a mix-up of rows could not pass
    traces = [np.asarray([row[1:] for row in s["trace"]], np.float64).tobytes() for s in serial]      # (row[0]: the task's name)
    for i in range(4):
        for j in range(i):
            assert traces[i] != traces[j], ("the serial traces of episodes", j, i, "coincide")
    reps = run_panda_episodes([("config_panda", SHIPPED + ov, JITTER) for ov in MIXED], max_ticks=ticks, settle_ticks=0, trace=True,
                              panda_runtime=True)
    for e, (r, s) in enumerate(zip(reps, serial)):
        _same(r, s, f"mixed episode {e}")
    assert [r["m3_panda_scene_instance_used"] for r in reps] == [True, False, False, True]
    assert [r["m3_panda_weighted_cost_instance_used"] for r in reps] == [False, False, True, False]


def test_one_full_length_episode_with_a_heavier_cube_and_a_spread_equals_its_serial_run():
    from m3p2i_aip_amd.episodes import run_panda_episodes
    ov = SHIPPED + MIXED[3]
    s = _serial(ov, 600, 7)
    r = run_panda_episodes([("config_panda", ov, JITTER)], max_ticks=600, settle_ticks=7, trace=True, panda_runtime=True)[0]
    _same(r, s, "full length")
    assert r["success"] and r["ticks"] < 600          # (it ends by success, so the seven settle steps ran before the cube metrics)
