"""Batched closed-loop episodes (point_env): N episodes of tools/closed_loop.run in lockstep.

    from m3p2i_aip_amd.episodes import run_point_episodes
    reports = run_point_episodes([("config_point", ["task=push", "goal=[-3,3]"], dict(dyn_phase=30)), ...], max_ticks=800)

One N-env "real world" (an IsaacGymWrapper(num_envs=N)) holds the episodes' 1-env worlds, one row each; each episode has
its own planner, Objective and task planner, built as tools/closed_loop.Tamp builds them.  Every tick is one library call
for all episodes (m3_episodes_tick: pre-command kernel, one batched command of the running planners, post-command kernel,
one synchronisation).  Each episode's report equals what closed_loop.run(cn, overrides, ticks=max_ticks, jitter=jitter)
returns, bit for bit: ticks, success, final error, collision ticks, trace rows.
"""
from __future__ import annotations

import time

import numpy as np
import torch

from . import _lib as L
from . import compat
from .engine import HipBatch, HipEpisodes


class _PlannerSide:
    """The planner side of one episode: tools/closed_loop.Tamp (scripts/reactive_tamp.py's REACTIVE_TAMP), built through
    the same module names."""

    def __init__(self, cfg):
        from m3p2i_aip.planners.motion_planner import m3p2i
        from m3p2i_aip.planners.task_planner import task_planner
        import m3p2i_aip.utils.isaacgym_utils.isaacgym_wrapper as wrapper
        from m3p2i_aip.planners.motion_planner.cost_functions import Objective
        self.cfg = cfg
        self.sim = wrapper.IsaacGymWrapper(cfg.isaacgym, cfg.env_type, num_envs=cfg.mppi.num_samples,
                                           viewer=False, device=cfg.mppi.device, cube_on_shelf=cfg.cube_on_shelf)
        self.objective = Objective(cfg)
        self.task_planner = task_planner.set_task_planner(cfg)
        self.task_success = False
        self.suction_active = False
        self.motion_planner = m3p2i.M3P2I(cfg, dynamics=self.dynamics, running_cost=self.running_cost)

    def dynamics(self, _, u, t=None):
        self.sim.set_dof_velocity_target_tensor(u)
        self.sim.step()
        return torch.stack([self.sim.robot_pos[:, 0], self.sim.robot_vel[:, 0],
                            self.sim.robot_pos[:, 1], self.sim.robot_vel[:, 1]], dim=1), u

    def running_cost(self, _):
        return self.objective.compute_cost(self.sim)

    def first_plan(self, dof_state, root_state):
        """Tamp.run_tamp of tick 0, returning the whole plan: (e) the planner's first command runs the fused / step probe
        on its own K-env sim and returns the STEP leg's plan -- this is that call."""
        self.sim._dof_state[:] = dof_state
        self.sim._root_state[:] = root_state
        self.sim.set_dof_state_tensor(self.sim._dof_state)
        self.sim.set_actor_root_state_tensor(self.sim._root_state)
        self.task_planner.update_plan(self.sim)
        self.motion_planner.update_gripper_command(self.task_planner.task)
        self.objective.update_objective(self.task_planner.task, self.task_planner.curr_goal)
        self.suction_active = self.motion_planner.get_pull_preference()
        self.task_success = bool(self.task_planner.check_task_success(self.sim))
        if self.task_success:
            raise RuntimeError("run_point_episodes: the host's success test disagrees with the device's at tick 0")
        return self.motion_planner.command(self.sim._dof_state[0])

    def close(self):
        self.sim.stop_sim()
        self.motion_planner._engine.close()


def _suction_mode(cfg):
    """What check_and_apply_suction does in closed_loop.run (compat._suction_enabled with cfg.suction_active set from
    run_tamp's get_pull_preference()): push / navigation never; pull with the planner's constant suction_active;
    push_pull (multi-modal) with the previous command's pull preference."""
    if cfg.task not in ("pull", "push_pull"):
        return L.SUCTION_OFF
    if cfg.multi_modal:
        return L.SUCTION_PULL_PREFERENCE
    return L.SUCTION_ON if bool(cfg.suction_active) else L.SUCTION_OFF


def _apply_jitter(real, e, jitter):
    """closed_loop.run's jitter of its 1-env world, the same torch ops on row e."""
    phase = int(jitter.get("dyn_phase", 0))
    ib = int(real._get_actor_index_by_name("box"))
    if jitter.get("box_start") is not None:
        real._root_state[e, ib, 0] = float(jitter["box_start"][0])
        real._root_state[e, ib, 1] = float(jitter["box_start"][1])
    real._root_state[e, ib, 0] += float(jitter.get("box", (0, 0))[0])
    real._root_state[e, ib, 1] += float(jitter.get("box", (0, 0))[1])
    off = sum(0.01 if 25 < (i % 100) < 75 else -0.01 for i in range(phase))
    idn = int(real._get_actor_index_by_name("dyn-obs"))
    real._root_state[e, idn, 0] += off
    real._root_state[e, idn, 1] += off
    real._dof_state[e, 0] += float(jitter.get("robot", (0, 0))[0])
    real._dof_state[e, 2] += float(jitter.get("robot", (0, 0))[1])
    return phase


class PointEpisodeSet:
    """One set of episodes in lockstep: built by the constructor, tick 0 by start() (each planner's first command on its
    own), then tick() per tick; reports() when no episode runs any more (or at max_ticks).  items: [(config name,
    overrides, config, jitter)] of one world (same dt, substeps, device)."""

    def __init__(self, items, max_ticks, trace=False):
        import m3p2i_aip.utils.isaacgym_utils.isaacgym_wrapper as wrapper
        t0 = time.perf_counter()
        self.items, self.max_ticks, self.trace = list(items), int(max_ticks), bool(trace)
        cfgs = [cfg for _, _, cfg, _ in self.items]
        self.sides = [_PlannerSide(cfg) for cfg in cfgs]
        c0, n = cfgs[0], len(self.items)
        self.real = real = wrapper.IsaacGymWrapper(c0.isaacgym, c0.env_type, num_envs=n, viewer=False, device=c0.mppi.device,
                                                   cube_on_shelf=c0.cube_on_shelf)
        phases = [_apply_jitter(real, e, jitter) if jitter else 0 for e, (*_, jitter) in enumerate(self.items)]
        if any(jitter for *_, jitter in self.items):
            real.set_dof_state_tensor(real._dof_state)
            real.set_actor_root_state_tensor(real._root_state)
        self.outs, specs = [], []
        for e, (side, cfg) in enumerate(zip(self.sides, cfgs)):
            mp = side.motion_planner
            mp._engine.use_torch_stream()
            mp._ensure_noise()
            out = torch.zeros(mp.T, mp.nu, device=mp.device, dtype=torch.float32)   # (an episode that never commands steps on 0)
            mp._engine.set_action_out(out)
            self.outs.append(out)
            g = side.task_planner.curr_goal.float().cpu().reshape(-1)
            specs.append((cfg.task, (float(g[0]), float(g[1])), phases[e], _suction_mode(cfg), float(cfg.kp_suction)))
        real._engine.use_torch_stream()
        self.eps = HipEpisodes(real._engine, [s.motion_planner._engine for s in self.sides], specs, self.max_ticks, trace=self.trace)
        self.batch = HipBatch(n, device=torch.device(c0.mppi.device).index or 0)
        self.lat = []
        self.build_s = time.perf_counter() - t0
        self.loop_s = 0.0

    def start(self):
        """Tick 0: each planner's first command on its own (the probe), between the two halves of the tick."""
        eps = self.eps
        eps.begin()
        st = eps.status()
        for e, side in enumerate(self.sides):
            if st[e]["done_tick"] >= 0:
                continue
            plan = side.first_plan(self.real._dof_state[e:e + 1], self.real._root_state[e:e + 1])
            if side.motion_planner._fused is not True:
                raise RuntimeError(f"run_point_episodes: episode {e}'s planner chose the step path at its probe; "
                                   "the batched command runs the fused path only")
            self.outs[e].copy_(plan)
            side.motion_planner._engine.set_action_out(self.outs[e])
        eps.end()

    @property
    def running(self):
        return self.eps.running if self.eps.ticks_done < self.max_ticks else 0

    def tick(self):
        t = time.perf_counter()
        self.eps.tick(self.batch)
        self.lat.append(time.perf_counter() - t)

    def run(self):
        self.start()
        t = time.perf_counter()
        while self.running:
            self.tick()
        self.loop_s = time.perf_counter() - t

    def reports(self):
        st, tr = self.eps.status(with_trace=True) if self.trace else (self.eps.status(), None)
        lat = self.lat
        p50 = float(np.percentile(lat, 50) * 1e3) if lat else 0.0
        p99 = float(np.percentile(lat, 99) * 1e3) if lat else 0.0
        reports = []
        for e, ((cn, ov, cfg, _), side) in enumerate(zip(self.items, self.sides)):
            s = st[e]
            i = s["done_tick"] if s["done_tick"] >= 0 else self.eps.ticks_done - 1
            goal = side.task_planner.curr_goal.float().cpu()
            who = torch.tensor(s["final_pos"], dtype=torch.float32)
            r = dict(config=cn, overrides=list(ov), K=cfg.mppi.num_samples, T=cfg.mppi.horizon, ticks=i + 1,
                     success=s["success"], transport="batched", sim_time_s=(i + 1) * cfg.isaacgym.dt,
                     timeline=[(0, side.task_planner.task)], tick_ms_p50=p50, tick_ms_p99=p99, build_s=self.build_s,
                     loop_s=self.loop_s,
                     final_pos_error=float(torch.norm(who - goal)),       # (d) CPU torch on the f32 positions
                     dyn_obs_collision_ticks=s["collision_ticks"])
            if self.trace:
                rows = i if s["success"] else i + 1      # (no row for the success tick: the serial loop ends before it)
                r["trace"] = tr[:rows, e].tolist()
            reports.append(r)
        return reports

    def close(self):
        for x in (getattr(self, "eps", None), getattr(self, "batch", None)):
            if x is not None:
                x.close()
        if getattr(self, "real", None) is not None:
            self.real.stop_sim()
        for side in getattr(self, "sides", []):
            side.close()


def build_set(episodes, max_ticks=800, trace=False):
    """A PointEpisodeSet of episodes [(config name, overrides, jitter)] that share one world."""
    compat.install(force_standins=True)
    items = []
    for idx, (cn, ov, jitter) in enumerate(episodes):
        cfg = compat.make_config(cn, list(ov))
        if cfg.env_type != "point_env":
            raise ValueError(f"run_point_episodes: episode {idx} is {cfg.env_type} (point_env only)")
        items.append((cn, list(ov), cfg, jitter))
    return PointEpisodeSet(items, max_ticks, trace)


def run_point_episodes(episodes, max_ticks=800, trace=False):
    """episodes: [(config name, overrides, jitter)] as closed_loop.run takes them (jitter may be None).  Returns one report
    per episode, in order: the dict closed_loop.run returns (ticks, success, sim_time_s, timeline, final_pos_error,
    dyn_obs_collision_ticks, trace if asked), with the set's tick_ms_p50 / tick_ms_p99 in place of the per-episode
    command_ms_*, and build_s (planner and world construction) / loop_s (ticks 1..) of the set.  Episodes whose worlds
    differ (dt, substeps, device) run as separate sets, one after the other."""
    if int(max_ticks) <= 0:
        raise ValueError("run_point_episodes: max_ticks must be > 0")
    compat.install(force_standins=True)
    groups = {}
    for idx, (cn, ov, jitter) in enumerate(episodes):
        cfg = compat.make_config(cn, list(ov))
        if cfg.env_type != "point_env":
            raise ValueError(f"run_point_episodes: episode {idx} is {cfg.env_type} (point_env only)")
        key = (float(cfg.isaacgym.dt), int(cfg.isaacgym.substeps), cfg.mppi.device)
        groups.setdefault(key, []).append((idx, (cn, list(ov), cfg, jitter)))
    out = [None] * len(episodes)
    for members in groups.values():
        es = PointEpisodeSet([m for _, m in members], int(max_ticks), bool(trace))
        try:
            es.run()
            reps = es.reports()
        finally:
            es.close()
        for (idx, _), r in zip(members, reps):
            out[idx] = r
    return out
