"""Batched closed-loop episodes: N episodes of tools/closed_loop.run in lockstep -- point_env (below) and
panda_env (§7d: run_panda_episodes / PandaEpisodeSet at the end of this module).

    from m3p2i_aip_amd.episodes import run_point_episodes
    reports = run_point_episodes([("config_point", ["task=push", "goal=[-3,3]"], dict(dyn_phase=30)), ...], max_ticks=800)

One N-env "real world" (an IsaacGymWrapper(num_envs=N)) holds the episodes' 1-env worlds, one row each; each episode has
its own planner, Objective and task planner, built as tools/closed_loop.Tamp builds them.  Every tick is one library call
for all episodes (m3_episodes_tick: pre-command kernel, one batched command of the running planners, post-command kernel,
one synchronisation).  Each episode's report equals what closed_loop.run(cn, overrides, ticks=max_ticks, jitter=jitter)
returns, bit for bit: ticks, success, final error, collision ticks, trace rows.  Episodes may differ in their arena
(`point_scene`, `world_point_scene` overrides): each planner plans in its own, each row of the world is stepped in its own.
"""
from __future__ import annotations

import dataclasses
import time

import numpy as np
import torch

from . import _lib as L
from . import compat
from . import scenes
from .engine import HipBatch, HipEpisodes, HipPandaEpisodes


class _PlannerSide:
    """The planner side of one episode: tools/closed_loop.Tamp (scripts/reactive_tamp.py's REACTIVE_TAMP), built through
    the same module names."""

    def __init__(self, cfg, panda_scenes=None, point_scenes=None):
        from m3p2i_aip.planners.motion_planner import m3p2i
        from m3p2i_aip.planners.task_planner import task_planner
        import m3p2i_aip.utils.isaacgym_utils.isaacgym_wrapper as wrapper
        from m3p2i_aip.planners.motion_planner.cost_functions import Objective
        self.cfg = cfg
        # (panda_scenes: the `rollout_workspace_spread` rows of a run-time panda set, as Tamp passes them; None everywhere else)
        # (point_scenes: the `rollout_arena_spread` rows of a point set with point_runtime, likewise)
        extra = {} if panda_scenes is None else dict(panda_scenes=panda_scenes)
        if point_scenes is not None:
            extra["point_scenes"] = point_scenes
        self.sim = wrapper.IsaacGymWrapper(cfg.isaacgym, cfg.env_type, num_envs=cfg.mppi.num_samples,
                                           viewer=False, device=cfg.mppi.device, cube_on_shelf=cfg.cube_on_shelf, **extra)
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
        if compat.prior_samples_on_device(self.cfg):     # (Tamp._set_prior_samples: set once, the device does the rest every tick)
            compat.set_device_prior_controller(self.cfg, self.motion_planner)
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
    overrides, config, jitter)] of one world (same dt, substeps, device).
    point_runtime: episodes may ask for an arena per sample of their planner (`rollout_arena_spread`): each planner's K-env sim is
    built with compat.rollout_point_scenes(cfg) as tools/closed_loop.Tamp builds it, so its tick-0 probe keeps the fused path and
    the engine holds the rows from then on (m3_episodes_create_ex with M3_EPISODES_ROLLOUT_SCENES, a batch with
    M3_BATCH_SECTION_POINT_ROLLOUT_SCENES).  Episodes with and without the key share the set.
    point_priors: episodes may ask for prior samples from a controller on the device (`prior_samples={..., device: true}`): the
    planner gets its controller before its first command and reads its episode's row of the world every tick, on the device
    (m3_episodes_create_ex with M3_EPISODES_PRIORS, a batch with M3_BATCH_SECTION_POINT_PRIORS).  Episodes with and without the
    key share the set."""

    def __init__(self, items, max_ticks, trace=False, point_runtime=False, point_priors=False):
        import m3p2i_aip.utils.isaacgym_utils.isaacgym_wrapper as wrapper
        t0 = time.perf_counter()
        self.items, self.max_ticks, self.trace = list(items), int(max_ticks), bool(trace)
        cfgs = [cfg for _, _, cfg, _ in self.items]
        self.point_runtime, self.point_priors = bool(point_runtime), bool(point_priors)
        if self.point_runtime:
            self.sides = [_PlannerSide(cfg, point_scenes=compat.rollout_point_scenes(cfg)) for cfg in cfgs]
        else:
            self.sides = [_PlannerSide(cfg) for cfg in cfgs]
        c0, n = cfgs[0], len(self.items)
        # each episode's world arena: its `point_scene` with its `world_point_scene` on top.  All the same: the single-arena
        # world as before; otherwise one arena per row (m3_set_point_scene_rows) -- the planners keep their own `point_scene`
        arenas = [compat.world_point_scene(cfg) for cfg in cfgs]
        rows = None if all(a == arenas[0] for a in arenas) else arenas
        self.real = real = wrapper.IsaacGymWrapper(compat.world_isaacgym_config(c0), c0.env_type, num_envs=n, viewer=False,
                                                   device=c0.mppi.device, cube_on_shelf=c0.cube_on_shelf, point_scenes=rows)
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
        engines = [s.motion_planner._engine for s in self.sides]
        dev = torch.device(c0.mppi.device).index or 0
        if self.point_priors:
            self.eps = HipEpisodes(real._engine, engines, specs, self.max_ticks, trace=self.trace, point_runtime=self.point_runtime,
                                   point_priors=True)
            self.batch = HipBatch(n, device=dev, point_runtime=self.point_runtime, point_priors=True)
        elif self.point_runtime:
            self.eps = HipEpisodes(real._engine, engines, specs, self.max_ticks, trace=self.trace, point_runtime=True)
            self.batch = HipBatch(n, device=dev, point_runtime=True)
        else:
            self.eps = HipEpisodes(real._engine, engines, specs, self.max_ticks, trace=self.trace)
            self.batch = HipBatch(n, device=dev)
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


def _check_episode_priors(cfg, idx, point_priors):
    """the `prior_samples` key of an episode of a lockstep set: only a controller on the device can serve it (the episodes'
    worlds live on the device and a tick is one library call for all of them), and only in a set built for priors.  The
    `rollout_arena_groups` key no set serves: the batched command has no aggregation between its rollout and its update."""
    if getattr(cfg, "rollout_arena_groups", None):
        raise ValueError(f"run_point_episodes: episode {idx} asks for sample groups (rollout_arena_groups), which the batched "
                         "command does not run (m3_set_sample_groups: m3_command only); use closed_loop.run")
    if not getattr(cfg, "prior_samples", None):
        return
    if not compat.prior_samples_on_device(cfg):
        raise ValueError(f"run_point_episodes: episode {idx} asks for prior samples from a host controller (prior_samples without "
                         "device: true), which a lockstep set cannot serve; use `device: true` or closed_loop.run")
    if not point_priors:
        raise ValueError(f"run_point_episodes: episode {idx} asks for prior samples (prior_samples), which the batched command "
                         "runs only on request (point_priors=True); or use closed_loop.run")


def build_set(episodes, max_ticks=800, trace=False, point_runtime=False, point_priors=False):
    """A PointEpisodeSet of episodes [(config name, overrides, jitter)] that share one world (point_runtime, point_priors: as
    run_point_episodes)."""
    compat.install(force_standins=True)
    items = []
    for idx, (cn, ov, jitter) in enumerate(episodes):
        cfg = compat.make_config(cn, list(ov))
        if cfg.env_type != "point_env":
            raise ValueError(f"run_point_episodes: episode {idx} is {cfg.env_type} (point_env only)")
        if not point_runtime and getattr(cfg, "rollout_arena_spread", None):
            raise ValueError(f"run_point_episodes: episode {idx} asks for an arena per sample (rollout_arena_spread), which the "
                             "batched command does not run (m3_set_point_rollout_scenes: m3_command only); use closed_loop.run")
        _check_episode_priors(cfg, idx, point_priors)
        items.append((cn, list(ov), cfg, jitter))
    return PointEpisodeSet(items, max_ticks, trace, point_runtime=point_runtime, point_priors=point_priors)


def run_point_episodes(episodes, max_ticks=800, trace=False, point_runtime=False, point_priors=False):
    """episodes: [(config name, overrides, jitter)] as closed_loop.run takes them (jitter may be None).  Returns one report
    per episode, in order: the dict closed_loop.run returns (ticks, success, sim_time_s, timeline, final_pos_error,
    dyn_obs_collision_ticks, trace if asked), with the set's tick_ms_p50 / tick_ms_p99 in place of the per-episode
    command_ms_*, and build_s (planner and world construction) / loop_s (ticks 1..) of the set.  Episodes whose worlds
    differ (dt, substeps, device) run as separate sets, one after the other.
    point_runtime=True: episodes may carry `rollout_arena_spread` (an arena per sample of the planner's rollout); without it
    they raise ValueError as before.
    point_priors=True: episodes may carry `prior_samples={..., device: true}` (prior samples from a controller on the device);
    without it, and for a host controller (no `device: true`) always, they raise ValueError."""
    if int(max_ticks) <= 0:
        raise ValueError("run_point_episodes: max_ticks must be > 0")
    compat.install(force_standins=True)
    groups = {}
    for idx, (cn, ov, jitter) in enumerate(episodes):
        cfg = compat.make_config(cn, list(ov))
        if cfg.env_type != "point_env":
            raise ValueError(f"run_point_episodes: episode {idx} is {cfg.env_type} (point_env only)")
        if not point_runtime and getattr(cfg, "rollout_arena_spread", None):
            raise ValueError(f"run_point_episodes: episode {idx} asks for an arena per sample (rollout_arena_spread), which the "
                             "batched command does not run (m3_set_point_rollout_scenes: m3_command only); use closed_loop.run")
        _check_episode_priors(cfg, idx, point_priors)
        key = (float(cfg.isaacgym.dt), int(cfg.isaacgym.substeps), cfg.mppi.device)
        groups.setdefault(key, []).append((idx, (cn, list(ov), cfg, jitter)))
    out = [None] * len(episodes)
    for members in groups.values():
        es = PointEpisodeSet([m for _, m in members], int(max_ticks), bool(trace), point_runtime=point_runtime, point_priors=point_priors)
        try:
            es.run()
            reps = es.reports()
        finally:
            es.close()
        for (idx, _), r in zip(members, reps):
            out[idx] = r
    return out


# ---------------------------------------------- panda_env ----------------------------------------------
class RowSim:
    """What PLANNER_AIF_PANDA touches of a simulator -- step(), env0_link_states_host(), link_row() -- served from one
    episode's row of the set's host copy of the planning view (HipPandaEpisodes.observe): the step update_plan asks for
    was taken by the pre kernel, for all episodes at once."""

    def __init__(self, env_type="panda_env"):
        self.env_type = env_type
        self.rows = None        # [bodies, 13] float32: this tick's rigid-body rows of the episode

    def step(self):
        pass

    def env0_link_states_host(self):
        return self.rows

    def link_row(self, actor_name, link_name):
        return scenes.body_index(self.env_type, actor_name, link_name)


class _PandaSide(_PlannerSide):
    """The planner side of one panda_env episode: Tamp.run_tamp split where the set takes over."""

    def __init__(self, cfg, panda_runtime=False):
        # (a run-time set: simulator and planner as closed_loop.Tamp builds them -- the spread's rows on the simulator, which
        # the planner attached to it takes over; the Objective carries `panda_cost_weights` either way)
        super().__init__(cfg, panda_scenes=compat.rollout_panda_scenes(cfg) if panda_runtime else None)
        self.row_sim = RowSim(cfg.env_type)
        self.rb0 = None

    def push_runtime(self):
        """What the planner's first command would push to its handle -- the workspace of the simulator it follows, that
        simulator's rows, the Objective's weights -- now: a run-time set reads them from the handle at its first observe,
        which comes before that command."""
        mp = self.motion_planner
        mp._bind_world()
        self.objective.push_cost_weights(mp._engine)

    def first(self, dof_state, root_state):
        """Tamp.run_tamp of tick 0 on the planner's own K-env simulator: the state upload, the task planner (its step
        included), then the first command -- the fused / step probe, whose step leg rolls that simulator on and leaves the
        velocity targets it keeps from then on.  Returns the whole plan, or None when the task is done already."""
        self.sim._dof_state[:] = dof_state
        self.sim._root_state[:] = root_state
        self.sim.set_dof_state_tensor(self.sim._dof_state)
        self.sim.set_actor_root_state_tensor(self.sim._root_state)
        self.task_planner.update_plan(self.sim)
        self.rb0 = self.sim.env0_link_states_host().copy()      # (the copy update_plan just read: no further read-back)
        self.motion_planner.update_gripper_command(self.task_planner.task)
        self.objective.update_objective(self.task_planner.task, self.task_planner.curr_goal)
        self.task_success = bool(self.task_planner.check_task_success(self.sim))
        if self.task_success:
            return None
        return self.motion_planner.command(self.sim._dof_state[0])

    def decide(self, rows):
        """Ticks 1..: run_tamp up to its command on this tick's rows; the objective goes to the handle as _push_objective
        sends it inside command().  (get_pull_preference() is not read: nothing in a panda_env tick uses it.)"""
        self.row_sim.rows = rows
        tp = self.task_planner
        tp.update_plan(self.row_sim)
        self.motion_planner.update_gripper_command(tp.task)
        self.objective.update_objective(tp.task, tp.curr_goal)
        self.task_success = bool(tp.check_task_success(self.row_sim))
        if not self.task_success:
            self.motion_planner._push_objective()


class PandaEpisodeSet:
    """One set of config_panda episodes in lockstep: built by the constructor, tick 0 by start() (each planner's first
    command on its own), then tick() while `active`; reports() afterwards.  items: [(config name, overrides, config,
    jitter)] of one world (same dt, substeps, device, cube_on_shelf); jitter: dict(cube=(dx, dy)) or None.
    panda_runtime: the episodes may differ in their workspaces and weights (`panda_scene`, `world_panda_scene`,
    `panda_cost_weights`, `rollout_workspace_spread`) -- row e of the world steps in episode e's world workspace, planner e plans
    in its own (m3_panda_episodes_create_ex with M3_PANDA_EPISODES_RUNTIME, a batch with M3_BATCH_PANDA_RUNTIME)."""

    def __init__(self, items, max_ticks, settle_ticks=0, trace=False, panda_runtime=False):
        import m3p2i_aip.utils.isaacgym_utils.isaacgym_wrapper as wrapper
        t0 = time.perf_counter()
        self.items, self.max_ticks, self.settle_ticks, self.trace = list(items), int(max_ticks), int(settle_ticks), bool(trace)
        self.panda_runtime = bool(panda_runtime)
        cfgs = [cfg for _, _, cfg, _ in self.items]
        c0, n = cfgs[0], len(self.items)
        if self.panda_runtime:
            self.sides = [_PandaSide(cfg, panda_runtime=True) for cfg in cfgs]
            # row e: the workspace closed_loop.run builds episode e's 1-env world with (world_isaacgym_config: `panda_scene`
            # with `world_panda_scene` on top)
            rows = [getattr(compat.world_isaacgym_config(cfg), "panda_scene", None) for cfg in cfgs]
            # (every row's workspace comes from the rows: the wrapper's single workspace, which episode 0's `panda_scene` would
            # set for all rows' views, stays the reference's)
            plain = dataclasses.replace(c0.isaacgym, panda_scene=None)
            self.real = real = wrapper.IsaacGymWrapper(plain, c0.env_type, num_envs=n, viewer=False, device=c0.mppi.device,
                                                       cube_on_shelf=c0.cube_on_shelf, panda_scenes=[r or None for r in rows])
        else:
            self.sides = [_PandaSide(cfg) for cfg in cfgs]
            self.real = real = wrapper.IsaacGymWrapper(c0.isaacgym, c0.env_type, num_envs=n, viewer=False, device=c0.mppi.device,
                                                       cube_on_shelf=c0.cube_on_shelf)
        # closed_loop.run's jitter of its 1-env world, the same torch ops on row e
        ia = int(real._get_actor_index_by_name("cubeA"))
        jittered = False
        for e, (*_, jitter) in enumerate(self.items):
            if jitter and "cube" in jitter:
                real._root_state[e, ia, 0] += float(jitter["cube"][0])
                real._root_state[e, ia, 1] += float(jitter["cube"][1])
                jittered = True
        if jittered:
            real.set_actor_root_state_tensor(real._root_state)
        self.outs = []
        for side in self.sides:
            mp = side.motion_planner
            mp._engine.use_torch_stream()
            mp._ensure_noise()
            out = torch.zeros(mp.T, mp.nu, device=mp.device, dtype=torch.float32)
            mp._engine.set_action_out(out)
            self.outs.append(out)
        real._engine.use_torch_stream()
        if self.panda_runtime:
            for side in self.sides:
                side.push_runtime()
            self.eps = HipPandaEpisodes(real._engine, [s.motion_planner._engine for s in self.sides], self.max_ticks,
                                        settle_ticks=self.settle_ticks, trace=self.trace, panda_runtime=True)
            self.batch = HipBatch(n, device=torch.device(c0.mppi.device).index or 0, panda_runtime=True)
        else:
            self.eps = HipPandaEpisodes(real._engine, [s.motion_planner._engine for s in self.sides], self.max_ticks,
                                        settle_ticks=self.settle_ticks, trace=self.trace)
            self.batch = HipBatch(n, device=torch.device(c0.mppi.device).index or 0)
        self.alive = [True] * n
        self.timelines = [[] for _ in range(n)]
        self.tasks = [[] for _ in range(n)]          # per running tick, for the trace rows
        self.lat, self.split = [], []                # per tick 1..: whole tick; (observe, host planners, act) seconds
        self.build_s = time.perf_counter() - t0
        self.first_s = self.loop_s = 0.0

    def _note(self, e, tick):
        side = self.sides[e]
        task = side.task_planner.task
        if not self.timelines[e] or self.timelines[e][-1][1] != task:
            self.timelines[e].append((tick, task))
        if side.task_success:
            self.alive[e] = False
        else:
            self.tasks[e].append(task)

    def start(self):
        """Tick 0: each planner's first command on its own simulator (the probe), between observe and act_first."""
        t0 = time.perf_counter()
        rb = self.eps.observe().copy()
        for e, side in enumerate(self.sides):
            plan = side.first(self.real._dof_state[e:e + 1], self.real._root_state[e:e + 1])
            # the pre kernel's row against the planner's own simulator after update_plan's step: the same bits, or the set
            # does not reproduce the serial loop
            if side.rb0.tobytes() != rb[e].tobytes():
                raise RuntimeError(f"run_panda_episodes: episode {e}: the planning view differs from the planner's own "
                                   "simulator at tick 0")
            self._note(e, 0)
            if plan is None:
                continue
            if side.motion_planner._fused is not True:
                raise RuntimeError(f"run_panda_episodes: episode {e}'s planner chose the step path at its probe; "
                                   "the batched command runs the fused path only")
            self.outs[e].copy_(plan)
            side.motion_planner._engine.set_action_out(self.outs[e])
        self.eps.act_first([s.sim._engine for s in self.sides], [not a for a in self.alive])
        self._after_act()
        self.first_s = time.perf_counter() - t0

    def _after_act(self):
        if self.eps.ticks_done >= self.max_ticks:        # (the post kernel ended whoever was still running)
            self.alive = [False] * len(self.alive)

    @property
    def active(self):
        return self.eps.active

    def tick(self):
        t0 = time.perf_counter()
        rb = self.eps.observe()
        t1 = time.perf_counter()
        tick = self.eps.ticks_done
        for e, side in enumerate(self.sides):
            if self.alive[e]:
                side.decide(rb[e])
                self._note(e, tick)
        t2 = time.perf_counter()
        self.eps.act(self.batch, [not a for a in self.alive])
        self._after_act()
        t3 = time.perf_counter()
        self.lat.append(t3 - t0)
        self.split.append((t1 - t0, t2 - t1, t3 - t2))

    def run(self):
        self.start()
        t = time.perf_counter()
        while self.active:
            self.tick()
        self.loop_s = time.perf_counter() - t

    def reports(self):
        st, tr = self.eps.status(with_trace=True) if self.trace else (self.eps.status(), None)
        p50 = float(np.percentile(self.lat, 50) * 1e3) if self.lat else 0.0
        p99 = float(np.percentile(self.lat, 99) * 1e3) if self.lat else 0.0
        sp = np.percentile(np.array(self.split), 50, axis=0) * 1e3 if self.split else np.zeros(3)
        reports = []
        for e, ((cn, ov, cfg, _), side) in enumerate(zip(self.items, self.sides)):
            s = st[e]
            if s["phase"] != L.PE_FROZEN:
                raise RuntimeError(f"run_panda_episodes: episode {e} has not ended (reports() before the set ran out)")
            i = s["done_tick"]
            # CPU torch on the f32 positions, as closed_loop.run
            cube, goal = torch.from_numpy(s["cubeA"]), torch.from_numpy(s["cubeB"])
            r = dict(config=cn, overrides=list(ov), K=cfg.mppi.num_samples, T=cfg.mppi.horizon, ticks=i + 1,
                     success=s["success"], transport="batched", sim_time_s=(i + 1) * cfg.isaacgym.dt,
                     timeline=list(self.timelines[e]), tick_ms_p50=p50, tick_ms_p99=p99,
                     observe_ms_p50=float(sp[0]), host_ms_p50=float(sp[1]), act_ms_p50=float(sp[2]),
                     build_s=self.build_s, first_s=self.first_s, loop_s=self.loop_s,
                     cube_to_goal_xy=float(torch.norm(cube[:2] - goal[:2])), cube_height_above_goal=float(cube[2] - goal[2]),
                     lanes_per_sample_used=side.motion_planner._engine.panda_lanes_per_sample_used())
            if self.panda_runtime:      # (what closed_loop.run reports of a planner with a workspace or weights of its own)
                eng = side.motion_planner._engine
                r["m3_panda_scene_instance_used"] = eng.panda_scene_instance_used()
                r["m3_panda_weighted_cost_instance_used"] = eng.panda_weighted_cost_instance_used()
            if self.trace:
                rows = i if s["success"] else i + 1      # (no row for the success tick: the serial loop ends before it)
                path, full = [], []
                for t in range(rows):
                    row, task = tr[t, e], self.tasks[e][t]
                    dof = row[L.PE_TR_DOF:L.PE_TR_ROOT]
                    act = row[L.PE_TR_ACTION:L.PE_TR_HAND]
                    path.append([task] + row[L.PE_TR_HAND:L.PE_TR_CUBE].tolist() + row[L.PE_TR_CUBE:L.PE_TR_CUBE + 7].tolist() +
                                dof[[14, 16]].tolist() + act[7:9].tolist())
                    full.append(dict(tick=t, task=task, dof_state=dof.tolist(),
                                     root_state=row[L.PE_TR_ROOT:L.PE_TR_ACTION].reshape(-1, 13).tolist(), action=act.tolist()))
                r["trace"] = path
                if full:
                    r["full"] = full
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


def _panda_groups(episodes, who, panda_runtime=False):
    compat.install(force_standins=True)
    groups = {}
    for idx, (cn, ov, jitter) in enumerate(episodes):
        cfg = compat.make_config(cn, list(ov))
        if cfg.env_type != "panda_env":
            raise ValueError(f"{who}: episode {idx} is {cfg.env_type} (panda_env only)")
        # the set's one N-env world is built from its first episode's config and every row steps in that handle's scene: an
        # episode's own workspace -- its masses included -- would be dropped, so the keys are refused here, not ignored
        # (a run-time set carries them: a workspace per row of the world, each planner's own on its handle)
        for key in () if panda_runtime else ("panda_scene", "world_panda_scene"):
            if getattr(cfg, key):
                raise ValueError(f"{who}: episode {idx}: `{key}` asks for a workspace of its own (m3_set_panda_scene), which the "
                                 "lockstep panda episodes do not run (one world handle, one scene); use closed_loop.run")
        if getattr(cfg, "panda_prior_samples", None):    # (with or without the run-time section: no table entry carries priors)
            raise ValueError(f"{who}: episode {idx}: `panda_prior_samples` asks for prior samples (m3_set_panda_prior_samples), "
                             "which the lockstep panda episodes do not run (their planners' batched command carries no table of "
                             "priors); use closed_loop.run")
        if not panda_runtime and getattr(cfg, "rollout_workspace_spread", None):
            raise ValueError(f"{who}: episode {idx}: `rollout_workspace_spread` asks for a workspace per sample "
                             "(m3_set_panda_rollout_scenes), which the lockstep panda episodes do not run (their planners' batched "
                             "command carries one scene); use closed_loop.run")
        if not panda_runtime and getattr(cfg, "panda_cost_weights", None):
            raise ValueError(f"{who}: episode {idx}: `panda_cost_weights` asks for cost weights of its own (m3_set_panda_cost_weights), "
                             "which the lockstep panda episodes do not run (their planners' batched command forms the literal "
                             "cost); use closed_loop.run")
        key = (float(cfg.isaacgym.dt), int(cfg.isaacgym.substeps), cfg.mppi.device, bool(cfg.cube_on_shelf))
        groups.setdefault(key, []).append((idx, (cn, list(ov), cfg, jitter)))
    return groups


def build_panda_set(episodes, max_ticks=600, settle_ticks=0, trace=False, panda_runtime=False):
    """A PandaEpisodeSet of episodes [(config name, overrides, jitter)] that share one world (panda_runtime: as
    run_panda_episodes)."""
    groups = _panda_groups(episodes, "build_panda_set", panda_runtime)
    if len(groups) != 1:
        raise ValueError("build_panda_set: the episodes' worlds differ (dt, substeps, device, cube_on_shelf)")
    return PandaEpisodeSet([m for _, m in next(iter(groups.values()))], max_ticks, settle_ticks, trace, panda_runtime=panda_runtime)


def run_panda_episodes(episodes, max_ticks=600, settle_ticks=0, trace=False, panda_runtime=False):
    """episodes: [("config_panda", overrides, jitter)] as closed_loop.run takes them (jitter: dict(cube=(dx, dy)) or None).
    Returns one report per episode, in order: what closed_loop.run(cn, overrides, ticks=max_ticks, jitter=jitter,
    settle_ticks=settle_ticks, trace=trace) returns, bit for bit (ticks, success, sim_time_s, timeline, cube_to_goal_xy,
    cube_height_above_goal, trace and full rows if asked), with the set's tick_ms_p50 / tick_ms_p99 in place of the
    per-episode command_ms_*, their split (observe_ms_p50, host_ms_p50, act_ms_p50), build_s / first_s / loop_s of the set
    (construction, tick 0, ticks 1..) and lanes_per_sample_used (the kernel form of the planner's last command).  Episodes
    whose worlds differ run as separate sets, one after the other.  A lone episode is better served by closed_loop.run.
    panda_runtime=True: the episodes may carry `panda_scene`, `world_panda_scene`, `panda_cost_weights` and
    `rollout_workspace_spread` overrides, each its own (refused with a ValueError otherwise) -- the reports still equal
    closed_loop.run's bit for bit and add m3_panda_scene_instance_used / m3_panda_weighted_cost_instance_used; the episodes
    still group by (dt, substeps, device, cube_on_shelf) only."""
    if int(max_ticks) <= 0:
        raise ValueError("run_panda_episodes: max_ticks must be > 0")
    if int(settle_ticks) < 0:
        raise ValueError("run_panda_episodes: settle_ticks must be >= 0")
    out = [None] * len(episodes)
    for members in _panda_groups(episodes, "run_panda_episodes", panda_runtime).values():
        es = PandaEpisodeSet([m for _, m in members], int(max_ticks), int(settle_ticks), bool(trace), panda_runtime=panda_runtime)
        try:
            es.run()
            reps = es.reports()
        finally:
            es.close()
        for (idx, _), r in zip(members, reps):
            out[idx] = r
    return out
