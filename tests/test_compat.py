"""The reference's scripts import through `m3p2i_aip_amd.compat`."""
import sys

import pytest


def test_reference_import_names_resolve():
    from m3p2i_aip_amd import compat
    compat.install(force_standins=True)
    from isaacgym import gymtorch  # noqa: F401
    import hydra, zerorpc  # noqa: F401,E401
    from m3p2i_aip.planners.motion_planner import m3p2i
    from m3p2i_aip.planners.task_planner import task_planner
    from m3p2i_aip.config.config_store import ExampleConfig
    import m3p2i_aip.utils.isaacgym_utils.isaacgym_wrapper as wrapper
    from m3p2i_aip.planners.motion_planner.cost_functions import Objective
    from m3p2i_aip.utils.data_transfer import bytes_to_torch, torch_to_bytes
    from m3p2i_aip.utils.skill_utils import check_and_apply_suction, time_tracking  # noqa: F401
    import torch
    assert hasattr(m3p2i, "M3P2I") and hasattr(wrapper, "IsaacGymWrapper") and Objective and ExampleConfig
    assert torch.equal(bytes_to_torch(torch_to_bytes(torch.arange(5.0))), torch.arange(5.0))
    cfg = compat.make_config("config_point", ["task=push_pull", "multi_modal=True", "goal=[-1, -1]",
                                               "mppi.num_samples=64"])
    assert cfg.multi_modal is True and cfg.goal == [-1, -1] and cfg.mppi.num_samples == 64
    assert cfg.mppi.horizon == 15 and cfg.isaacgym.dt == 0.05 and cfg.kp_suction == 400
    p = compat.make_config("config_panda")
    assert p.env_type == "panda_env" and p.mppi.nx == 18 and p.isaacgym.dt == 0.01 and p.pre_height_diff == 0.05
    cfg.mppi.device = "cpu"   # PLANNER_SIMPLE only builds the goal tensor (no GPU in this container)
    tp = task_planner.set_task_planner(cfg)
    assert tp.task == "push_pull" and tuple(tp.curr_goal.tolist()) == (-1.0, -1.0)
    with pytest.raises(AttributeError):
        compat.make_config("config_point", ["no_such_key=1"])


def test_reference_script_entry_points_on_the_shims(monkeypatch):
    """What scripts/reactive_tamp.py and scripts/sim.py build at module level, on the shims: a hydra-decorated entry point
    (version_base=None, the package's config folder, config_point) that composes its config from the command line's
    key=value overrides, the skill_utils / zerorpc names sim.py calls, and the planner process's constructor -- the
    wrapper of cfg.mppi.num_samples environments on cfg.mppi.device -- failing loudly when there is no GPU."""
    from m3p2i_aip_amd import compat
    from m3p2i_aip_amd._lib import M3Error
    compat.install(force_standins=True)
    import hydra
    import zerorpc
    import torch
    from m3p2i_aip.config.config_store import ExampleConfig
    from m3p2i_aip.utils.skill_utils import check_and_apply_suction, time_tracking
    import m3p2i_aip.utils.isaacgym_utils.isaacgym_wrapper as wrapper

    @hydra.main(version_base=None, config_path="../src/m3p2i_aip/config", config_name="config_point")
    def entry(cfg: ExampleConfig):
        return cfg

    monkeypatch.setattr(sys, "argv", ["reactive_tamp.py", "task=push_pull", "mppi.num_samples=64"])
    cfg = entry()
    assert cfg.env_type == "point_env" and cfg.task == "push_pull" and cfg.mppi.num_samples == 64
    monkeypatch.setattr(sys, "argv", ["sim.py", "-cn", "config_panda"])
    assert entry().env_type == "panda_env"
    assert check_and_apply_suction is compat.check_and_apply_suction and time_tracking is compat.time_tracking
    assert callable(zerorpc.Server) and hasattr(zerorpc.Client(), "connect")
    if not torch.cuda.is_available():
        with pytest.raises(M3Error):
            wrapper.IsaacGymWrapper(cfg.isaacgym, cfg.env_type, num_envs=cfg.mppi.num_samples, viewer=False,
                                    device=cfg.mppi.device, cube_on_shelf=cfg.cube_on_shelf)


@pytest.mark.gpu
def test_reactive_tamp_wiring_through_compat_names_gpu():
    """reactive_tamp.py:22-61 written against the reference's module names, on the GPU."""
    import torch
    from m3p2i_aip_amd import compat
    compat.install(force_standins=True)
    from m3p2i_aip.planners.motion_planner import m3p2i
    from m3p2i_aip.planners.task_planner import task_planner
    import m3p2i_aip.utils.isaacgym_utils.isaacgym_wrapper as wrapper
    from m3p2i_aip.planners.motion_planner.cost_functions import Objective
    from m3p2i_aip.utils.data_transfer import bytes_to_torch, torch_to_bytes
    cfg = compat.make_config("config_point", ["task=push", "goal=[-1, -1]", "mppi.num_samples=256",
                                               "mppi.horizon=16"])

    class R:
        def __init__(self):
            self.sim = wrapper.IsaacGymWrapper(cfg.isaacgym, cfg.env_type, num_envs=cfg.mppi.num_samples,
                                               viewer=False, device=cfg.mppi.device, cube_on_shelf=cfg.cube_on_shelf)
            self.objective = Objective(cfg)
            self.task_planner = task_planner.set_task_planner(cfg)
            self.motion_planner = m3p2i.M3P2I(cfg, dynamics=self.dynamics, running_cost=self.running_cost)

        def dynamics(self, _, u, t=None):
            self.sim.set_dof_velocity_target_tensor(u)
            self.sim.step()
            return torch.stack([self.sim.robot_pos[:, 0], self.sim.robot_vel[:, 0],
                                self.sim.robot_pos[:, 1], self.sim.robot_vel[:, 1]], dim=1), u

        def running_cost(self, _):
            return self.objective.compute_cost(self.sim)

    r = R()
    real = wrapper.IsaacGymWrapper(cfg.isaacgym, cfg.env_type, num_envs=1, device=cfg.mppi.device)
    d0 = None
    for i in range(40):   # sim.py:38-55 + reactive_tamp.py:43-61, in-process
        r.sim._dof_state[:] = bytes_to_torch(torch_to_bytes(real._dof_state))
        r.sim._root_state[:] = bytes_to_torch(torch_to_bytes(real._root_state))
        r.sim.set_dof_state_tensor(r.sim._dof_state)
        r.sim.set_actor_root_state_tensor(r.sim._root_state)
        r.task_planner.update_plan(r.sim)
        r.objective.update_objective(r.task_planner.task, r.task_planner.curr_goal)
        r.motion_planner.get_pull_preference()
        if r.task_planner.check_task_success(r.sim):
            break
        action = r.motion_planner.command(r.sim._dof_state[0])[0]
        real.set_dof_velocity_target_tensor(action.view(1, 2))
        real.step()
        box = real.get_actor_position_by_name("box")[0, :2]
        d = torch.norm(box - r.task_planner.curr_goal).item()
        d0 = d if d0 is None else d0
    assert r.motion_planner.probe_result["fused"] is True
    assert d < d0 - 0.3, (d0, d)   # the closed loop pushes the box towards the goal


@pytest.mark.gpu
def test_panda_reactive_tamp_with_aif_task_planner_gpu():
    """reactive_tamp.py:22-88 for config_panda through the reference's module names: the
    active-inference task planner picks reach -> (pick) from the wrapper's link poses, M3P2I gets
    the gripper command + objective, and the 1-env world driven by the returned action brings
    the gripper towards the cube."""
    import torch
    from m3p2i_aip_amd import compat
    compat.install(force_standins=True)
    from m3p2i_aip.planners.motion_planner import m3p2i
    from m3p2i_aip.planners.task_planner import task_planner
    import m3p2i_aip.utils.isaacgym_utils.isaacgym_wrapper as wrapper
    from m3p2i_aip.planners.motion_planner.cost_functions import Objective
    cfg = compat.make_config("config_panda", ["mppi.num_samples=512"])

    class R:
        def __init__(self):
            self.sim = wrapper.IsaacGymWrapper(cfg.isaacgym, cfg.env_type, num_envs=cfg.mppi.num_samples,
                                               viewer=False, device=cfg.mppi.device, cube_on_shelf=cfg.cube_on_shelf)
            self.objective = Objective(cfg)
            self.task_planner = task_planner.set_task_planner(cfg)
            self.motion_planner = m3p2i.M3P2I(cfg, dynamics=self.dynamics, running_cost=self.running_cost)

        def dynamics(self, _, u, t=None):
            self.sim.set_dof_velocity_target_tensor(u)
            self.sim.step()
            return torch.stack([self.sim.robot_pos[:, 0], self.sim.robot_vel[:, 0],
                                self.sim.robot_pos[:, 1], self.sim.robot_vel[:, 1]], dim=1), u

        def running_cost(self, _):
            return self.objective.compute_cost(self.sim)

    r = R()
    assert isinstance(r.task_planner, task_planner.PLANNER_AIF_PANDA)
    real = wrapper.IsaacGymWrapper(cfg.isaacgym, cfg.env_type, num_envs=1, device=cfg.mppi.device,
                                   cube_on_shelf=cfg.cube_on_shelf)

    def reach_dist():
        ee = (real.get_actor_link_by_name("panda", "panda_leftfinger")[0, :3]
              + real.get_actor_link_by_name("panda", "panda_rightfinger")[0, :3]) / 2
        return torch.norm(ee - real.get_actor_link_by_name("cubeA", "box")[0, :3]).item()

    d0 = reach_dist()
    tasks = []
    for i in range(150):
        r.sim._dof_state[:] = real._dof_state
        r.sim._root_state[:] = real._root_state
        r.sim.set_dof_state_tensor(r.sim._dof_state)
        r.sim.set_actor_root_state_tensor(r.sim._root_state)
        r.task_planner.update_plan(r.sim)                                  # tamp_interface()
        r.motion_planner.update_gripper_command(r.task_planner.task)
        r.objective.update_objective(r.task_planner.task, r.task_planner.curr_goal)
        r.motion_planner.get_pull_preference()
        tasks.append(r.task_planner.task)
        if r.task_planner.check_task_success(r.sim):
            break
        action = r.motion_planner.command(r.sim._dof_state[0])[0]
        assert action.shape == (9,) and torch.isfinite(action).all()
        real.set_dof_velocity_target_tensor(action.view(1, 9))
        real.step()
        if tasks[-1] == "pick":
            break
    d1 = reach_dist()
    print("panda closed loop: ticks", len(tasks), "tasks", sorted(set(tasks)), "reach dist", d0, "->", d1)
    assert tasks[0] == "reach" and set(tasks) <= {"reach", "pick"}
    assert d1 < 0.5 * d0, (d0, d1)
    assert r.motion_planner.probe_result["fused"] is True


@pytest.mark.gpu
def test_device_suction_skill_matches_reference_golden_gpu(golden):
    """calculate_suction / check_suction_condition / check_and_apply_suction of the 1-env real world
    (utils/skill_utils.py:36-94, called by scripts/sim.py:41-49) run as a HIP kernel on the wrapper's
    environments (m3_sim_suction_forces, m3_sim_check_and_apply_suction): forces and conditions against
    values recorded from the reference's own functions (make_golden.py g7_skill)."""
    import types
    import numpy as np
    import torch
    from m3p2i_aip_amd import compat, _lib as L
    from m3p2i_aip_amd import isaacgym_wrapper as wrapper
    robot, box = golden["g7s_robot"], golden["g7s_box"]
    K = robot.shape[0]
    cfg = types.SimpleNamespace(task="pull", suction_active=True, kp_suction=400)

    def world(n, rows):
        sim = wrapper.IsaacGymWrapper(wrapper.IsaacGymConfig(dt=0.05), "point_env", num_envs=n, device="cuda:0")
        sim._dof_state[:, 0] = torch.tensor(robot[rows, 0], device="cuda:0")
        sim._dof_state[:, 2] = torch.tensor(robot[rows, 1], device="cuda:0")
        bi = int(sim._get_actor_index_by_name("box"))
        sim._root_state[:, bi, 0:2] = torch.tensor(box[rows], device="cuda:0")
        sim.set_dof_state_tensor(sim._dof_state)
        sim.set_actor_root_state_tensor(sim._root_state)
        return sim

    sim = world(K, slice(None))                                   # K > 1: threshold 1.8
    f = compat.calculate_suction(cfg, sim).cpu().numpy()
    np.testing.assert_allclose(f, golden["g7s_forces_K64"], rtol=1e-5, atol=1e-3)
    sim.stop_sim()
    hits = 0
    for i in range(0, K, 3):                                      # 1-env worlds: threshold 1.5 + the condition
        s1 = world(1, slice(i, i + 1))
        np.testing.assert_allclose(compat.calculate_suction(cfg, s1).cpu().numpy()[0], golden["g7s_forces_K1"][i],
                                   rtol=1e-5, atol=1e-3)
        a = torch.tensor(golden["g7s_action"][i], device="cuda:0")
        cond = compat.check_suction_condition(cfg, s1, a)
        assert cond == bool(golden["g7s_condition"][i]), i
        for gate in (True, torch.ones(1, dtype=torch.int32, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0")):
            s1._engine.buffer(L.BUF_SIM_WORLD)[18:22].zero_()
            cfg.suction_active = gate
            compat.check_and_apply_suction(cfg, s1, a)            # stages the pair as the next step's external force
            pend = s1._engine.buffer(L.BUF_SIM_WORLD)[18:22, 0].cpu().numpy()
            on = cond and (gate is True or bool(gate.item()))
            want = golden["g7s_forces_K1"][i]
            exp = np.concatenate([want[-1, :2], want[int(s1._get_actor_index_by_name("box")), :2]]) if on else np.zeros(4)
            np.testing.assert_allclose(pend, exp, rtol=1e-5, atol=1e-3)
        cfg.suction_active = True
        hits += cond
        s1.stop_sim()
    assert 0 < hits < len(range(0, K, 3))
