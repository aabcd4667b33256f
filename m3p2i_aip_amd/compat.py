"""Compatibility layer: lets the reference's `scripts/reactive_tamp.py` (and `scripts/sim.py`)
import and run unchanged on this package.

`install()` registers this package's classes under the module names the scripts import
(`reactive_tamp.py:1-8`, `sim.py:1-6`).  Nothing of the reference is copied and Isaac Gym is
not needed.  Launcher / RPC pieces (hydra, zerorpc) are outside the hot path (SURVEY.md
section 8(f)); when the real packages are absent, small stand-ins cover exactly the calls the
scripts make (`hydra.main` composition of config_point / config_panda + key=value overrides;
`zerorpc.Server / Client` over TCP + msgpack: m3p2i_aip_amd/rpc.py).

Host-side helpers restated here (all O(1) per command, no data parallelism):
  PLANNER_SIMPLE / PLANNER_AIF_PANDA / AiAgent / adapt_act_sel / MDPIsCubeAtReal
                            planners/task_planner/*.py  (-> m3p2i_aip_amd/task_planner.py)
  torch_to_bytes / bytes_to_torch   utils/data_transfer.py:4-12
  calculate_suction / check_suction_condition / check_and_apply_suction
                            utils/skill_utils.py:36-94 -> HIP kernel k_sim_suction (device, no host sync)
  time_tracking             utils/skill_utils.py:25-33
  ExampleConfig defaults    config/config_point.yaml, config_panda.yaml, mppi/*.yaml,
                            isaacgym/*.yaml, config/config_store.py:7-29
"""
from __future__ import annotations

import io
import sys
import time
import types
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

from . import cost_functions, isaacgym_wrapper, planner, task_planner


# ------------------------------------------------------------------ data_transfer.py:4-12
def torch_to_bytes(t) -> bytes:
    """data_transfer.py:4-7: a torch.save archive.  Small plain tensors -- the states and the action of every tick -- through
    blobs.TensorBlobCodec (the same archive, written by patching a copy: ~10 us instead of ~170)."""
    from .blobs import CODEC
    return CODEC.save(t)


def bytes_to_torch(b: bytes):
    """data_transfer.py:9-12.  The blob comes off a network socket: weights_only=True restricts the unpickler to
    tensors and plain containers (bool / int / float / str / list / dict), which is all the scripts exchange.  An archive that
    equals a known one of a small plain tensor everywhere but in its payload is read by lifting the payload out (CRC checked)."""
    from .blobs import CODEC
    try:
        return CODEC.load(b)
    except TypeError:       # torch < 1.13 has no weights_only: refuse rather than fall back to the full unpickler
        raise RuntimeError("bytes_to_torch needs torch >= 1.13 (torch.load(weights_only=True)); this torch is "
                           + torch.__version__) from None


# ------------------------------------------------------------------ task_planner.py (module)
PLANNER_SIMPLE = task_planner.PLANNER_SIMPLE
PLANNER_AIF_PANDA = task_planner.PLANNER_AIF_PANDA
set_task_planner = task_planner.set_task_planner


# ------------------------------------------------------------------ skill_utils.py:25-94
# The suction skill of the 1-env "real world" (scripts/sim.py:41-49).  The geometry lives in the HIP
# library (m3_sim_suction_forces / m3_sim_check_and_apply_suction, csrc/rollout_point.hip:
# k_sim_suction); what stays on the host is the part that only reads the config.
def _device_gate(cfg):
    """cfg.suction_active handed over as a device tensor (planner.pull_preference_tensor()): the kernel
    reads it, the host never does."""
    g = cfg.suction_active
    return g if (torch.is_tensor(g) and g.is_cuda) else None


def _suction_enabled(cfg):
    if cfg.task not in ("pull", "push_pull"):
        return False
    return True if _device_gate(cfg) is not None else bool(cfg.suction_active)


def calculate_suction(cfg, sim):
    """[num_envs, bodies_per_env, 3] suction forces on the box and the robot's last link."""
    return sim._engine.sim_suction_forces(cfg.kp_suction)


def check_suction_condition(cfg, sim, action):
    """bool for env 0 (one host sync, as the reference's .item())."""
    if not _suction_enabled(cfg):
        return False
    g = _device_gate(cfg)
    return bool(sim._engine.sim_check_and_apply_suction(action, cfg.kp_suction, apply=False, want_flags=True,
                                                        enabled=None if g is None else g.to(torch.int32).reshape(1))[0].item())


def check_and_apply_suction(cfg, sim, action):
    """Stages the suction pair for the next sim.step() wherever the condition holds; enqueued on the
    stream, nothing is read back (the reference's "suction!!!" / "no suction..." prints are dropped)."""
    if _suction_enabled(cfg):
        g = _device_gate(cfg)
        sim._engine.sim_check_and_apply_suction(action, cfg.kp_suction, apply=True,
                                                enabled=None if g is None else g.to(torch.int32).reshape(1))


def time_tracking(t, cfg):
    actual_dt = time.time() - t
    if cfg.isaacgym.dt / actual_dt > 1.0:
        time.sleep(cfg.isaacgym.dt - actual_dt)
    return time.time()


# ------------------------------------------------------------------ config_store.py + yaml values
@dataclass
class ExampleConfig:
    mppi: planner.MPPIConfig
    isaacgym: isaacgym_wrapper.IsaacGymConfig
    env_type: str = "point_env"
    task: str = "push"
    goal: List[float] = field(default_factory=lambda: [-3.75, -3.75])
    kp_suction: int = 0
    suction_active: bool = False
    multi_modal: bool = False
    pre_height_diff: float = 0.0
    cube_on_shelf: bool = False
    render: bool = False
    n_steps: int = 0
    nx: int = 4
    avoid_dyn_obs: bool = False     # EXTENSION (not a key of the reference's config_store.py): cost_functions.Objective
    cost_weights: Optional[Dict[str, float]] = None   # EXTENSION, point_env: e.g. `cost_weights={push_align: 2.5}`; None = the
                                                      # reference's literals (cost_functions.Objective, _lib.COST_WEIGHT_DEFAULTS)
    panda_cost_weights: Optional[Dict[str, float]] = None   # EXTENSION, panda_env: e.g. `panda_cost_weights={pick_ori: 25.0}`;
                                                            # None = the reference's literals (_lib.PANDA_COST_WEIGHT_DEFAULTS)
    point_scene: Optional[Dict[str, float]] = None    # EXTENSION, point_env: field overrides of the arena, e.g.
                                                      # `point_scene={obs_x: -1.0, wall: 2.95}` (_lib.POINT_SCENE_DEFAULTS); the
                                                      # wrappers built from cfg.isaacgym set it on their engines, the planners
                                                      # that attach to them take it over
    world_point_scene: Optional[Dict[str, float]] = None   # EXTENSION, point_env: field overrides of the REAL world only, on top
                                                           # of point_scene (model mismatch: the planner and its K-env simulator
                                                           # keep point_scene); world_isaacgym_config applies it
    panda_scene: Optional[Dict[str, object]] = None    # EXTENSION, panda_env: field overrides of the workspace, e.g.
                                                       # `panda_scene={table: [0, 0, 0.99, 0.6, 0.6, 0.025], mu: 0.5}`
                                                       # (_lib.PANDA_SCENE_DEFAULTS); wrappers and planners as for point_scene
    world_panda_scene: Optional[Dict[str, object]] = None   # EXTENSION, panda_env: field overrides of the REAL world only, on
                                                            # top of panda_scene (the planner keeps panda_scene)
    rollout_arena_spread: Optional[Dict[str, object]] = None   # EXTENSION, point_env: `rollout_arena_spread={spread: 0.3, seed: 1,
                                                               # fields: [box_m, box_mu_g, mu_rb]}` -- the planner's K rollouts
                                                               # each in an arena of their own around point_scene (the samples
                                                               # 0, K / 2 and K - 1 stay nominal); rollout_point_scenes builds
                                                               # the rows the planner's K-env simulator carries
    rollout_arena_groups: Optional[Dict[str, object]] = None   # EXTENSION, point_env: `rollout_arena_groups={models: 4, spread: 0.3,
                                                               # seed: 1, fields: [...], worst: 1.0}` -- every control sequence
                                                               # of the planner rolled out in the same M arenas around
                                                               # point_scene, the M costs aggregated (mean of the worst share)
                                                               # ahead of the update: groups.grouped_layout, MPPI.set_sample_groups;
                                                               # exclusive with rollout_arena_spread
    prior_samples: Optional[Dict[str, object]] = None   # EXTENSION, point_env: `prior_samples={controller: go_to, n: 4}` -- n of the
                                                        # K rollouts take the proposals of a host-side ancillary controller
                                                        # (priors.go_to / priors.push_behind), set before every command
                                                        # (tools/closed_loop.py; MPPI.set_prior_samples)
    panda_prior_samples: Optional[Dict[str, object]] = None   # EXTENSION, panda_env: `panda_prior_samples={controller: hold, n: 4}`
                                                              # or `{controller: joint_go_to, n: 4, q: [7 or 9 joint targets]}` -- n
                                                              # of the K rollouts take the proposals of a host-side ancillary
                                                              # controller (priors.hold / priors.joint_go_to), set before every
                                                              # command (tools/closed_loop.py; MPPI.set_panda_prior_samples)
    rollout_workspace_spread: Optional[Dict[str, object]] = None   # EXTENSION, panda_env: `rollout_workspace_spread={spread: 0.3,
                                                                   # seed: 1, fields: [cube_m, mu, obs_m]}` -- the planner's K
                                                                   # rollouts each in a workspace of their own around panda_scene
                                                                   # (the samples 0, K / 2 and K - 1 stay nominal);
                                                                   # rollout_panda_scenes builds the rows


def make_config(config_name="config_point", overrides=()):
    """config/config_{point,panda}.yaml + the mppi/ and isaacgym/ groups they compose, then
    `key=value` / `group.key=value` overrides as on the reference's command line."""
    import yaml
    if config_name == "config_point":
        m = planner.MPPIConfig(mppi_mode="halton-spline", sampling_method="halton", num_samples=200,
                               horizon=15, nx=4, device="cuda:0", lambda_=0.5, u_min=[-3.0, -3.0],
                               u_max=[3.0, 3.0], noise_sigma=[[3.0, 0.0], [0.0, 3.0]], u_per_command=15,
                               sample_null_action=True, filter_u=True, use_priors=False)
        g = isaacgym_wrapper.IsaacGymConfig(dt=0.05, spacing=10)
        cfg = ExampleConfig(mppi=m, isaacgym=g, env_type="point_env", task="push", goal=[-3.75, -3.75],
                            kp_suction=400, suction_active=True, multi_modal=False)
    elif config_name == "config_panda":
        sig = [[0.0] * 9 for _ in range(9)]
        for i in range(7):
            sig[i][i] = 10.0
        sig[7][7] = sig[8][8] = 0.8
        m = planner.MPPIConfig(mppi_mode="halton-spline", sampling_method="halton", num_samples=200,
                               horizon=12, nx=18, device="cuda:0", u_min=[-2.0] * 7 + [-1.5] * 2,
                               u_max=[2.0] * 7 + [1.5] * 2, lambda_=0.05, noise_sigma=sig, u_per_command=12,
                               sample_null_action=True, filter_u=True, use_priors=False)
        g = isaacgym_wrapper.IsaacGymConfig(dt=0.01, spacing=2, camera_pos=[0, 1.5, 2.8], camera_target=[0, 0, 1])
        cfg = ExampleConfig(mppi=m, isaacgym=g, env_type="panda_env", task="reactive_pick", goal=[0.0] * 7,
                            multi_modal=False, pre_height_diff=0.05, cube_on_shelf=False)
    else:
        raise ValueError(f"unknown config {config_name!r}")
    for ov in overrides:
        key, _, val = ov.partition("=")
        obj = cfg
        parts = key.split(".")
        for p in parts[:-1]:
            obj = getattr(obj, p)
        if not hasattr(obj, parts[-1]):
            raise AttributeError(f"unknown config key {key!r}")
        setattr(obj, parts[-1], yaml.safe_load(val))
    if cfg.point_scene:
        if cfg.env_type != "point_env":
            raise ValueError("point_scene: point_env only")
        cfg.isaacgym.point_scene = dict(cfg.point_scene)   # (the wrappers are built from cfg.isaacgym)
    if cfg.world_point_scene:
        if cfg.env_type != "point_env":
            raise ValueError("world_point_scene: point_env only")
        cfg.world_point_scene = dict(cfg.world_point_scene)
    if cfg.rollout_arena_spread:
        cfg.rollout_arena_spread = dict(cfg.rollout_arena_spread)
        _check_rollout_arena_spread(cfg)
    if cfg.rollout_arena_groups:
        cfg.rollout_arena_groups = dict(cfg.rollout_arena_groups)
        check_rollout_arena_groups(cfg)
    if cfg.prior_samples:
        cfg.prior_samples = dict(cfg.prior_samples)
        check_prior_samples(cfg)
    if cfg.panda_prior_samples:
        cfg.panda_prior_samples = dict(cfg.panda_prior_samples)
        check_panda_prior_samples(cfg)
    if cfg.rollout_workspace_spread:
        cfg.rollout_workspace_spread = dict(cfg.rollout_workspace_spread)
        _check_rollout_workspace_spread(cfg)
    for key in ("panda_scene", "world_panda_scene"):
        given = getattr(cfg, key)
        if given:
            if cfg.env_type != "panda_env":
                raise ValueError(f"{key}: panda_env only")
            from ._lib import panda_scene_fields
            try:
                panda_scene_fields(given)     # (unknown fields, wrong lengths)
            except ValueError as e:
                raise ValueError(f"{key}: {e}") from None
            setattr(cfg, key, dict(given))
    if cfg.panda_scene:
        cfg.isaacgym.panda_scene = dict(cfg.panda_scene)   # (the wrappers are built from cfg.isaacgym)
    if cfg.panda_cost_weights:
        if cfg.env_type != "panda_env":
            raise ValueError("panda_cost_weights: panda_env only")
        from ._lib import PANDA_COST_WEIGHT_DEFAULTS
        cfg.panda_cost_weights = dict(cfg.panda_cost_weights)
        unknown = sorted(set(cfg.panda_cost_weights) - set(PANDA_COST_WEIGHT_DEFAULTS))
        if unknown:
            raise ValueError(f"panda_cost_weights: unknown panda cost weight(s) {unknown}: one of {list(PANDA_COST_WEIGHT_DEFAULTS)}")
    return cfg


def check_prior_samples(cfg):
    """the parsed `prior_samples` key as (controller name, n); ValueError for what it cannot mean"""
    from . import _lib, priors
    given = dict(cfg.prior_samples)
    if cfg.env_type != "point_env":
        raise ValueError("prior_samples: point_env only")
    unknown = sorted(set(given) - {"controller", "n", "device"})
    if unknown or given.get("controller") not in priors.CONTROLLERS:
        raise ValueError(f"prior_samples: {{controller: {' | '.join(priors.CONTROLLERS)}, n: 4}} (unknown key(s) {unknown})")
    n = int(given.get("n", 4))
    if not 1 <= n <= min(_lib.MAX_PRIOR_SAMPLES, int(cfg.mppi.num_samples) // 2 - 2):
        raise ValueError(f"prior_samples: n {n} is not in 1 .. min({_lib.MAX_PRIOR_SAMPLES}, num_samples / 2 - 2)")
    if "device" in given:
        if not isinstance(given["device"], bool):
            raise ValueError(f"prior_samples: device is true or false, not {given['device']!r}")
        if given["device"] and n > _lib.MAX_PRIOR_CONTROLLER_SEQS:
            raise ValueError(f"prior_samples: device: true takes n in 1 .. {_lib.MAX_PRIOR_CONTROLLER_SEQS}, not {n}")
    return str(given["controller"]), n


def check_panda_prior_samples(cfg):
    """the parsed `panda_prior_samples` key as (controller name, n, q: the joint targets of joint_go_to or None); ValueError for
    what it cannot mean"""
    from . import _lib, priors
    given = dict(cfg.panda_prior_samples)
    if cfg.env_type != "panda_env":
        raise ValueError("panda_prior_samples: panda_env only")
    unknown = sorted(set(given) - {"controller", "n", "q"})
    if unknown or given.get("controller") not in priors.PANDA_CONTROLLERS:
        raise ValueError(f"panda_prior_samples: {{controller: {' | '.join(priors.PANDA_CONTROLLERS)}, n: 4, q: [...]}} "
                         f"(unknown key(s) {unknown})")
    n = int(given.get("n", 4))
    if not 1 <= n <= min(_lib.MAX_PRIOR_SAMPLES, int(cfg.mppi.num_samples) // 2 - 2):
        raise ValueError(f"panda_prior_samples: n {n} is not in 1 .. min({_lib.MAX_PRIOR_SAMPLES}, num_samples / 2 - 2)")
    name, q = str(given["controller"]), given.get("q")
    if name == "joint_go_to":
        if not isinstance(q, (list, tuple)) or len(q) not in (7, 9):
            raise ValueError(f"panda_prior_samples: joint_go_to takes q: [7 or 9 joint targets], not {q!r}")
        q = [float(x) for x in q]
    elif q is not None:
        raise ValueError("panda_prior_samples: q is joint_go_to's (hold takes none)")
    return name, n, q


def panda_prior_sequences(cfg, q_now):
    """the [n, T, 9] sequences of the `panda_prior_samples` key for the arm at joint positions q_now (nine), and the sample
    indices they go to (prior_sample_indices): hold gives n equal rows of zeros, joint_go_to one row per speed factor
    1 - j / n"""
    from . import priors
    name, n, q = check_panda_prior_samples(cfg)
    m = cfg.mppi
    if name == "hold":
        seqs = priors.hold(int(m.horizon), n)
    else:
        seqs = priors.joint_go_to(q_now, q, int(m.horizon), float(cfg.isaacgym.dt), [float(x) for x in m.u_max],
                                  [1.0 - j / n for j in range(n)])
    return seqs, prior_sample_indices(int(m.num_samples), n, bool(cfg.multi_modal))


def prior_samples_on_device(cfg):
    """the optional `device: true` of the `prior_samples` key: the controller runs on the device (MPPI.set_prior_controller),
    set once instead of computed on the host every tick"""
    given = getattr(cfg, "prior_samples", None)
    return bool(given) and bool(dict(given).get("device", False))


def set_device_prior_controller(cfg, planner):
    """`prior_samples={..., device: true}`: the key's controller on the planner, once (MPPI.set_prior_controller) -- the kind the
    host path takes for the task (push_behind where there is a box to go behind, else go_to), the key's n default speed factors,
    the samples of prior_sample_indices"""
    name, n = check_prior_samples(cfg)
    kind = "push_behind" if name == "push_behind" and cfg.task != "navigation" else "go_to"
    planner.set_prior_controller(kind, n, prior_sample_indices(int(cfg.mppi.num_samples), n, bool(cfg.multi_modal)))


def prior_sample_indices(K, n, multi_modal):
    """where the n priors of the `prior_samples` key sit among the K samples: the first n non-special samples; in
    multi-modal mode split between the two halves, so that both modes hear the controller"""
    if not multi_modal:
        return list(range(n))
    first = (n + 1) // 2
    return list(range(1, 1 + first)) + list(range(K // 2 + 1, K // 2 + 1 + n - first))


ROLLOUT_ARENA_SPREAD_KEYS = ("spread", "seed", "fields")


def _check_rollout_arena_spread(cfg):
    """the parsed `rollout_arena_spread` key as (spread, seed, fields); ValueError for what it cannot mean"""
    given = dict(cfg.rollout_arena_spread)
    if cfg.env_type != "point_env":
        raise ValueError("rollout_arena_spread: point_env only")
    unknown = sorted(set(given) - set(ROLLOUT_ARENA_SPREAD_KEYS))
    if unknown or "spread" not in given:
        raise ValueError(f"rollout_arena_spread: {{spread: S, seed: n, fields: [...]}} (unknown key(s) {unknown})")
    spread = float(given["spread"])
    if not 0.0 <= spread < 1.0:
        raise ValueError(f"rollout_arena_spread: spread {spread!r} is not a share in [0, 1)")
    fields = tuple(given.get("fields") or ("box_m", "box_mu_g", "mu_rb"))
    return spread, int(given.get("seed", 0) or 0), fields


ROLLOUT_ARENA_GROUPS_KEYS = ("models", "spread", "seed", "fields", "worst")


def check_rollout_arena_groups(cfg):
    """the parsed `rollout_arena_groups` key as (models, spread, seed, fields, worst); ValueError for what it cannot mean"""
    from . import groups
    given = dict(cfg.rollout_arena_groups)
    if cfg.env_type != "point_env":
        raise ValueError("rollout_arena_groups: point_env only")
    if getattr(cfg, "rollout_arena_spread", None):
        raise ValueError("rollout_arena_groups: exclusive with rollout_arena_spread (an arena per sample, or the same M arenas "
                         "for every control sequence)")
    if getattr(cfg, "prior_samples", None):
        raise ValueError("rollout_arena_groups: exclusive with prior_samples (m3_set_sample_groups refuses a handle with priors)")
    unknown = sorted(set(given) - set(ROLLOUT_ARENA_GROUPS_KEYS))
    if unknown or "models" not in given or "spread" not in given:
        raise ValueError(f"rollout_arena_groups: {{models: M, spread: S, seed: n, fields: [...], worst: f}} (unknown key(s) {unknown})")
    models = given["models"]
    if isinstance(models, bool) or not isinstance(models, int) or not 2 <= models <= groups.MAX_MEMBERS:
        raise ValueError(f"rollout_arena_groups: models {models!r} is not an integer in 2 .. {groups.MAX_MEMBERS}")
    spread = float(given["spread"])
    if not 0.0 <= spread < 1.0:
        raise ValueError(f"rollout_arena_groups: spread {spread!r} is not a share in [0, 1)")
    worst = float(given.get("worst", 1.0))
    if not 0.0 < worst <= 1.0:
        raise ValueError(f"rollout_arena_groups: worst {worst!r} is not in (0, 1]")
    if cfg.mppi.mppi_mode == "simple" or cfg.mppi.sampling_method == "random":
        raise ValueError("rollout_arena_groups: needs a noise table (mppi_mode halton-spline, sampling_method halton)")
    fields = tuple(given.get("fields") or ("box_m", "box_mu_g", "mu_rb"))
    groups.grouped_layout(int(cfg.mppi.num_samples), models, bool(cfg.multi_modal))    # (no room for a group: its ValueError)
    return models, spread, int(given.get("seed", 0) or 0), fields, worst


def rollout_arena_group_layout(cfg):
    """(group_of, model_of, arenas) of the `rollout_arena_groups` key: groups.grouped_layout for the planner's K samples and
    the M arenas scenes.spread_point_scenes(M, spread, seed, base=point_scene, fields) -- sample k plans in arenas[model_of[k]],
    a sample with model -1 in point_scene itself"""
    from . import groups, scenes
    models, spread, seed, fields, _ = check_rollout_arena_groups(cfg)
    group_of, model_of = groups.grouped_layout(int(cfg.mppi.num_samples), models, bool(cfg.multi_modal))
    arenas = scenes.spread_point_scenes(models, spread, seed, base=getattr(cfg, "point_scene", None), fields=fields)
    return group_of, model_of, arenas


def rollout_point_scenes(cfg, k_offset=0, n=None):
    """The arenas of the planner's samples under the `rollout_arena_spread` key, or None without it: the rows
    [k_offset, k_offset + n) (all K by default) of scenes.spread_point_scenes(K, spread, seed, base=point_scene, fields,
    nominal_rows=(0, K // 2, K - 1)).  The planner's K-env simulator is built with them (IsaacGymWrapper(point_scenes=...));
    the planner attached to it takes them over, so its fused path stays the step path on that simulator.
    Under the `rollout_arena_groups` key: sample k's row is the arena of its model (rollout_arena_group_layout), the nominal
    arena for the samples on their own."""
    if getattr(cfg, "rollout_arena_groups", None):
        _, model_of, arenas = rollout_arena_group_layout(cfg)
        base = dict(getattr(cfg, "point_scene", None) or {})
        rows = [dict(arenas[m]) if m >= 0 else dict(base) for m in model_of.tolist()]
        n = len(rows) - int(k_offset) if n is None else int(n)
        return rows[int(k_offset):int(k_offset) + n]
    if not getattr(cfg, "rollout_arena_spread", None):
        return None
    from . import scenes
    spread, seed, fields = _check_rollout_arena_spread(cfg)
    K = int(cfg.mppi.num_samples)
    rows = scenes.spread_point_scenes(K, spread, seed, base=getattr(cfg, "point_scene", None), fields=fields,
                                      nominal_rows=(0, K // 2, K - 1))
    n = K - int(k_offset) if n is None else int(n)
    return rows[int(k_offset):int(k_offset) + n]


def _check_rollout_workspace_spread(cfg):
    """the parsed `rollout_workspace_spread` key as (spread, seed, fields); ValueError for what it cannot mean"""
    from ._lib import PANDA_SCENE_DEFAULTS
    given = dict(cfg.rollout_workspace_spread)
    if cfg.env_type != "panda_env":
        raise ValueError("rollout_workspace_spread: panda_env only")
    unknown = sorted(set(given) - set(ROLLOUT_ARENA_SPREAD_KEYS))
    if unknown or "spread" not in given:
        raise ValueError(f"rollout_workspace_spread: {{spread: S, seed: n, fields: [...]}} (unknown key(s) {unknown})")
    spread = float(given["spread"])
    if not 0.0 <= spread < 1.0:
        raise ValueError(f"rollout_workspace_spread: spread {spread!r} is not a share in [0, 1)")
    fields = tuple(given.get("fields") or ("cube_m", "mu", "obs_m"))
    unknown = sorted(set(fields) - set(PANDA_SCENE_DEFAULTS))
    if unknown:
        raise ValueError(f"rollout_workspace_spread: unknown panda scene field(s) {unknown}: one of {list(PANDA_SCENE_DEFAULTS)}")
    return spread, int(given.get("seed", 0) or 0), fields


def rollout_panda_scenes(cfg, k_offset=0, n=None):
    """The workspaces of the planner's samples under the `rollout_workspace_spread` key, or None without it: the rows
    [k_offset, k_offset + n) (all K by default) of scenes.spread_panda_scenes(K, spread, seed, base=panda_scene, fields,
    nominal_rows=(0, K // 2, K - 1)).  The planner's K-env simulator is built with them (IsaacGymWrapper(panda_scenes=...));
    the planner attached to it takes them over, so its fused path stays the step path on that simulator."""
    if not getattr(cfg, "rollout_workspace_spread", None):
        return None
    from . import scenes
    spread, seed, fields = _check_rollout_workspace_spread(cfg)
    K = int(cfg.mppi.num_samples)
    rows = scenes.spread_panda_scenes(K, spread, seed, base=getattr(cfg, "panda_scene", None), fields=fields,
                                      nominal_rows=(0, K // 2, K - 1))
    n = K - int(k_offset) if n is None else int(n)
    return rows[int(k_offset):int(k_offset) + n]


def world_point_scene(cfg):
    """The field overrides of the arena of cfg's REAL world: `point_scene` with `world_point_scene` on top ({} = the
    reference's arena)."""
    return {**(getattr(cfg, "point_scene", None) or {}), **(getattr(cfg, "world_point_scene", None) or {})}


def world_panda_scene(cfg):
    """The field overrides of the workspace of cfg's REAL world: `panda_scene` with `world_panda_scene` on top ({} = the
    reference's workspace)."""
    return {**(getattr(cfg, "panda_scene", None) or {}), **(getattr(cfg, "world_panda_scene", None) or {})}


def world_isaacgym_config(cfg):
    """cfg.isaacgym as the 1-env or N-env REAL world is built from it: cfg.isaacgym itself unless `world_point_scene` /
    `world_panda_scene` is set, else a copy whose point_scene / panda_scene carries those overrides too.  The planner's
    K-env simulator is built from cfg.isaacgym."""
    import dataclasses
    if getattr(cfg, "world_panda_scene", None):
        return dataclasses.replace(cfg.isaacgym, panda_scene=world_panda_scene(cfg))
    if not getattr(cfg, "world_point_scene", None):
        return cfg.isaacgym
    return dataclasses.replace(cfg.isaacgym, point_scene=world_point_scene(cfg))


def _hydra_standin():
    m = types.ModuleType("hydra")

    def main(version_base=None, config_path=None, config_name="config_point"):
        def deco(fn):
            def run(*a, **k):
                if a or k:
                    return fn(*a, **k)
                argv, name, ov = sys.argv[1:], config_name, []
                i = 0
                while i < len(argv):
                    if argv[i] in ("-cn", "--config-name"):
                        name = argv[i + 1]
                        i += 2
                    else:
                        ov.append(argv[i])
                        i += 1
                return fn(make_config(name, ov))
            return run
        return deco

    m.main = main
    return m


def _zerorpc_standin():
    """`zerorpc` is not installed here: the Server / Client pair of m3p2i_aip_amd.rpc (same calls, a plain
    TCP + msgpack transport) answers to the name, so reactive_tamp.py:89-94 and sim.py:29-49 run as two
    processes."""
    from . import rpc
    m = types.ModuleType("zerorpc")
    m.Server, m.Client = rpc.Server, rpc.Client
    m.RemoteError, m.LostRemote = rpc.RemoteError, rpc.LostRemote
    return m


def install(force_standins: bool = False):
    """Make `import m3p2i_aip...`, `import isaacgym`, `hydra`, `zerorpc` resolve to this build."""
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    ig = mod("isaacgym")
    ig.gymtorch = mod("isaacgym.gymtorch")
    ig.gymapi = mod("isaacgym.gymapi")
    root = mod("m3p2i_aip")
    mod("m3p2i_aip.planners")
    mp = mod("m3p2i_aip.planners.motion_planner")
    mp.m3p2i = mod("m3p2i_aip.planners.motion_planner.m3p2i", M3P2I=planner.M3P2I)
    mp.mppi = mod("m3p2i_aip.planners.motion_planner.mppi", MPPI=planner.MPPI, MPPIConfig=planner.MPPIConfig)
    mp.cost_functions = mod("m3p2i_aip.planners.motion_planner.cost_functions",
                            Objective=cost_functions.Objective)
    tp = mod("m3p2i_aip.planners.task_planner")
    tp.task_planner = mod("m3p2i_aip.planners.task_planner.task_planner", set_task_planner=set_task_planner,
                          PLANNER_SIMPLE=PLANNER_SIMPLE, PLANNER_AIF_PANDA=PLANNER_AIF_PANDA,
                          PLANNER_PATROLLING=task_planner.PLANNER_PATROLLING)
    tp.ai_agent = mod("m3p2i_aip.planners.task_planner.ai_agent", AiAgent=task_planner.AiAgent)
    tp.adaptive_action_selection = mod("m3p2i_aip.planners.task_planner.adaptive_action_selection",
                                       adapt_act_sel=task_planner.adapt_act_sel)
    tp.parallel_action_selection = mod("m3p2i_aip.planners.task_planner.parallel_action_selection",
                                       par_act_sel=task_planner.par_act_sel)
    tp.isaac_state_action_templates = mod(
        "m3p2i_aip.planners.task_planner.isaac_state_action_templates",
        MDPIsCubeAtReal=task_planner.MDPIsCubeAtReal,
        **{n: getattr(task_planner, n) for n in task_planner.TEMPLATE_TABLE})
    cfgm = mod("m3p2i_aip.config")
    cfgm.config_store = mod("m3p2i_aip.config.config_store", ExampleConfig=ExampleConfig)
    ut = mod("m3p2i_aip.utils")
    ut.data_transfer = mod("m3p2i_aip.utils.data_transfer", torch_to_bytes=torch_to_bytes,
                           bytes_to_torch=bytes_to_torch)
    ut.skill_utils = mod("m3p2i_aip.utils.skill_utils", calculate_suction=calculate_suction,
                         check_suction_condition=check_suction_condition,
                         check_and_apply_suction=check_and_apply_suction, time_tracking=time_tracking)
    iu = mod("m3p2i_aip.utils.isaacgym_utils")
    sys.modules["m3p2i_aip.utils.isaacgym_utils.isaacgym_wrapper"] = isaacgym_wrapper
    iu.isaacgym_wrapper = isaacgym_wrapper
    ut.isaacgym_utils = iu
    root.planners, root.config, root.utils = sys.modules["m3p2i_aip.planners"], cfgm, ut
    sys.modules["m3p2i_aip.planners"].motion_planner = mp
    sys.modules["m3p2i_aip.planners"].task_planner = tp
    for name, make in (("hydra", _hydra_standin), ("zerorpc", _zerorpc_standin)):
        have = False
        if not force_standins:
            try:
                __import__(name)
                have = True
            except Exception:
                have = False
        if not have:
            sys.modules[name] = make()
