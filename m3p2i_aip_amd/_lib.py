"""ctypes binding of libm3p2i_hip.so (C-ABI declared in include/m3p2i_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or a call fails this
module raises.  Build with ``python -m m3p2i_aip_amd.build`` (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes as C
import os

MAX_NU = 9
MAX_PRIOR_SAMPLES = 256
TOPK = 20
ABI_VERSION = 4

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("M3P2I_HIP_LIB") or os.path.join(_HERE, "lib", "libm3p2i_hip.so")

ENV_POINT, ENV_PANDA = 0, 1
HALTON_PLAIN, HALTON_FAURE = 0, 1
IPC_HANDLE_BYTES = 64
TASKS = {"navigation": 0, "push": 1, "pull": 2, "push_pull": 3, "reach": 4, "pick": 5,
         "place": 6, "idle": 7}

(BUF_STATES, BUF_ACTIONS, BUF_COST_HORIZON, BUF_TRAJ_COST, BUF_TRAJ_COST_ALL, BUF_WEIGHTS,
 BUF_WEIGHTS_1, BUF_WEIGHTS_2, BUF_MEAN, BUF_MEAN_1, BUF_MEAN_2, BUF_BEST, BUF_BEST_1,
 BUF_BEST_2, BUF_ACTION_OUT, BUF_TOP_IDX, BUF_TOP_TRAJS, BUF_REDUCE, BUF_NOISE,
 BUF_PENDING_FORCE, BUF_INFO, BUF_SIM_WORLD, BUF_RECORD, BUF_RECORDS_ALL, BUF_NOISE_ALL, BUF_COV,
 BUF_RECORD_B, BUF_RECORDS_B_ALL, BUF_COUNT) = range(29)


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int), ("device", C.c_int), ("K_global", C.c_int),
                ("K_local", C.c_int), ("k_offset", C.c_int), ("T", C.c_int), ("nu", C.c_int),
                ("env_type", C.c_int), ("multi_modal", C.c_int), ("mode_simple", C.c_int),
                ("sampling_random", C.c_int), ("sample_null_action", C.c_int),
                ("filter_u", C.c_int), ("u_per_command", C.c_int),
                ("u_min", C.c_float * MAX_NU), ("u_max", C.c_float * MAX_NU),
                ("noise_sigma_diag", C.c_float * MAX_NU), ("u_scale", C.c_float),
                ("gamma", C.c_float), ("lambda_", C.c_float), ("step_size_mean", C.c_float),
                ("kp_suction", C.c_float), ("pre_height_diff", C.c_float), ("dt", C.c_float),
                ("substeps", C.c_int), ("solver_iters", C.c_int), ("cube_on_shelf", C.c_int),
                ("sim_only", C.c_int), ("shard_mix", C.c_int), ("noise_abs_cost", C.c_int),
                ("update_cov", C.c_int), ("full_sigma", C.c_int), ("noise_mu", C.c_float * MAX_NU),
                ("noise_sigma_full", C.c_float * (MAX_NU * MAX_NU)), ("seed", C.c_ulonglong)]


BATCH_PANDA_RUNTIME = 1   # M3_BATCH_PANDA_RUNTIME (m3_batch_create_ex)
PANDA_EPISODES_RUNTIME = 1   # M3_PANDA_EPISODES_RUNTIME (m3_panda_episodes_create_ex)
BATCH_SECTION_PANDA_RUNTIME = 1          # M3_BATCH_SECTION_PANDA_RUNTIME (m3_batch_create_sections)
BATCH_SECTION_POINT_ROLLOUT_SCENES = 2   # M3_BATCH_SECTION_POINT_ROLLOUT_SCENES
EPISODES_ROLLOUT_SCENES = 1              # M3_EPISODES_ROLLOUT_SCENES (m3_episodes_create_ex)
BATCH_SECTION_POINT_PRIORS = 32          # M3_BATCH_SECTION_POINT_PRIORS (4, 8 and 16 stay unknown section bits)
EPISODES_PRIORS = 8                      # M3_EPISODES_PRIORS (2 and 4 stay unknown flag bits)


PRIOR_CONTROLLER_GO_TO, PRIOR_CONTROLLER_PUSH_BEHIND = 1, 2   # m3_prior_controller.kind (m3p2i_hip_ext.h)
PRIOR_CONTROLLER_KINDS = {"go_to": PRIOR_CONTROLLER_GO_TO, "push_behind": PRIOR_CONTROLLER_PUSH_BEHIND}
MAX_PRIOR_CONTROLLER_SEQS = 16


class PriorController(C.Structure):   # m3_prior_controller
    _fields_ = [("kind", C.c_int), ("n", C.c_int), ("speed", C.c_float * MAX_PRIOR_CONTROLLER_SEQS),
                ("standoff", C.c_float), ("reach", C.c_float)]


class PointWorld(C.Structure):
    _fields_ = [("robot", C.c_float * 4), ("box", C.c_float * 7), ("dyn_obs", C.c_float * 7)]


COST_WEIGHT_DEFAULTS = dict(nav_dist=1.0, collision=1000.0, robot_box=1.0, box_goal=10.0, push_dist=3.0, push_align=1.0,
                            pull_dist=3.0, pull_vel=3.0, pull_align=7.0)   # m3_point_cost_weights, in field order


class PointCostWeights(C.Structure):
    _fields_ = [(n, C.c_float) for n in COST_WEIGHT_DEFAULTS]


PANDA_COST_WEIGHT_DEFAULTS = dict(reach_dist=10.0, reach_tilt=3.0, pick_goal=10.0, pick_ori=15.0, collision=1000.0,
                                  shelf_force=4.0, place_grip=2.0)   # m3_panda_cost_weights, in field order


class PandaCostWeights(C.Structure):
    _fields_ = [(n, C.c_float) for n in PANDA_COST_WEIGHT_DEFAULTS]


# m3_point_scene, in field order, with the values of m3_default_point_scene (the reference's arena; the oracle's
# m3o_point_scene_default): box_I / dyn_I = 16 * (0.4^2 + 0.4^2) / 12 and *_req = 0.3825978 * 0.4 are formed in binary32 there
def _f32(x):
    return C.c_float(x).value


_I_DEFAULT = _f32(_f32(_f32(16.0) * _f32(_f32(_f32(0.4) * _f32(0.4)) + _f32(_f32(0.4) * _f32(0.4)))) / 12.0)
_REQ_DEFAULT = _f32(_f32(0.3825978) * _f32(0.4))
POINT_SCENE_DEFAULTS = dict(
    robot_r=0.2, robot_m=10.0,
    box_hx=0.2, box_hy=0.2, box_m=16.0, box_I=_I_DEFAULT, box_mu_g=0.75, box_req=_REQ_DEFAULT,
    dyn_hx=0.2, dyn_hy=0.2, dyn_m=16.0, dyn_I=_I_DEFAULT, dyn_mu_g=1.0, dyn_req=_REQ_DEFAULT,
    obs_x=2.0, obs_y=2.0, obs_hx=0.15, obs_hy=0.2, wall=3.95,
    mu_rb=0.275, mu_rd=0.525, mu_ro=0.525, mu_rw=0.525, mu_bw=0.75, mu_dw=1.0, mu_bd=0.75, mu_bo=0.75, mu_do=1.0)


class PointSceneFields(C.Structure):
    _fields_ = [(n, C.c_float) for n in POINT_SCENE_DEFAULTS]


# m3_panda_scene, in field order, with the values of m3_default_panda_scene (the reference's workspace; the oracle's
# m3o_panda_scene_default)
PANDA_SCENE_DEFAULTS = dict(
    base=(-0.45, 0.0, 1.125), table=(0.0, 0.0, 1.0, 0.6, 0.6, 0.025), shelf=(0.5, 0.0, 1.175, 0.1, 0.1, 0.15),
    obs_half=(0.1, 0.1, 0.01), obs_m=0.8, cube_m=0.125, mu=1.0)


class PandaSceneFields(C.Structure):
    _fields_ = [(n, C.c_float * len(v) if isinstance(v, tuple) else C.c_float) for n, v in PANDA_SCENE_DEFAULTS.items()]


def panda_scene_fields(overrides=None):
    """PandaSceneFields from field overrides over PANDA_SCENE_DEFAULTS (array fields as sequences of their length); ValueError
    for an unknown field (with the list of fields) or a wrong length."""
    overrides = dict(overrides or {})
    unknown = sorted(set(overrides) - set(PANDA_SCENE_DEFAULTS))
    if unknown:
        raise ValueError(f"unknown panda scene field(s) {unknown}: one of {list(PANDA_SCENE_DEFAULTS)}")
    sc = PandaSceneFields()
    for n, lit in PANDA_SCENE_DEFAULTS.items():
        v = overrides.get(n, lit)
        if isinstance(lit, tuple):
            v = [float(x) for x in v]
            if len(v) != len(lit):
                raise ValueError(f"panda scene field {n!r}: {len(v)} values, it has {len(lit)}")
            setattr(sc, n, (C.c_float * len(lit))(*v))
        else:
            setattr(sc, n, float(v))
    return sc


def panda_scene_dict(sc):
    """all fields of a PandaSceneFields as a mapping like PANDA_SCENE_DEFAULTS (binary32 values)"""
    return {n: tuple(getattr(sc, n)) if isinstance(lit, tuple) else getattr(sc, n) for n, lit in PANDA_SCENE_DEFAULTS.items()}


class Info(C.Structure):
    _fields_ = [("eta", C.c_float), ("eta_1", C.c_float), ("eta_2", C.c_float),
                ("beta", C.c_float), ("beta_1", C.c_float), ("beta_2", C.c_float),
                ("iters", C.c_int), ("iters_1", C.c_int), ("iters_2", C.c_int),
                ("best_idx", C.c_int), ("best_idx_1", C.c_int), ("best_idx_2", C.c_int),
                ("wsum_push", C.c_float), ("wsum_pull", C.c_float),
                ("pull_preference", C.c_int), ("calls", C.c_int)]


INFO_WORDS = C.sizeof(Info) // 4
INFO_PULL_PREFERENCE = Info.pull_preference.offset // 4   # index of the field in an int32 view of M3_BUF_INFO


class EpisodeSpec(C.Structure):
    _fields_ = [("task", C.c_int), ("goal", C.c_float * 2), ("dyn_phase", C.c_int), ("suction", C.c_int),
                ("kp_suction", C.c_float)]


class EpisodeStatus(C.Structure):
    _fields_ = [("done_tick", C.c_int), ("success", C.c_int), ("collision_ticks", C.c_int), ("final_pos", C.c_float * 2)]


SUCTION_OFF, SUCTION_ON, SUCTION_PULL_PREFERENCE = 0, 1, 2


class PandaEpisodeStatus(C.Structure):
    _fields_ = [("phase", C.c_int), ("done_tick", C.c_int), ("success", C.c_int), ("settle_left", C.c_int),
                ("cubeA", C.c_float * 3), ("cubeB", C.c_float * 3)]


PE_RUNNING, PE_SETTLING, PE_FROZEN = 0, 1, 2
PANDA_EPISODE_TRACE_FLOATS = 132
# offsets inside a trace row: dof_state 18 | root_state 91 | action 9 | panda_hand pose 7 | cubeA body pose 7
PE_TR_DOF, PE_TR_ROOT, PE_TR_ACTION, PE_TR_HAND, PE_TR_CUBE = 0, 18, 109, 118, 125


class Timing(C.Structure):
    _fields_ = [("rollout_ms", C.c_float), ("update_ms", C.c_float),
                ("finalize_ms", C.c_float), ("total_ms", C.c_float)]


# every symbol include/m3p2i_hip.h declares: (name, restype, argtypes)
_H = C.c_void_p
_FP = C.c_void_p  # float* (host or device), passed as integer addresses
SYMBOLS = [
    ("m3_abi_version", C.c_int, []),
    ("m3_build_id", C.c_char_p, []),
    ("m3_last_error", C.c_char_p, [_H]),
    ("m3_default_config", None, [C.POINTER(Config), C.c_int]),
    ("m3_create", C.c_int, [C.POINTER(Config), C.POINTER(_H)]),
    ("m3_destroy", None, [_H]),
    ("m3_set_stream", C.c_int, [_H, C.c_void_p]),
    ("m3_enable_timing", C.c_int, [_H, C.c_int]),
    ("m3_set_rollout_lanes", C.c_int, [_H, C.c_int]),
    ("m3_set_point_rollout_form", C.c_int, [_H, C.c_int]),
    ("m3_point_rollout_form_used", C.c_int, [_H]),
    ("m3_set_panda_lanes_per_sample", C.c_int, [_H, C.c_int]),
    ("m3_panda_lanes_per_sample_used", C.c_int, [_H]),
    ("m3_panda_near_share", C.c_int, [_H]),
    ("m3_set_panda_reach_cost_kernel", C.c_int, [_H, C.c_int]),
    ("m3_set_update_launches", C.c_int, [_H, C.c_int]),
    ("m3_set_ladder_spins", C.c_int, [_H, C.c_int]),
    ("m3_set_wave_order", C.c_int, [_H, C.c_int]),
    ("m3_relabel_samples", C.c_int, [_H]),
    ("m3_set_noise", C.c_int, [_H, _FP, C.c_int]),
    ("m3_set_noise_knots", C.c_int, [_H, _FP, C.c_int, C.c_int, C.c_float, C.c_int]),
    ("m3_set_noise_global", C.c_int, [_H, _FP, C.c_int]),
    ("m3_set_noise_knots_global", C.c_int, [_H, _FP, C.c_int, C.c_int, C.c_float, C.c_int]),
    ("m3_set_noise_halton", C.c_int, [_H, C.c_int, C.c_int, C.c_float]),
    ("m3_set_noise_halton_scrambled", C.c_int, [_H, C.c_int, C.c_int, C.c_float, C.c_int]),
    ("m3_sample_noise", C.c_int, [_H]),
    ("m3_set_call_count", C.c_int, [_H, C.c_uint]),
    ("m3_set_objective", C.c_int, [_H, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int]),
    ("m3_set_avoid_dyn_obs", C.c_int, [_H, C.c_int]),
    ("m3_default_point_cost_weights", None, [C.POINTER(PointCostWeights)]),
    ("m3_set_point_cost_weights", C.c_int, [_H, C.POINTER(PointCostWeights)]),
    ("m3_get_point_cost_weights", C.c_int, [_H, C.POINTER(PointCostWeights)]),
    ("m3_set_weighted_cost_instance", C.c_int, [_H, C.c_int]),
    ("m3_default_point_scene", None, [C.POINTER(PointSceneFields)]),
    ("m3_set_point_scene", C.c_int, [_H, C.POINTER(PointSceneFields)]),
    ("m3_get_point_scene", C.c_int, [_H, C.POINTER(PointSceneFields)]),
    ("m3_set_point_scene_instance", C.c_int, [_H, C.c_int]),
    ("m3_set_point_scene_rows", C.c_int, [_H, C.POINTER(PointSceneFields), C.c_int]),
    ("m3_get_point_scene_row", C.c_int, [_H, C.c_int, C.POINTER(PointSceneFields)]),
    ("m3_point_scene_rows_set", C.c_int, [_H]),
    ("m3_set_point_rollout_scenes", C.c_int, [_H, C.POINTER(PointSceneFields), C.c_int]),
    ("m3_get_point_rollout_scene", C.c_int, [_H, C.c_int, C.POINTER(PointSceneFields)]),
    ("m3_point_rollout_scenes_set", C.c_int, [_H]),
    ("m3_default_panda_scene", None, [C.POINTER(PandaSceneFields)]),
    ("m3_set_panda_scene", C.c_int, [_H, C.POINTER(PandaSceneFields)]),
    ("m3_get_panda_scene", C.c_int, [_H, C.POINTER(PandaSceneFields)]),
    ("m3_set_panda_scene_instance", C.c_int, [_H, C.c_int]),
    ("m3_panda_scene_instance_used", C.c_int, [_H]),
    ("m3_set_panda_scene_rows", C.c_int, [_H, C.POINTER(PandaSceneFields), C.c_int]),
    ("m3_get_panda_scene_row", C.c_int, [_H, C.c_int, C.POINTER(PandaSceneFields)]),
    ("m3_panda_scene_rows_set", C.c_int, [_H]),
    ("m3_set_panda_rollout_scenes", C.c_int, [_H, C.POINTER(PandaSceneFields), C.c_int]),
    ("m3_get_panda_rollout_scene", C.c_int, [_H, C.c_int, C.POINTER(PandaSceneFields)]),
    ("m3_panda_rollout_scenes_set", C.c_int, [_H]),
    ("m3_default_panda_cost_weights", None, [C.POINTER(PandaCostWeights)]),
    ("m3_set_panda_cost_weights", C.c_int, [_H, C.POINTER(PandaCostWeights)]),
    ("m3_get_panda_cost_weights", C.c_int, [_H, C.POINTER(PandaCostWeights)]),
    ("m3_set_panda_weighted_cost_instance", C.c_int, [_H, C.c_int]),
    ("m3_panda_weighted_cost_instance_used", C.c_int, [_H]),
    ("m3_point_rollout_plan", C.c_int, [C.c_int] * 8 + [C.c_float] + [C.c_int] * 6 + [C.POINTER(C.c_int)]),
    ("m3_point_rollout_plan_ex", C.c_int, [C.c_int] * 8 + [C.c_float] + [C.c_int] * 7 + [C.POINTER(C.c_int)]),
    ("m3_set_prior_samples", C.c_int, [_H, C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    ("m3_set_prior_samples_device", C.c_int, [_H, C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    ("m3_prior_samples_set", C.c_int, [_H]),
    ("m3_get_prior_sample", C.c_int, [_H, C.c_int, C.POINTER(C.c_int), _FP]),
    ("m3_prior_samples_used", C.c_int, [_H]),
    ("m3_set_panda_prior_samples", C.c_int, [_H, C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    ("m3_set_panda_prior_samples_device", C.c_int, [_H, C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    ("m3_panda_prior_samples_set", C.c_int, [_H]),
    ("m3_get_panda_prior_sample", C.c_int, [_H, C.c_int, C.POINTER(C.c_int), _FP]),
    ("m3_panda_prior_samples_used", C.c_int, [_H]),
    ("m3_owned_blocks_live", C.c_longlong, []),
    ("m3_set_multi_modal", C.c_int, [_H, C.c_int]),
    ("m3_set_plan", C.c_int, [_H, C.c_int, _FP]),
    ("m3_set_action_out", C.c_int, [_H, C.c_void_p]),
    ("m3_set_beta", C.c_int, [_H, C.c_float]),
    ("m3_reset", C.c_int, [_H]),
    ("m3_set_world_point", C.c_int, [_H, C.POINTER(PointWorld)]),
    ("m3_set_world_point_raw", C.c_int, [_H, C.POINTER(C.c_float)]),
    ("m3_bind_sim_point", C.c_int, [_H, _FP, _FP, C.c_int, C.c_int, C.c_int]),
    ("m3_set_world_panda_raw", C.c_int, [_H, C.POINTER(C.c_float)]),
    ("m3_bind_sim_panda", C.c_int, [_H, _FP, _FP, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("m3_command", C.c_int, [_H, _FP]),
    ("m3_rollout", C.c_int, [_H]),
    ("m3_update", C.c_int, [_H]),
    ("m3_finalize", C.c_int, [_H]),
    ("m3_update_finalize", C.c_int, [_H]),
    ("m3_p2p_export", C.c_int, [_H, C.c_void_p]),
    ("m3_p2p_connect", C.c_int, [_H, C.c_void_p, C.c_int]),
    ("m3_p2p_connect_local", C.c_int, [_H, C.POINTER(_H), C.c_int]),
    ("m3_p2p_put", C.c_int, [_H]),
    ("m3_p2p_wait", C.c_int, [_H]),
    ("m3_p2p_exchange", C.c_int, [_H]),
    ("m3_p2p_put_ch", C.c_int, [_H, C.c_int]),
    ("m3_p2p_wait_ch", C.c_int, [_H, C.c_int]),
    ("m3_p2p_exchange_b", C.c_int, [_H]),
    ("m3_update_b", C.c_int, [_H]),
    ("m3_record_b_len", C.c_int, [_H]),
    ("m3_p2p_status", C.c_int, [_H, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("m3_p2p_set_timeout_ms", C.c_int, [_H, C.c_int, C.c_int]),
    ("m3_p2p_clear_error", C.c_int, [_H]),
    ("m3_p2p_detach", C.c_int, [_H]),
    ("m3_p2p_set_memory_kind", C.c_int, [_H, C.c_int]),
    ("m3_batch_create", C.c_int, [C.c_int, C.c_int, C.POINTER(_H)]),
    ("m3_batch_create_ex", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(_H)]),
    ("m3_batch_flags", C.c_int, [_H]),
    ("m3_batch_destroy", None, [_H]),
    ("m3_batch_last_error", C.c_char_p, [_H]),
    ("m3_batch_command", C.c_int, [_H, C.POINTER(_H), C.c_int, _FP]),
    ("m3_batch_launches", C.c_int, [_H, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("m3_episodes_create", C.c_int, [_H, C.POINTER(_H), C.POINTER(EpisodeSpec), C.c_int, C.c_int, C.c_int, C.POINTER(_H)]),
    ("m3_episodes_tick", C.c_int, [_H, _H]),
    ("m3_episodes_begin", C.c_int, [_H]),
    ("m3_episodes_end", C.c_int, [_H]),
    ("m3_episodes_status", C.c_int, [_H, C.POINTER(EpisodeStatus), C.c_void_p]),
    ("m3_episodes_ticks_done", C.c_int, [_H]),
    ("m3_episodes_running", C.c_int, [_H]),
    ("m3_episodes_destroy", None, [_H]),
    ("m3_episodes_last_error", C.c_char_p, [_H]),
    ("m3_panda_episodes_create", C.c_int, [_H, C.POINTER(_H), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_H)]),
    ("m3_panda_episodes_observe", C.c_int, [_H, C.POINTER(C.POINTER(C.c_float))]),
    ("m3_panda_episodes_act", C.c_int, [_H, _H, C.POINTER(C.c_int)]),
    ("m3_panda_episodes_act_first", C.c_int, [_H, C.POINTER(_H), C.POINTER(C.c_int)]),
    ("m3_panda_episodes_status", C.c_int, [_H, C.POINTER(PandaEpisodeStatus), C.c_void_p]),
    ("m3_panda_episodes_ticks_done", C.c_int, [_H]),
    ("m3_panda_episodes_running", C.c_int, [_H]),
    ("m3_panda_episodes_active", C.c_int, [_H]),
    ("m3_panda_episodes_destroy", None, [_H]),
    ("m3_panda_episodes_last_error", C.c_char_p, [_H]),
    ("m3_get_buffer", C.c_int, [_H, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]),
    ("m3_reduce_len", C.c_int, [_H]),
    ("m3_record_len", C.c_int, [_H]),
    ("m3_get_info", C.c_int, [_H, C.POINTER(Info)]),
    ("m3_get_timing", C.c_int, [_H, C.POINTER(Timing)]),
    ("m3_sim_bind_views", C.c_int, [_H, _FP, _FP, _FP, _FP, C.c_int, C.c_int]),
    ("m3_sim_pull_state", C.c_int, [_H]),
    ("m3_sim_shift_actor", C.c_int, [_H, C.c_int, C.c_float, C.c_float, C.c_float]),
    ("m3_sim_step_with_target", C.c_int, [_H, C.c_void_p]),
    ("m3_sim_push_state", C.c_int, [_H]),
    ("m3_sim_set_velocity_target", C.c_int, [_H, _FP]),
    ("m3_sim_apply_body_forces", C.c_int, [_H, _FP]),
    ("m3_sim_step", C.c_int, [_H]),
    ("m3_cost", C.c_int, [_H, _FP]),
    ("m3_sim_suction_forces", C.c_int, [_H, C.c_float, _FP]),
    ("m3_sim_check_and_apply_suction", C.c_int, [_H, _FP, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    ("m3_wave_order", C.c_int, [_H, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    ("m3_set_sample_groups", C.c_int, [_H, C.POINTER(C.c_int), C.c_int, C.c_float]),
    ("m3_sample_groups_set", C.c_int, [_H]),
    ("m3_get_sample_group", C.c_int, [_H, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("m3_sample_group_raw_costs", C.c_int, [_H, C.POINTER(C.c_void_p)]),
    ("m3_aggregate_sample_groups", C.c_int, [_H]),
]

# every symbol include/m3p2i_hip_ext.h declares -- additive forms of calls above, in a table of their own: SYMBOLS stays the list
# of include/m3p2i_hip.h, name for name
SYMBOLS_EXT = [
    ("m3_panda_episodes_create_ex", C.c_int, [_H, C.POINTER(_H), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_H)]),
    ("m3_panda_episodes_flags", C.c_int, [_H]),
    ("m3_batch_create_sections", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(_H)]),
    ("m3_episodes_create_ex", C.c_int, [_H, C.POINTER(_H), C.POINTER(EpisodeSpec), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_H)]),
    ("m3_episodes_flags", C.c_int, [_H]),
    ("m3_default_prior_controller", None, [C.POINTER(PriorController), C.c_int, C.c_int]),
    ("m3_set_prior_controller", C.c_int, [_H, C.POINTER(PriorController), C.POINTER(C.c_int)]),
    ("m3_get_prior_controller", C.c_int, [_H, C.POINTER(PriorController)]),
    ("m3_prior_controller_fill", C.c_int, [_H]),
    ("m3_prior_table", C.c_int, [_H, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
]

_lib = None


class M3Error(RuntimeError):
    pass


def load():
    """Load the HIP library.  Raises if it has not been built -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise M3Error(f"{LIB_PATH} not found: build it with `python -m m3p2i_aip_amd.build` "
                      "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # torch must be imported FIRST: it maps its bundled libamdhip64.so.7, and our NEEDED entry
    # then resolves to that same runtime (one HIP runtime per process), so device pointers
    # and streams are interchangeable between torch and the library.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS + SYMBOLS_EXT:
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    if lib.m3_abi_version() != ABI_VERSION:
        raise M3Error("libm3p2i_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc, handle=None):
    if rc != 0:
        lib = load()
        msg = lib.m3_last_error(handle)
        raise M3Error(f"m3p2i_hip error {rc}: {msg.decode() if msg else ''}")
