/*
 * m3p2i_hip_ext.h -- entry points of libm3p2i_hip.so added beside the list of include/m3p2i_hip.h (M3_ABI_VERSION stays 4: a
 * caller of that header alone sees no change).  They are additive "_ex" forms of calls declared there and are bound from a
 * table of their own in m3p2i_aip_amd/_lib.py (SYMBOLS_EXT).
 */
#ifndef M3P2I_HIP_EXT_H
#define M3P2I_HIP_EXT_H
#include "m3p2i_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- lockstep panda_env episodes with run-time workspaces, weights and rows -----
 * On request (additive; M3_ABI_VERSION stays 4): flags == 0 is m3_panda_episodes_create, word for word -- the same checks,
 * messages and kernels; unknown bits are M3_ERR_BAD_ARG.  A set created with M3_PANDA_EPISODES_RUNTIME also takes a world with
 * a run-time workspace (m3_set_panda_scene) or a workspace per environment (m3_set_panda_scene_rows), and planners that need
 * the run-time-scene instance, the weighted family (m3_set_panda_cost_weights), both, or have a workspace per sample
 * (m3_set_panda_rollout_scenes).  Every other refusal of m3_panda_episodes_create stays, in the same order; a switch forced off
 * (m3_set_panda_scene_instance(h, 0) / m3_set_panda_weighted_cost_instance(h, 0)) against what the handle holds is M3_ERR_STATE
 * at create and at every tick, nothing launched.
 * Which workspace a tick's two steps run in.  The post kernel steps row e of the world in the world's workspace: scenes[e] of
 * m3_set_panda_scene_rows, else its single scene.  The pre kernel, which reproduces the step of row 0 of planner e's own
 * simulator, runs in the workspace that row steps in: row 0 of the planner's per-sample rows when it has them, else the planner
 * handle's single scene; the link poses of the planning view go through that workspace's base, and its rows of the table, the
 * shelf stand and the robot's mount show that workspace too.  The set owns two tables of 22 words per row for this (device
 * and pinned, allocated at create); m3_set_panda_scene, _scene_rows, _rollout_scenes or the weights called between two ticks
 * apply from the next tick -- observe brings the planning side up to date, act / act_first the world side, one asynchronous
 * copy each and only when a row changed; no allocation, no further synchronisation.  The dt / substeps of every row are the
 * world's (m3_panda_episodes_act_first insists that the simulators' equal them).
 * m3_panda_episodes_act of such a set passes the batch's own flag on: a batch created without M3_BATCH_PANDA_RUNTIME refuses a
 * planner that needs the run-time section with m3_batch_command's code and message, before anything is launched.
 * At the default workspaces and weights a run-time set gives the bits of a plain one (its two kernels read their scene from
 * the tables). */
#define M3_PANDA_EPISODES_RUNTIME 1
int m3_panda_episodes_create_ex(m3_handle* world, m3_handle* const* planners, int n, int max_ticks, int settle_ticks, int trace,
                                int flags, m3_panda_episodes** out);
int m3_panda_episodes_flags(const m3_panda_episodes* eps);   /* the flags it was created with; M3_ERR_BAD_ARG for NULL */

#ifdef __cplusplus
}
#endif
#endif
