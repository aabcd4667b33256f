/*
 * m3p2i_hip_ext.h -- entry points of libm3p2i_hip.so added beside the list of include/m3p2i_hip.h (M3_ABI_VERSION stays 4: a
 * caller of that header alone sees no change).  They are additive "_ex" / "_sections" forms of calls declared there and are bound from a
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

/* ---- batched command and lockstep episodes of point_env planners with an arena per sample (DESIGN.md sections 7b.3, 7c3) ----
 * On request (additive; M3_ABI_VERSION stays 4).  m3_batch_create, m3_batch_create_ex and m3_episodes_create keep refusing a
 * point_env planner with an arena per sample (m3_set_point_rollout_scenes), with the codes and messages they always had.
 *
 * m3_batch_create_sections(device, max_handles, sections, &out): a batch whose table slots have the sections asked for.
 * sections == 0 is m3_batch_create; M3_BATCH_SECTION_PANDA_RUNTIME is M3_BATCH_PANDA_RUNTIME of m3_batch_create_ex (the same
 * bit); unknown bits are M3_ERR_BAD_ARG ("unknown section bits").  M3_BATCH_SECTION_POINT_ROLLOUT_SCENES sizes the slots for a
 * fourth section of point_env rollout entries, behind plain / weighted / scene: m3_batch_command on such a batch accepts,
 * besides everything else, an unsharded point_env planner handle with an arena per sample.  Such handles are grouped by K, T
 * and lanes per wavefront (one kernel instance; handles with different dt / substeps / weights / rows share a launch), one
 * rollout launch per group, counted by m3_batch_launches; the update side is as for every handle.  An entry carries the
 * handle's arguments, its scene's uniform members, its weights and a pointer to the handle's OWN device table of rows: the
 * batch keeps no rows.  Each handle's results are bit-identical to its own m3_command's.  Every other refusal of
 * m3_batch_command stays, in the same order and with the same words; m3_set_point_scene_instance(h, 0) against a handle with
 * rows is M3_ERR_STATE ("... forced off ...").  m3_batch_flags returns the section bits.  All device and pinned memory is
 * allocated here; a call allocates nothing.
 * Ordering: m3_set_point_rollout_scenes uploads the handle's table with an asynchronous copy on the handle's stream -- the
 * stream of the batch's launches (all handles of a call share one) -- so rows set between two batched calls apply from the
 * next one, exactly as between two m3_command calls; the pinned source of the previous upload is rewritten only after a
 * synchronisation of that stream. */
#define M3_BATCH_SECTION_PANDA_RUNTIME 1
#define M3_BATCH_SECTION_POINT_ROLLOUT_SCENES 2
int m3_batch_create_sections(int device, int max_handles, int sections, m3_batch** out);

/* m3_episodes_create_ex(..., flags, &out): flags == 0 is m3_episodes_create, word for word -- the same checks, messages and
 * kernels; unknown bits are M3_ERR_BAD_ARG.  A set created with M3_EPISODES_ROLLOUT_SCENES also takes planners with an arena
 * per sample, at create and at every tick; every other refusal stays.  m3_episodes_tick hands the running planners to the
 * batch it is given: a batch without M3_BATCH_SECTION_POINT_ROLLOUT_SCENES refuses such a planner with m3_batch_command's own
 * code and message, before anything of the tick is launched.  The world side is unchanged: row e steps in the WORLD handle's
 * arena (its compiled-in scene, m3_set_point_scene or m3_set_point_scene_rows); a planner's rows are the arenas of its
 * rollout's samples only.  Rows set or cleared (m3_set_point_rollout_scenes) between two ticks apply from the next tick.  The
 * set allocates what m3_episodes_create allocates, at create; a tick allocates nothing. */
#define M3_EPISODES_ROLLOUT_SCENES 1
int m3_episodes_create_ex(m3_handle* world, m3_handle* const* planners, const m3_episode_spec* specs, int n, int max_ticks,
                          int trace, int flags, m3_episodes** out);
int m3_episodes_flags(const m3_episodes* eps);   /* the flags it was created with; M3_ERR_BAD_ARG for NULL */

#ifdef __cplusplus
}
#endif
#endif
