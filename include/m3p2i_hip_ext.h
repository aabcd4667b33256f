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

/* ---- prior samples from an ancillary controller ON THE DEVICE ----
 * On request (additive; M3_ABI_VERSION stays 4): a handle without a controller launches exactly the kernels and returns exactly
 * the codes and messages it did.  m3_set_prior_samples takes sequences a caller computed; a controller is a rule the LIBRARY
 * evaluates, on the device, from the world each rollout starts from: one small kernel (k_prior_controllers, one lane per
 * sequence) on the handle's stream directly ahead of the rollout of m3_rollout / m3_command fills the handle's table of prior
 * samples -- no upload, no synchronisation, no allocation, nothing to do per tick on the host.  Robot and box are those of the
 * world the rollout reads (row 0 of bound views, else m3_set_world_point's); the goal is the objective's (m3_set_objective);
 * dt and u_max are the handle's.  The arithmetic is csrc/prior_controllers.hpp, binary32 in a fixed order (its text is the
 * spec; a host build of it gives the kernel's bits):
 *   one drive step   d = target - pos; dist = |d|; dist > 0: v = min(dist / dt, speed), u = (d / dist) * v, else u = 0;
 *                    pos += u * dt
 *   GO_TO            T drive steps toward the goal
 *   PUSH_BEHIND      behind = box + standoff * (box - goal) / |box - goal|  ((1, 0) for a box at the goal); toward `behind`
 *                    until |behind - pos| <= reach (tested before each step), toward the goal from then on
 *   speed of seq j   speed[j] * min(|u_max[0]|, |u_max[1]|)
 * No clamp (the rollout's select clamps) and no contacts (what the rollout is for).
 * m3_set_prior_controller(h, pc, sample_idx): sequence j becomes the prior of GLOBAL sample sample_idx[j] (pc->n indices).
 * Every check m3_set_prior_samples makes on the handle and on the indices, with its codes; besides, M3_ERR_BAD_ARG for an
 * unknown kind, n outside 1 .. M3_MAX_PRIOR_CONTROLLER_SEQS, a factor, standoff or reach that is not finite or not positive;
 * every check before any state changes.  Allocates what the first m3_set_prior_samples call on the handle allocates, through
 * the same ledger entries, and nothing more.  pc == NULL clears controller and priors.  Against m3_set_prior_samples[_device]
 * the last call wins.  Survives m3_reset.  m3_prior_samples_set returns n; m3_get_prior_sample with seq != NULL is
 * M3_ERR_STATE, as after the device setter.  PUSH_BEHIND on a handle whose task is navigation refuses the rollout
 * (M3_ERR_STATE, before any launch): it is not silently downgraded.
 * Like every handle with priors, one with a controller is refused by m3_batch_command and m3_episodes_* unless the batch and
 * the set were created for priors (M3_BATCH_SECTION_POINT_PRIORS, M3_EPISODES_PRIORS below). */
#define M3_PRIOR_CONTROLLER_GO_TO 1
#define M3_PRIOR_CONTROLLER_PUSH_BEHIND 2
#define M3_MAX_PRIOR_CONTROLLER_SEQS 16
typedef struct {
    int   kind;        /* M3_PRIOR_CONTROLLER_GO_TO = 1, M3_PRIOR_CONTROLLER_PUSH_BEHIND = 2 */
    int   n;           /* 1 .. M3_MAX_PRIOR_CONTROLLER_SEQS (16) */
    float speed[16];   /* factors of the speed limit */
    float standoff;
    float reach;
} m3_prior_controller;
/* the defaults of priors.py: speeds 1 - j / n, standoff 0.45, reach 0.05 (n outside 1 .. 16: clamped into it) */
void m3_default_prior_controller(m3_prior_controller* pc, int kind, int n);
int m3_set_prior_controller(m3_handle* h, const m3_prior_controller* pc, const int* sample_idx);
int m3_get_prior_controller(const m3_handle* h, m3_prior_controller* out);   /* out->kind == 0: none */
/* launches the controller alone, for the world currently set or bound and the current objective (the step path and the tests
 * read the table behind it); M3_ERR_STATE without a controller or where the rollout would refuse the handle */
int m3_prior_controller_fill(m3_handle* h);
/* a read-only view of the handle's table of prior samples: device, [M3_MAX_PRIOR_SAMPLES][T][nu] of which *n rows are set
 * (stream-ordered: written by the setters' copies and the controller kernel on the handle's stream); M3_ERR_STATE before the
 * first setter call */
int m3_prior_table(const m3_handle* h, const float** tab_dev, int* n);

/* ---- batched command and lockstep episodes of point_env planners with prior samples ----
 * On request (additive).  m3_batch_create, m3_batch_create_ex and every batch without the bit below keep refusing a handle with
 * prior samples, in the words they always had.
 * M3_BATCH_SECTION_POINT_PRIORS (m3_batch_create_sections) sizes the slots for a FIFTH section of point_env rollout entries,
 * behind the per-sample one: m3_batch_command on such a batch accepts, besides everything else, an unsharded point_env planner
 * handle with prior samples -- set on the host, on the device or by a controller, with or without an arena per sample (the
 * section's entry carries the rows too, so such a handle needs no M3_BATCH_SECTION_POINT_ROLLOUT_SCENES).  Its value is 32: 4, 8
 * and 16 stay "unknown section bits", as callers have been told.  Such handles sort last and are grouped by K, T and lanes per
 * wavefront (one kernel family, kb_rollout_point_pr*: handles with different tasks, weights, dt, rows and priors share a launch),
 * one rollout launch per group, counted by m3_batch_launches.  Ahead of the rollout launches, ONE launch of the batched
 * controller kernel (kb_prior_controllers, not counted) serves every entry with a controller.  An entry points at the handle's
 * OWN slot map, table of priors and rows: the batch stores none of them and a call allocates nothing.  Each handle's results are
 * bit-identical to its own m3_command's.  Every other refusal of m3_batch_command stays, in the same order and words.
 * M3_EPISODES_PRIORS (m3_episodes_create_ex; value 8: 2 and 4 stay unknown): a set created with it accepts planners with prior
 * samples at create, tick, begin and end; a set without it keeps refusing them.  m3_episodes_tick passes the batch's own bit on:
 * a batch without the priors section refuses such a planner with m3_batch_command's code and message, ahead of the pre kernel,
 * so nothing of the tick is launched.  Planner e is bound to row e of the world, so its controller reads episode e's robot and
 * box every tick, on the device.  Priors set or cleared between two ticks apply from the next tick.  The set allocates nothing
 * new. */
#define M3_BATCH_SECTION_POINT_PRIORS 32
#define M3_EPISODES_PRIORS 8

#ifdef __cplusplus
}
#endif
#endif
