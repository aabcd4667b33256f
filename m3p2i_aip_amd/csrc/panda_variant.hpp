// panda_variant.hpp -- which panda_env kernels a handle runs, what the launch records and why a path refuses the handle: decided
// here and nowhere else (host only; no HIP dependency, so that tests/native/panda_variant_host.cpp can walk every input on its
// own).  m3_api.hip fills PandaVariantInput from the handle and maps the refusals to their texts; the launchers of
// m3_internal.hpp take the variant.  DESIGN.md section 7h.
#pragma once

namespace m3 {

// the kernel families (the files they live in: rollout_panda.hip, rollout_panda_scene.hip, rollout_panda_weights.hip,
// rollout_panda_rows.hip, rollout_panda_priors.hip; their table forms in rollout_panda.hip and rollout_panda_batch_rt.hip)
enum PandaVariant {
    PANDA_LITERAL,    // the reference's workspace and cost weights compiled in
    PANDA_SCENE,      // the workspace a kernel argument (PandaSceneRT), the literal cost
    PANDA_WEIGHTED,   // ... and the cost weights a kernel argument (PandaCostWeights)
    PANDA_ROWS,       // ... and the workspace words of a lane from its row of the handle's table; weights always
    PANDA_PRIORS      // ... and the controls of some samples the caller's sequences (m3_set_panda_prior_samples); the rows optional
};
// the families whose cost is the weighted overload of panda_cost (the reach-cost kernel behind their rollout is the weighted one)
constexpr bool panda_cost_weighted(PandaVariant v) { return v == PANDA_WEIGHTED || v == PANDA_ROWS || v == PANDA_PRIORS; }
// every family but the literal one exists as GENERAL builds only: the plan's choice of the literal kernel's build means nothing
constexpr bool panda_general_only(PandaVariant v) { return v != PANDA_LITERAL; }
// BatchKey::variant of a batch-side variant: 0 kb_rollout_panda (the literal section of the table), 1 kb_rollout_panda_w,
// 2 kb_rollout_panda_v (the run-time section)
constexpr int panda_batch_key(PandaVariant v) { return v == PANDA_ROWS ? 2 : v == PANDA_LITERAL ? 0 : 1; }

struct PandaVariantInput {
    int scene_instance;       // m3_set_panda_scene_instance: -1 by the values, 0 / 1 forced
    int weighted_instance;    // m3_set_panda_weighted_cost_instance: -1 by the weights, 0 / 1 forced
    bool geometry_default;    // the workspace is the reference's but for the two masses (panda_scene_geometry_is_default)
    bool weights_default;     // the cost weights are the defaults bit for bit
    bool rollout_scenes_on;   // m3_set_panda_rollout_scenes: a workspace per sample of the fused rollout
    bool scene_rows_on;       // m3_set_panda_scene_rows: a workspace per environment of a sim_only handle
    bool sim_only;
    bool priors_on = false;   // m3_set_panda_prior_samples: samples of the fused rollout that take the caller's sequences
};

enum PandaSide {
    PANDA_SIDE_ROLLOUT,   // m3_rollout / m3_command
    PANDA_SIDE_STEP,      // m3_sim_step*
    PANDA_SIDE_VIEWS,     // m3_sim_pull_state / m3_sim_push_state
    PANDA_SIDE_COST,      // m3_cost
    PANDA_SIDE_BATCH      // m3_batch_command with the run-time section: LITERAL, WEIGHTED (a run-time scene alone too) or ROWS
};

enum PandaRefusal {
    PANDA_REFUSAL_NONE,
    // the handle cannot run its own kernels (M3_ERR_STATE)
    PANDA_SCENE_OFF_ENV_ROWS,       // the run-time-scene instance is forced off but ... a workspace per environment
    PANDA_SCENE_OFF_SAMPLE_ROWS,    // ... a workspace per sample
    PANDA_SCENE_OFF_GEOMETRY,       // ... a workspace that is not the default
    PANDA_WEIGHTS_OFF_TUNED,        // the weighted cost instance is forced off but the weights are not the defaults
    // a path whose kernels know the literal family only cannot take the handle (M3_ERR_UNSUPPORTED)
    PANDA_UNBATCHED_SCENE,
    PANDA_UNBATCHED_SAMPLE_ROWS,
    PANDA_UNBATCHED_ENV_ROWS,
    PANDA_UNBATCHED_WEIGHTS,
    // prior samples (m3_set_panda_prior_samples): their kernels are run-time-scene, weighted kernels (M3_ERR_STATE) ...
    PANDA_SCENE_OFF_PRIORS,         // the run-time-scene instance is forced off but the handle has prior samples
    PANDA_WEIGHTS_OFF_PRIORS,       // the weighted cost instance is forced off but the handle has prior samples
    // ... that only m3_rollout / m3_command launch (M3_ERR_UNSUPPORTED)
    PANDA_UNBATCHED_PRIORS
};

constexpr int PANDA_USED_UNCHANGED = -1;
struct PandaDecision {
    PandaVariant variant;
    int scene_used, weighted_used;   // what panda_scene_used / panda_weighted_used become: 0, 1 or PANDA_USED_UNCHANGED
    PandaRefusal refusal;            // of the handle's own kernels on this side; the rest is what an accepted call does
};

// the run-time-scene instances: by the values -- anything but the two masses off the defaults -- or as the switch says
inline bool panda_scene_runtime(const PandaVariantInput& in) {
    return in.scene_instance < 0 ? !in.geometry_default : in.scene_instance != 0;
}
// the weighted kernels (on the run-time scene, whatever panda_scene_runtime says): by the weights, or as the switch says
inline bool panda_weighted(const PandaVariantInput& in) {
    return in.weighted_instance < 0 ? !in.weights_default : in.weighted_instance != 0;
}

// why the handle cannot run its kernels.  The rows' kernels are run-time-scene kernels, so the scene switch refuses rows on
// every side; the weights matter where a cost is formed.
inline PandaRefusal panda_refusal(const PandaVariantInput& in, PandaSide side) {
    // (no table entry carries a slot map and a table of priors: ahead of everything the handle's own kernels would refuse)
    if (side == PANDA_SIDE_BATCH && in.priors_on) return PANDA_UNBATCHED_PRIORS;
    if (in.scene_instance == 0 && in.scene_rows_on) return PANDA_SCENE_OFF_ENV_ROWS;
    if (in.scene_instance == 0 && in.rollout_scenes_on) return PANDA_SCENE_OFF_SAMPLE_ROWS;
    if (in.scene_instance == 0 && !in.geometry_default) return PANDA_SCENE_OFF_GEOMETRY;
    const bool forms_cost = side == PANDA_SIDE_ROLLOUT || side == PANDA_SIDE_COST || side == PANDA_SIDE_BATCH;
    if (forms_cost && in.weighted_instance == 0 && !in.weights_default) return PANDA_WEIGHTS_OFF_TUNED;
    // (the prior family is one: run-time scene and weighted cost.  The rollout alone launches it)
    if (side == PANDA_SIDE_ROLLOUT && in.priors_on && in.scene_instance == 0) return PANDA_SCENE_OFF_PRIORS;
    if (side == PANDA_SIDE_ROLLOUT && in.priors_on && in.weighted_instance == 0) return PANDA_WEIGHTS_OFF_PRIORS;
    return PANDA_REFUSAL_NONE;
}

inline PandaDecision panda_decision(const PandaVariantInput& in, PandaSide side) {
    const bool rt = panda_scene_runtime(in), wt = panda_weighted(in);
    PandaDecision d{PANDA_LITERAL, PANDA_USED_UNCHANGED, PANDA_USED_UNCHANGED, panda_refusal(in, side)};
    switch (side) {
        case PANDA_SIDE_ROLLOUT:
        case PANDA_SIDE_BATCH:
            // rows: one family, weights always; weighted: one family on the run-time scene.  "used" keeps saying whether the
            // WEIGHTS / the WORKSPACE needed the instance
            d.variant = in.rollout_scenes_on ? PANDA_ROWS : wt ? PANDA_WEIGHTED : rt ? PANDA_SCENE : PANDA_LITERAL;
            d.scene_used = (in.rollout_scenes_on || rt) ? 1 : 0;
            d.weighted_used = wt ? 1 : 0;
            // (the table's run-time section has ONE construction for a scene, weights or both: rollout_panda_batch_rt.hip)
            if (side == PANDA_SIDE_BATCH && d.variant == PANDA_SCENE) d.variant = PANDA_WEIGHTED;
            // prior samples win over every other family (the batch side refuses them: panda_refusal); the workspace is a kernel
            // argument in all their kernels, "weighted" keeps saying whether the WEIGHTS needed the instance
            if (side == PANDA_SIDE_ROLLOUT && in.priors_on) { d.variant = PANDA_PRIORS; d.scene_used = 1; }
            break;
        case PANDA_SIDE_STEP:
            d.scene_used = (in.scene_rows_on || rt) ? 1 : 0;
            [[fallthrough]];        // (the kernels: as the views')
        case PANDA_SIDE_VIEWS:      // (step, pull and push read no cost: no weighted form)
            d.variant = in.scene_rows_on ? PANDA_ROWS : rt ? PANDA_SCENE : PANDA_LITERAL;
            break;
        case PANDA_SIDE_COST:       // (rows: one kernel, weights always -- at the defaults the literal cost's bits)
            d.variant = in.scene_rows_on ? PANDA_ROWS : wt ? PANDA_WEIGHTED : rt ? PANDA_SCENE : PANDA_LITERAL;
            d.weighted_used = wt ? 1 : 0;
            break;
    }
    return d;
}

// Why a path that carries a PandaScene and the literal cost only (a batch table without the run-time section, the lockstep
// episodes' kernels) cannot take the handle.  A sim_only handle passes the weights: its step reads none.  Which message wins
// when several conditions hold is part of each caller's contract, so the order is an argument: the scene comes first, then
// rows before weights (m3_batch_command, m3_panda_episodes_create) or weights before rows (the episodes' ticks).
enum PandaUnbatchedOrder { PANDA_ROWS_THEN_WEIGHTS, PANDA_WEIGHTS_THEN_ROWS };
inline PandaRefusal panda_unbatched(const PandaVariantInput& in, PandaUnbatchedOrder order) {
    if (in.priors_on) return PANDA_UNBATCHED_PRIORS;
    if (panda_scene_runtime(in)) return PANDA_UNBATCHED_SCENE;
    const PandaRefusal rows = in.rollout_scenes_on ? PANDA_UNBATCHED_SAMPLE_ROWS
                              : in.scene_rows_on   ? PANDA_UNBATCHED_ENV_ROWS
                                                   : PANDA_REFUSAL_NONE;
    const PandaRefusal weights = (!in.sim_only && panda_weighted(in)) ? PANDA_UNBATCHED_WEIGHTS : PANDA_REFUSAL_NONE;
    const PandaRefusal first = order == PANDA_ROWS_THEN_WEIGHTS ? rows : weights;
    const PandaRefusal second = order == PANDA_ROWS_THEN_WEIGHTS ? weights : rows;
    return first != PANDA_REFUSAL_NONE ? first : second;
}

// The lockstep episodes (m3_panda_episodes_*) come in two modes.  A set made by m3_panda_episodes_create runs the literal pre and
// post kernels and hands its planners to the literal section of a batch table: it takes what panda_unbatched passes.  A set made
// with M3_PANDA_EPISODES_RUNTIME runs the rows kernels on its own two tables (a single scene is n equal rows: one family) and
// hands its planners to the batch's run-time section: nothing is "unbatched" any more, what remains is what the handle's own
// kernels refuse -- the forced-off switches, on the step side for the world (its step reads no weight) and on the batch side for
// a planner.  `order` is read by the literal mode only.
enum PandaEpisodesMode { PANDA_EPISODES_LITERAL, PANDA_EPISODES_RUNTIME };
constexpr PandaVariant panda_episodes_variant(PandaEpisodesMode mode) { return mode == PANDA_EPISODES_RUNTIME ? PANDA_ROWS : PANDA_LITERAL; }
inline PandaRefusal panda_episodes_refusal(const PandaVariantInput& in, PandaEpisodesMode mode, PandaUnbatchedOrder order) {
    if (mode == PANDA_EPISODES_LITERAL) return panda_unbatched(in, order);
    return panda_refusal(in, in.sim_only ? PANDA_SIDE_STEP : PANDA_SIDE_BATCH);
}
// the refusals of panda_refusal are M3_ERR_STATE (but the batch side's PANDA_UNBATCHED_PRIORS), those of panda_unbatched
// M3_ERR_UNSUPPORTED
constexpr bool panda_refusal_is_state(PandaRefusal r) {
    return (r >= PANDA_SCENE_OFF_ENV_ROWS && r <= PANDA_WEIGHTS_OFF_TUNED) || r == PANDA_SCENE_OFF_PRIORS || r == PANDA_WEIGHTS_OFF_PRIORS;
}

}  // namespace m3
