// Host program of the panda_env variant decision for tests/test_panda_variant_cpu.py: the product's csrc/panda_variant.hpp
// compiled by g++ (it has no HIP dependency).  It walks every input -- 3 x 3 settings of the two instance switches x 2^5 flags --
// and compares, per side, the header's answer (variant, both "used" records, the refusal that wins) with the if-chains of
// m3_api.hip as they stood BEFORE the header existed (commit f6e002f), transcribed below line by line onto a struct with the
// handle's field names: the reference is that commit, not the code under test.  Then the properties the kernels rely on.
// A program with its own main, so that it also runs under -fsanitize=address,undefined as it is.
//   g++ -O2 -std=c++17 panda_variant_host.cpp -o panda_variant_host && ./panda_variant_host
#include <cstdio>

#include "../../m3p2i_aip_amd/csrc/panda_variant.hpp"

namespace {
using namespace m3;

long checks = 0;
int failures = 0;

// ---- the reference: m3_api.hip of f6e002f ------------------------------------------------------------------------------------
struct Handle {   // the fields the chains read (every handle here is a panda_env handle)
    int panda_scene_instance, panda_weighted_instance;
    bool geometry_default, weights_default;   // panda_scene_geometry_is_default(h->panda_scene), default_panda_cost_weights(h)
    bool panda_rollout_scenes_on, panda_scene_rows_on, sim_only;
    int panda_scene_used, panda_weighted_used;
};
const int KEPT = 77;   // what the "used" records hold before a call: a call that leaves one alone leaves this

bool ref_scene_runtime(const Handle* h) {
    return h->panda_scene_instance < 0 ? !h->geometry_default : h->panda_scene_instance != 0;
}
PandaRefusal ref_scene_refusal(const Handle* h) {
    if (h->panda_scene_instance == 0 && h->panda_scene_rows_on) return PANDA_SCENE_OFF_ENV_ROWS;
    if (h->panda_scene_instance == 0 && h->panda_rollout_scenes_on) return PANDA_SCENE_OFF_SAMPLE_ROWS;
    if (h->panda_scene_instance == 0 && !h->geometry_default) return PANDA_SCENE_OFF_GEOMETRY;
    return PANDA_REFUSAL_NONE;
}
PandaRefusal ref_scene_unbatched(const Handle* h) { return ref_scene_runtime(h) ? PANDA_UNBATCHED_SCENE : PANDA_REFUSAL_NONE; }
PandaRefusal ref_rows_unbatched(const Handle* h) {
    if (h->panda_rollout_scenes_on) return PANDA_UNBATCHED_SAMPLE_ROWS;
    if (h->panda_scene_rows_on) return PANDA_UNBATCHED_ENV_ROWS;
    return PANDA_REFUSAL_NONE;
}
bool ref_weighted(const Handle* h) {
    return h->panda_weighted_instance < 0 ? !h->weights_default : h->panda_weighted_instance != 0;
}
PandaRefusal ref_weights_refusal(const Handle* h) {
    if (h->panda_weighted_instance == 0 && !h->weights_default) return PANDA_WEIGHTS_OFF_TUNED;
    return PANDA_REFUSAL_NONE;
}
PandaRefusal ref_weights_unbatched(const Handle* h) {
    return (!h->sim_only && ref_weighted(h)) ? PANDA_UNBATCHED_WEIGHTS : PANDA_REFUSAL_NONE;
}
// rollout_refusal's panda part
PandaRefusal ref_rollout_refusal(const Handle* h) {
    if (PandaRefusal why = ref_scene_refusal(h)) return why;
    if (PandaRefusal why = ref_weights_refusal(h)) return why;
    return PANDA_REFUSAL_NONE;
}
// m3_rollout (1484-1493): which launcher, what it records
PandaVariant ref_rollout(Handle* h) {
    if (h->panda_rollout_scenes_on) {
        h->panda_scene_used = 1; h->panda_weighted_used = ref_weighted(h) ? 1 : 0;
        return PANDA_ROWS;      // launch_rollout_panda_v
    }
    else if (ref_weighted(h)) {
        h->panda_scene_used = ref_scene_runtime(h) ? 1 : 0; h->panda_weighted_used = 1;
        return PANDA_WEIGHTED;  // launch_rollout_panda_w
    }
    else if (ref_scene_runtime(h)) { h->panda_scene_used = 1; h->panda_weighted_used = 0; return PANDA_SCENE; }   // launch_rollout_panda_s
    else { h->panda_scene_used = 0; h->panda_weighted_used = 0; return PANDA_LITERAL; }                           // launch_rollout_panda
}
// m3_sim_pull_state / m3_sim_push_state (2503-2505, 2525-2527)
PandaVariant ref_views(const Handle* h) {
    if (h->panda_scene_rows_on) return PANDA_ROWS;          // launch_psim_pull_v / _push_v
    else if (ref_scene_runtime(h)) return PANDA_SCENE;      // launch_psim_pull_s / _push_s
    else return PANDA_LITERAL;
}
// sim_step_impl (2562-2566)
PandaVariant ref_step(Handle* h) {
    h->panda_scene_used = (h->panda_scene_rows_on || ref_scene_runtime(h)) ? 1 : 0;
    if (h->panda_scene_rows_on) return PANDA_ROWS;          // launch_psim_step_v
    else if (h->panda_scene_used) return PANDA_SCENE;       // launch_psim_step_s
    else return PANDA_LITERAL;
}
// m3_cost (2619-2627)
PandaRefusal ref_cost_refusal(const Handle* h) {
    if (PandaRefusal why = ref_scene_refusal(h)) return why;
    if (PandaRefusal why = ref_weights_refusal(h)) return why;
    return PANDA_REFUSAL_NONE;
}
PandaVariant ref_cost(Handle* h) {
    h->panda_weighted_used = ref_weighted(h) ? 1 : 0;
    if (h->panda_scene_rows_on) return PANDA_ROWS;          // launch_psim_cost_v
    else if (h->panda_weighted_used) return PANDA_WEIGHTED; // launch_psim_cost_w
    else if (ref_scene_runtime(h)) return PANDA_SCENE;      // launch_psim_cost_s
    else return PANDA_LITERAL;
}
// batch_panda_variant (2235) and the record behind the batched launch (2350-2357)
int ref_batch_variant(const Handle* h) {
    if (h->panda_rollout_scenes_on) return 2;
    return (ref_weighted(h) || ref_scene_runtime(h)) ? 1 : 0;
}
void ref_batch_record(Handle* h, int variant) {
    const bool rt = ref_scene_runtime(h), wt = ref_weighted(h);
    if (variant == 2) { h->panda_scene_used = 1; h->panda_weighted_used = wt ? 1 : 0; }
    else if (wt) { h->panda_scene_used = rt ? 1 : 0; h->panda_weighted_used = 1; }
    else { h->panda_scene_used = rt ? 1 : 0; h->panda_weighted_used = 0; }
}
// batch_refusal without the run-time section (2204-2215) and m3_panda_episodes_create's world (2931-2932): scene, rows, weights
PandaRefusal ref_unbatched_batch(const Handle* h) {
    if (PandaRefusal why = ref_scene_unbatched(h)) return why;
    if (PandaRefusal why = ref_rows_unbatched(h)) return why;
    if (PandaRefusal why = ref_weights_unbatched(h)) return why;
    return PANDA_REFUSAL_NONE;
}
// peps_ready (3039-3041): scene, weights, rows
PandaRefusal ref_unbatched_ticks(const Handle* h) {
    PandaRefusal why = PANDA_REFUSAL_NONE;
    if (!why) why = ref_scene_unbatched(h);
    if (!why) why = ref_weights_unbatched(h);
    if (!why) why = ref_rows_unbatched(h);
    return why;
}

// ---- the comparison ------------------------------------------------------------------------------------------------------------
const PandaVariantInput* at = nullptr;
void expect(bool ok, const char* what) {
    ++checks;
    if (ok) return;
    if (++failures <= 20)
        std::fprintf(stderr, "FAIL %s: scene_instance %d weighted_instance %d geometry_default %d weights_default %d "
                             "rollout_scenes_on %d scene_rows_on %d sim_only %d\n",
                     what, at->scene_instance, at->weighted_instance, at->geometry_default, at->weights_default,
                     at->rollout_scenes_on, at->scene_rows_on, at->sim_only);
}
// what a record holds after m3_api.hip applied a decision to it
int applied(int used) { return used == PANDA_USED_UNCHANGED ? KEPT : used; }
void same(const PandaDecision& d, PandaVariant variant, const Handle& after, PandaRefusal refusal, const char* side) {
    char what[96];
    std::snprintf(what, sizeof(what), "%s: variant", side);
    expect(d.variant == variant, what);
    std::snprintf(what, sizeof(what), "%s: panda_scene_used", side);
    expect(applied(d.scene_used) == after.panda_scene_used, what);
    std::snprintf(what, sizeof(what), "%s: panda_weighted_used", side);
    expect(applied(d.weighted_used) == after.panda_weighted_used, what);
    std::snprintf(what, sizeof(what), "%s: refusal", side);
    expect(d.refusal == refusal, what);
}
}  // namespace

int main() {
    for (int si = -1; si <= 1; ++si)
        for (int wi = -1; wi <= 1; ++wi)
            for (int flags = 0; flags < 32; ++flags) {
                PandaVariantInput in;
                in.scene_instance = si;
                in.weighted_instance = wi;
                in.geometry_default = (flags & 1) != 0;
                in.weights_default = (flags & 2) != 0;
                in.rollout_scenes_on = (flags & 4) != 0;
                in.scene_rows_on = (flags & 8) != 0;
                in.sim_only = (flags & 16) != 0;
                at = &in;
                const Handle h0 = {si, wi, in.geometry_default, in.weights_default, in.rollout_scenes_on, in.scene_rows_on,
                                   in.sim_only, KEPT, KEPT};
                expect(panda_scene_runtime(in) == ref_scene_runtime(&h0), "panda_scene_runtime");
                expect(panda_weighted(in) == ref_weighted(&h0), "panda_weighted");
                {
                    Handle h = h0;
                    const PandaVariant v = ref_rollout(&h);
                    same(panda_decision(in, PANDA_SIDE_ROLLOUT), v, h, ref_rollout_refusal(&h0), "rollout");
                }
                {
                    Handle h = h0;
                    const PandaVariant v = ref_step(&h);
                    same(panda_decision(in, PANDA_SIDE_STEP), v, h, ref_scene_refusal(&h0), "step");
                }
                same(panda_decision(in, PANDA_SIDE_VIEWS), ref_views(&h0), h0, ref_scene_refusal(&h0), "views");
                {
                    Handle h = h0;
                    const PandaVariant v = ref_cost(&h);
                    same(panda_decision(in, PANDA_SIDE_COST), v, h, ref_cost_refusal(&h0), "cost");
                }
                {
                    Handle h = h0;
                    const int key = ref_batch_variant(&h0);
                    ref_batch_record(&h, key);
                    const PandaDecision d = panda_decision(in, PANDA_SIDE_BATCH);
                    // (the variant of the batch side is one of the table's three constructions; its key is the parent's integer)
                    same(d, key == 2 ? PANDA_ROWS : key == 1 ? PANDA_WEIGHTED : PANDA_LITERAL, h, ref_rollout_refusal(&h0), "batch");
                    expect(panda_batch_key(d.variant) == key, "batch: BatchKey::variant");
                    expect(panda_general_only(d.variant) == (key != 0), "batch: roll.general forced for the run-time section");
                    expect((d.variant == PANDA_LITERAL) == (key == 0), "batch: the literal section holds variant 0 only");
                    expect((d.variant == PANDA_ROWS) == (key == 2), "batch: the entry carries rows for variant 2 only");
                    // property: variant 2 exactly when the handle has a workspace per sample
                    expect((panda_batch_key(d.variant) == 2) == in.rollout_scenes_on, "batch: variant 2 iff rollout_scenes_on");
                }
                expect(panda_unbatched(in, PANDA_ROWS_THEN_WEIGHTS) == ref_unbatched_batch(&h0), "unbatched: scene, rows, weights");
                expect(panda_unbatched(in, PANDA_WEIGHTS_THEN_ROWS) == ref_unbatched_ticks(&h0), "unbatched: scene, weights, rows");
                if (in.sim_only) {   // (m3_panda_episodes_create asks its world, a sim_only handle, about the scene and rows only)
                    PandaRefusal why = ref_scene_unbatched(&h0);
                    if (!why) why = ref_rows_unbatched(&h0);
                    expect(panda_unbatched(in, PANDA_ROWS_THEN_WEIGHTS) == why, "unbatched: the episodes' world");
                }
                // ---- properties ----
                const PandaSide sides[] = {PANDA_SIDE_ROLLOUT, PANDA_SIDE_STEP, PANDA_SIDE_VIEWS, PANDA_SIDE_COST, PANDA_SIDE_BATCH};
                for (PandaSide side : sides) {
                    const PandaDecision d = panda_decision(in, side);
                    const bool rows_here = (side == PANDA_SIDE_ROLLOUT || side == PANDA_SIDE_BATCH) ? in.rollout_scenes_on : in.scene_rows_on;
                    // all defaults: the literal kernels on every side, both records 0 wherever the side writes them
                    if (si < 0 && wi < 0 && in.geometry_default && in.weights_default && !in.rollout_scenes_on && !in.scene_rows_on) {
                        expect(d.variant == PANDA_LITERAL && d.refusal == PANDA_REFUSAL_NONE, "defaults: the literal kernels, no refusal");
                        expect(d.scene_used <= 0 && d.weighted_used <= 0, "defaults: both records 0 (or left alone)");
                    }
                    // rows on a side: the rows kernels, and the scene record 1 wherever the side writes it
                    if (rows_here) {
                        expect(d.variant == PANDA_ROWS, "rows: the rows kernels");
                        expect(d.scene_used == 1 || d.scene_used == PANDA_USED_UNCHANGED, "rows: panda_scene_used 1");
                        if (side == PANDA_SIDE_ROLLOUT || side == PANDA_SIDE_STEP || side == PANDA_SIDE_BATCH)
                            expect(d.scene_used == 1, "rows: the rollout, the batch and the step record panda_scene_used 1");
                    } else expect(d.variant != PANDA_ROWS, "no rows: never the rows kernels");
                    // the step and the views have no weighted form
                    if (side == PANDA_SIDE_STEP || side == PANDA_SIDE_VIEWS) expect(d.variant != PANDA_WEIGHTED, "step / views: no weighted form");
                }
                {   // the cost side never depends on geometry alone: with the scene switch left alone (forced off, a changed geometry
                    // is a refusal by design) the same answer for either geometry, unless the geometry is what selects the kernel
                    PandaVariantInput other = in;
                    other.geometry_default = !in.geometry_default;
                    const PandaDecision a = panda_decision(in, PANDA_SIDE_COST), b = panda_decision(other, PANDA_SIDE_COST);
                    expect(a.weighted_used == b.weighted_used && a.scene_used == b.scene_used, "cost: the records do not depend on geometry");
                    if (a.variant != b.variant)
                        expect((a.variant == PANDA_SCENE && b.variant == PANDA_LITERAL) || (a.variant == PANDA_LITERAL && b.variant == PANDA_SCENE),
                               "cost: geometry only moves the literal cost between the compiled-in and the run-time scene");
                    expect(panda_cost_weighted(a.variant) == panda_cost_weighted(b.variant), "cost: weighted or literal cost regardless of geometry");
                }
            }
    std::printf("%ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
