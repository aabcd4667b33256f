// Host program of the panda_env variant decision WITH PRIOR SAMPLES for tests/test_panda_prior_samples_cpu.py: the product's
// csrc/panda_variant.hpp compiled by g++.  It walks priors_on over every other input -- 3 x 3 settings of the two instance
// switches x 2^5 flags -- and checks the rules of DESIGN.md section 7l against the header's own answer for the same input WITHOUT
// prior samples (which tests/native/panda_variant_host.cpp pins to the if-chains of the commit before the header existed):
//   rollout: the prior family wins over every other, panda_scene_used = 1, panda_weighted_used as without priors; what refused
//            without priors still refuses, with the same reason; else a forced-off scene or weighted switch refuses (STATE);
//   batch:   PANDA_UNBATCHED_PRIORS (UNSUPPORTED) ahead of everything; panda_unbatched and the episodes' refusal alike;
//   step, views, cost: priors_on is not read.
// A program with its own main, so that it also runs under -fsanitize=address,undefined as it is.
//   g++ -O2 -std=c++17 panda_variant_priors_host.cpp -o panda_variant_priors_host && ./panda_variant_priors_host
#include <cstdio>

#include "../../m3p2i_aip_amd/csrc/panda_variant.hpp"

namespace {
using namespace m3;

long checks = 0;
int failures = 0;
const PandaVariantInput* at = nullptr;

void expect(bool ok, const char* what) {
    ++checks;
    if (ok) return;
    if (++failures <= 20)
        std::fprintf(stderr, "FAIL %s: scene_instance %d weighted_instance %d geometry_default %d weights_default %d "
                             "rollout_scenes_on %d scene_rows_on %d sim_only %d priors_on %d\n",
                     what, at->scene_instance, at->weighted_instance, at->geometry_default, at->weights_default,
                     at->rollout_scenes_on, at->scene_rows_on, at->sim_only, at->priors_on);
}
bool same(const PandaDecision& a, const PandaDecision& b) {
    return a.variant == b.variant && a.scene_used == b.scene_used && a.weighted_used == b.weighted_used && a.refusal == b.refusal;
}
bool is_priors_refusal(PandaRefusal r) { return r == PANDA_SCENE_OFF_PRIORS || r == PANDA_WEIGHTS_OFF_PRIORS || r == PANDA_UNBATCHED_PRIORS; }
}  // namespace

int main() {
    // a default-constructed input has no prior samples: what tests/native/panda_variant_host.cpp declares and fills stays valid
    expect(!PandaVariantInput{}.priors_on, "priors_on defaults to false");
    expect(panda_cost_weighted(PANDA_PRIORS), "the prior family forms the weighted cost (the weighted reach-cost kernel behind it)");
    expect(panda_general_only(PANDA_PRIORS), "the prior family has GENERAL builds only");
    expect(panda_refusal_is_state(PANDA_SCENE_OFF_PRIORS) && panda_refusal_is_state(PANDA_WEIGHTS_OFF_PRIORS), "forced off: M3_ERR_STATE");
    expect(!panda_refusal_is_state(PANDA_UNBATCHED_PRIORS), "unbatched: M3_ERR_UNSUPPORTED");
    expect(PANDA_PRIORS > PANDA_ROWS, "PANDA_PRIORS at the end of the enum");
    const PandaSide sides[] = {PANDA_SIDE_ROLLOUT, PANDA_SIDE_STEP, PANDA_SIDE_VIEWS, PANDA_SIDE_COST, PANDA_SIDE_BATCH};
    const PandaUnbatchedOrder orders[] = {PANDA_ROWS_THEN_WEIGHTS, PANDA_WEIGHTS_THEN_ROWS};
    for (int si = -1; si <= 1; ++si)
        for (int wi = -1; wi <= 1; ++wi)
            for (int flags = 0; flags < 32; ++flags) {
                PandaVariantInput off;
                off.scene_instance = si;
                off.weighted_instance = wi;
                off.geometry_default = (flags & 1) != 0;
                off.weights_default = (flags & 2) != 0;
                off.rollout_scenes_on = (flags & 4) != 0;
                off.scene_rows_on = (flags & 8) != 0;
                off.sim_only = (flags & 16) != 0;
                PandaVariantInput on = off;
                on.priors_on = true;
                // ---- without priors: never the family, never one of its refusals ----
                at = &off;
                for (PandaSide side : sides) {
                    const PandaDecision d = panda_decision(off, side);
                    expect(d.variant != PANDA_PRIORS && !is_priors_refusal(d.refusal), "no priors: never the prior family or its refusals");
                }
                for (PandaUnbatchedOrder o : orders) {
                    expect(!is_priors_refusal(panda_unbatched(off, o)), "no priors: panda_unbatched");
                    expect(!is_priors_refusal(panda_episodes_refusal(off, PANDA_EPISODES_LITERAL, o)), "no priors: episodes, literal");
                    expect(!is_priors_refusal(panda_episodes_refusal(off, PANDA_EPISODES_RUNTIME, o)), "no priors: episodes, run-time");
                }
                // ---- with priors ----
                at = &on;
                {   // the rollout
                    const PandaDecision d = panda_decision(on, PANDA_SIDE_ROLLOUT), d0 = panda_decision(off, PANDA_SIDE_ROLLOUT);
                    expect(d.variant == PANDA_PRIORS, "rollout: the prior family wins over every other");
                    expect(d.scene_used == 1, "rollout: panda_scene_used 1");
                    expect(d.weighted_used == d0.weighted_used && d.weighted_used == (panda_weighted(on) ? 1 : 0),
                           "rollout: panda_weighted_used by the weights, as without priors");
                    PandaRefusal want = d0.refusal;
                    if (want == PANDA_REFUSAL_NONE && si == 0) want = PANDA_SCENE_OFF_PRIORS;
                    if (want == PANDA_REFUSAL_NONE && wi == 0) want = PANDA_WEIGHTS_OFF_PRIORS;
                    expect(d.refusal == want, "rollout: the refusal");
                    expect(d.refusal == PANDA_REFUSAL_NONE || panda_refusal_is_state(d.refusal), "rollout: every refusal is M3_ERR_STATE");
                    expect((si == 0 || wi == 0) == (d.refusal != PANDA_REFUSAL_NONE), "rollout: refused exactly with a switch forced off");
                    expect(panda_refusal(on, PANDA_SIDE_ROLLOUT) == d.refusal, "rollout: panda_refusal is the decision's");
                }
                {   // the batch
                    const PandaDecision d = panda_decision(on, PANDA_SIDE_BATCH);
                    expect(d.refusal == PANDA_UNBATCHED_PRIORS, "batch: PANDA_UNBATCHED_PRIORS ahead of everything");
                    expect(d.variant != PANDA_PRIORS, "batch: no table form of the prior family");
                }
                // step, views, cost: priors_on is not read
                expect(same(panda_decision(on, PANDA_SIDE_STEP), panda_decision(off, PANDA_SIDE_STEP)), "step ignores priors_on");
                expect(same(panda_decision(on, PANDA_SIDE_VIEWS), panda_decision(off, PANDA_SIDE_VIEWS)), "views ignore priors_on");
                expect(same(panda_decision(on, PANDA_SIDE_COST), panda_decision(off, PANDA_SIDE_COST)), "cost ignores priors_on");
                for (PandaUnbatchedOrder o : orders) {
                    expect(panda_unbatched(on, o) == PANDA_UNBATCHED_PRIORS, "panda_unbatched: PANDA_UNBATCHED_PRIORS");
                    expect(panda_episodes_refusal(on, PANDA_EPISODES_LITERAL, o) == PANDA_UNBATCHED_PRIORS, "episodes, literal: PANDA_UNBATCHED_PRIORS");
                    // (run-time set: a planner is asked on the batch side; the world -- sim_only, which cannot have priors -- on the
                    // step side, which does not read priors_on)
                    const PandaRefusal r = panda_episodes_refusal(on, PANDA_EPISODES_RUNTIME, o);
                    if (on.sim_only) expect(r == panda_episodes_refusal(off, PANDA_EPISODES_RUNTIME, o), "episodes, run-time: the world");
                    else expect(r == PANDA_UNBATCHED_PRIORS, "episodes, run-time: a planner: PANDA_UNBATCHED_PRIORS");
                }
            }
    std::printf("%ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
