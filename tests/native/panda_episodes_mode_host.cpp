// Host program of the lockstep panda episodes' decision for tests/test_panda_episodes_runtime_cpu.py: the product's
// csrc/panda_variant.hpp compiled by g++ (it has no HIP dependency).  It walks every input tests/native/panda_variant_host.cpp
// walks -- 3 x 3 settings of the two instance switches x 2^5 flags -- and checks panda_episodes_refusal in both modes:
//   literal (m3_panda_episodes_create, flags == 0): panda_unbatched's answer, for both orders;
//   run-time (M3_PANDA_EPISODES_RUNTIME): only the forced-off refusals remain -- written out below as the issue states them, not
//   through panda_refusal -- with their M3_ERR_STATE enumerators, whatever the order; no PANDA_UNBATCHED_* is ever returned.
// A program with its own main, so that it also runs under -fsanitize=address,undefined as it is.
//   g++ -O2 -std=c++17 panda_episodes_mode_host.cpp -o panda_episodes_mode_host && ./panda_episodes_mode_host
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
                             "rollout_scenes_on %d scene_rows_on %d sim_only %d\n",
                     what, at->scene_instance, at->weighted_instance, at->geometry_default, at->weights_default,
                     at->rollout_scenes_on, at->scene_rows_on, at->sim_only);
}

// what a run-time set still refuses: a switch forced off against what the handle holds.  The scene switch first (rows per
// environment, rows per sample, the geometry), then -- for a planner, whose command forms a cost -- the weights' switch
PandaRefusal ref_runtime(const PandaVariantInput& in) {
    if (in.scene_instance == 0) {
        if (in.scene_rows_on) return PANDA_SCENE_OFF_ENV_ROWS;
        if (in.rollout_scenes_on) return PANDA_SCENE_OFF_SAMPLE_ROWS;
        if (!in.geometry_default) return PANDA_SCENE_OFF_GEOMETRY;
    }
    if (!in.sim_only && in.weighted_instance == 0 && !in.weights_default) return PANDA_WEIGHTS_OFF_TUNED;
    return PANDA_REFUSAL_NONE;
}
bool is_unbatched(PandaRefusal r) {
    return r == PANDA_UNBATCHED_SCENE || r == PANDA_UNBATCHED_SAMPLE_ROWS || r == PANDA_UNBATCHED_ENV_ROWS || r == PANDA_UNBATCHED_WEIGHTS;
}
}  // namespace

int main() {
    expect(panda_episodes_variant(PANDA_EPISODES_LITERAL) == PANDA_LITERAL, "the literal mode launches the literal kernels");
    expect(panda_episodes_variant(PANDA_EPISODES_RUNTIME) == PANDA_ROWS, "the run-time mode launches the rows kernels");
    const PandaUnbatchedOrder orders[] = {PANDA_ROWS_THEN_WEIGHTS, PANDA_WEIGHTS_THEN_ROWS};
    int inputs = 0, runtime_refused = 0, literal_refused = 0;
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
                ++inputs;
                for (PandaUnbatchedOrder order : orders) {
                    const PandaRefusal lit = panda_episodes_refusal(in, PANDA_EPISODES_LITERAL, order);
                    expect(lit == panda_unbatched(in, order), "literal mode: panda_unbatched's answer");
                    expect(lit == PANDA_REFUSAL_NONE || is_unbatched(lit), "literal mode: an M3_ERR_UNSUPPORTED enumerator or none");
                    expect(!panda_refusal_is_state(lit), "literal mode: never M3_ERR_STATE");
                    const PandaRefusal rt = panda_episodes_refusal(in, PANDA_EPISODES_RUNTIME, order);
                    expect(rt == ref_runtime(in), "run-time mode: only the forced-off refusals remain");
                    expect(!is_unbatched(rt), "run-time mode: nothing is unbatched");
                    expect(panda_refusal_is_state(rt) == (rt != PANDA_REFUSAL_NONE), "run-time mode: a refusal is M3_ERR_STATE");
                    literal_refused += lit != PANDA_REFUSAL_NONE;
                    runtime_refused += rt != PANDA_REFUSAL_NONE;
                }
                // with both switches left alone a run-time set takes every handle
                if (si < 0 && wi < 0) expect(panda_episodes_refusal(in, PANDA_EPISODES_RUNTIME, PANDA_ROWS_THEN_WEIGHTS) == PANDA_REFUSAL_NONE,
                                             "run-time mode: automatic switches refuse nothing");
            }
    // (the walk is not vacuous: both modes refuse somewhere, the run-time mode less often)
    expect(inputs == 288 && runtime_refused > 0 && literal_refused > runtime_refused, "the walk covers refusals of both modes");
    std::printf("%ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
