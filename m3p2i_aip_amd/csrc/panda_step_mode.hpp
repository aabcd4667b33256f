// panda_step_mode.hpp -- the bodies the panda_env step-mode kernels share over the scene's type (as point_step_mode.hpp for the
// point_env): the views' two directions, k_psim_pull / k_psim_push and their _s, _v twins in rollout_panda.hip,
// rollout_panda_scene.hip, rollout_panda_rows.hip.  A shell is its guard, for the rows family the lane's scene
// (panda_scene_row_scene) and one call.
//
// The step and cost shells (k_psim_step*, k_psim_cost*) and the lockstep episodes' kernels (k_panda_episodes_pre / _post) are NOT
// instances of a body here: as instances their machine code moved (commuted operands, other register allocation, other spill
// counts -- profiles/panda_variant_dispatch/README.md has the table), and this header exists to remove copies, not to change
// kernels.  They stay written out, each next to its launcher; what they have in common with these bodies are the helpers of
// rollout_panda_common.hpp (psoa_load / psoa_store, panda_world_from_sim, panda_push_views).
#pragma once
#include "rollout_panda_common.hpp"

namespace m3 {

// set_dof_state_tensor / set_actor_root_state_tensor of row i: the world from the wrapper's views.  Everything derived (sleep
// flags, warm-started impulses, contact forces) is cleared and the held latch inferred from geometry
template <class SC>
__device__ __forceinline__ void psim_pull_body(const SC& sc, const SimViews& v, float* wd, int Kl, int i) {
    PandaWorld w;
    panda_world_from_sim(v.dof_state + (size_t)i * 18, v.root_state + (size_t)i * v.n_actors * 13,
                         v.box_actor, v.dyn_actor, v.obs_actor, w);  // box_actor = cubeA, dyn_actor = cubeB here
    panda_infer_held(sc, w);
    psoa_store(wd, Kl, i, w);
}

// refresh_*_tensor of row i: the wrapper's views from the world
template <class SC>
__device__ __forceinline__ void psim_push_body(const SC& sc, const SimViews& v, const float* wd, int Kl, int i) {
    PandaWorld w;
    psoa_load(wd, Kl, i, w);
    panda_push_views(sc, v, i, w);
}

}  // namespace m3
