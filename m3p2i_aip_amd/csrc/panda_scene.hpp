// panda_scene.hpp -- the panda_env workspace as run-time state (m3_set_panda_scene, include/m3p2i_hip.h): the defaults, the
// per-field checks and the host-side construction of the kernels' scenes.  Host code only; f32, in the oracle's order.
#pragma once
#include "../../include/m3p2i_hip.h"
#include "panda_dyn.hpp"

#include <cmath>
#include <cstring>
#include <string>

namespace m3 {

// the reference's workspace: PandaScene's constants (panda.yaml, 1_table.yaml, 3_shelf_stand.yaml, 4_obs.yaml,
// 5_cubeA.yaml / 6_cubeB.yaml, actor_utils.py:27)
constexpr m3_panda_scene PANDA_SCENE_DEFAULT = {
    {-0.45f, 0.0f, 1.125f},
    {0.0f, 0.0f, 1.0f, 0.6f, 0.6f, 0.025f},
    {0.5f, 0.0f, 1.175f, 0.1f, 0.1f, 0.15f},
    {0.1f, 0.1f, 0.01f},
    0.8f, 0.125f, 1.0f};
constexpr int PANDA_SCENE_FLOATS = 21;
static_assert(sizeof(m3_panda_scene) == PANDA_SCENE_FLOATS * sizeof(float), "m3_panda_scene: twenty-one floats");

// what field i is called in a message, and what it must satisfy: 0 any finite value (a position), 1 > 0 (a half extent,
// a mass), 2 >= 0 (friction)
inline std::string panda_scene_field_name(int i) {
    auto idx = [](const char* n, int j) { return std::string(n) + "[" + std::to_string(j) + "]"; };
    if (i < 3) return idx("base", i);
    if (i < 9) return idx("table", i - 3);
    if (i < 15) return idx("shelf", i - 9);
    if (i < 18) return idx("obs_half", i - 15);
    return i == 18 ? "obs_m" : i == 19 ? "cube_m" : "mu";
}
inline int panda_scene_field_rule(int i) {
    if (i < 3) return 0;
    if (i < 15) return ((i - 3) % 6 < 3) ? 0 : 1;
    if (i < 20) return 1;
    return 2;
}
// empty if the scene passes, else "<field> <what is wrong>"
inline std::string panda_scene_fault(const m3_panda_scene& src) {
    float f[PANDA_SCENE_FLOATS];
    std::memcpy(f, &src, sizeof(f));
    for (int i = 0; i < PANDA_SCENE_FLOATS; ++i) {
        const int rule = panda_scene_field_rule(i);
        const char* what = !std::isfinite(f[i]) ? " is not finite"
                           : (rule == 1 && !(f[i] > 0.0f)) ? " must be > 0"
                           : (rule == 2 && f[i] < 0.0f) ? " must be >= 0" : nullptr;
        if (what) return panda_scene_field_name(i) + what;
    }
    return std::string();
}
// the 21 floats are the defaults bit for bit (-0.0f is not 0.0f here)
inline bool panda_scene_is_default(const m3_panda_scene& p) { return std::memcmp(&p, &PANDA_SCENE_DEFAULT, sizeof(p)) == 0; }
// ... but for the two masses, which reach the kernels through PandaScene's run-time part: such a scene runs on PandaScene
inline bool panda_scene_geometry_is_default(const m3_panda_scene& p) {
    m3_panda_scene q = p;
    q.obs_m = PANDA_SCENE_DEFAULT.obs_m; q.cube_m = PANDA_SCENE_DEFAULT.cube_m;
    return panda_scene_is_default(q);
}

inline PandaSceneRT make_panda_scene_rt(const m3_panda_scene& p, float dt, int substeps, int iters = 6) {
    PandaSceneRT s;
    make_panda_scene(s, dt, substeps, iters, p.cube_m, p.obs_m);
    for (int i = 0; i < 3; ++i) { s.base[i] = p.base[i]; s.obs_half[i] = p.obs_half[i]; }
    for (int i = 0; i < 6; ++i) { s.table[i] = p.table[i]; s.shelf[i] = p.shelf[i]; }
    s.mu = p.mu;
    return s;
}

}  // namespace m3
