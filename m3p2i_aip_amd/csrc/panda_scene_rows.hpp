// panda_scene_rows.hpp -- one workspace PER ENVIRONMENT of a sim_only panda_env handle (m3_set_panda_scene_rows) or PER SAMPLE
// of a planner handle's fused rollout (m3_set_panda_rollout_scenes; extension): the device table of the
// rows and how a lane overwrites the workspace words of its PandaSceneRT from its row.  Shared by m3_api.hip (the host packs),
// rollout_panda_rows.hip (the kernels load) and the host build in tests/native/panda_scene_rows_host.cpp (both).
//
// A row of the table is a PandaSceneRT formed ON THE HOST by make_panda_scene_rt (panda_scene.hpp: the derived constants in the
// oracle's order) -- nothing is derived on the device.  Only the 22 words that depend on the workspace are in the table; what
// depends on dt / substeps / iters alone (h, inv_h, the counts, a, rden, dv, invI, pmax, hD, the sleep thresholds) stays in the
// kernel-argument copy of the handle's pscene_rt, so the trip counts of the substep and solver loops are wave-uniform.
// Layout: word-major, [PANDA_SCENE_ROW_WORDS][K_local] like the SoA world -- lane i reads word w at tab[w * K_local + i]: the
// lanes of a wavefront read consecutive addresses, the lanes of one sample (8 or 16 of them in the many-lane forms) one address.
#pragma once
#include "panda_dyn.hpp"

namespace m3 {

constexpr int PANDA_SCENE_ROW_WORDS = 22;

// X(member, count) for every per-workspace member of PandaSceneRT, in table order (count 1: a scalar member)
#define M3_PANDA_SCENE_ROW_ARRAYS(X) X(base, 3) X(table, 6) X(shelf, 6) X(obs_half, 3)
#define M3_PANDA_SCENE_ROW_SCALARS(X) X(mu) X(invm_cube) X(invI_cube) X(invm_obs)

#define M3_COUNT_ARRAY(name, n) +n
#define M3_COUNT_SCALAR(name) +1
static_assert(0 M3_PANDA_SCENE_ROW_ARRAYS(M3_COUNT_ARRAY) M3_PANDA_SCENE_ROW_SCALARS(M3_COUNT_SCALAR) == PANDA_SCENE_ROW_WORDS,
              "the table's words");
// every member of PandaSceneRT is either in the table or one of the 52 uniform ones (substeps and iters among them)
static_assert(sizeof(PandaSceneRT) == (PANDA_SCENE_ROW_WORDS + 52) * sizeof(float), "PandaSceneRT grew: table or uniform?");
#undef M3_COUNT_ARRAY
#undef M3_COUNT_SCALAR

// host: row i of the table from the row's scene (make_panda_scene_rt with the handle's dt / substeps)
inline void panda_scene_row_pack(const PandaSceneRT& s, float* table, int Kl, int i) {
    float* p = table + i;
    int w = 0;
#define M3_PACK_ARRAY(name, n) for (int j = 0; j < n; ++j) p[(size_t)(w++) * Kl] = s.name[j];
#define M3_PACK_SCALAR(name) p[(size_t)(w++) * Kl] = s.name;
    M3_PANDA_SCENE_ROW_ARRAYS(M3_PACK_ARRAY)
    M3_PANDA_SCENE_ROW_SCALARS(M3_PACK_SCALAR)
#undef M3_PACK_ARRAY
#undef M3_PACK_SCALAR
}

// device (and the host build): the workspace words of `s` from row i; the uniform members of `s` stay
__host__ __device__ __forceinline__ void panda_scene_row_load(PandaSceneRT& s, const float* table, int Kl, int i) {
    const float* p = table + i;
    int w = 0;
#define M3_LOAD_ARRAY(name, n)                                                                                             \
    _Pragma("unroll") for (int j = 0; j < n; ++j) s.name[j] = p[(size_t)(w++) * Kl];
#define M3_LOAD_SCALAR(name) s.name = p[(size_t)(w++) * Kl];
    M3_PANDA_SCENE_ROW_ARRAYS(M3_LOAD_ARRAY)
    M3_PANDA_SCENE_ROW_SCALARS(M3_LOAD_SCALAR)
#undef M3_LOAD_ARRAY
#undef M3_LOAD_SCALAR
}
// the scene of row i as a value: the uniform members from `uni`, the rest from the table
__host__ __device__ __forceinline__ PandaSceneRT panda_scene_row_scene(const PandaSceneRT& uni, const float* table, int Kl, int i) {
    PandaSceneRT s = uni;
    panda_scene_row_load(s, table, Kl, i);
    return s;
}

}  // namespace m3
