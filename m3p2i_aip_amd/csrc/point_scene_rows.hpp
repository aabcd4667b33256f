// point_scene_rows.hpp -- one arena PER ENVIRONMENT of a sim_only point_env handle (m3_set_point_scene_rows; extension): the
// device table of the rows and how a lane turns its row back into a PointSceneRT.  Shared by m3_api.hip (the host packs),
// rollout_point_scene_rows.hip (the kernels load) and the host build in tests/native/point_scene_rows_host.cpp (both).
//
// A row of the table is a PointSceneRT formed ON THE HOST by make_point_scene_rt (planar_dyn.hpp: the derived constants in the
// oracle's order) -- nothing is derived on the device.  Only the words that depend on the arena are in the table; what depends
// on dt / substeps / solver_iters alone (h, inv_h, substeps, iters, gam, dmax) and the five solver constants stay in the
// kernel-argument copy of the handle's scene_rt, so the trip counts of the substep and solver loops are wave-uniform.
// Layout: word-major, [POINT_SCENE_ROW_WORDS][K_local] like the SoA world -- the 64 lanes of a wavefront read consecutive
// addresses.
#pragma once
#include "planar_dyn.hpp"

namespace m3 {

constexpr int POINT_SCENE_ROW_WORDS = 38;

// X(member) for every per-arena member of PointSceneRT, in table order
#define M3_POINT_SCENE_ROW_FIELDS(X)                                                                                       \
    X(md) X(LlinB) X(LangB) X(LlinD) X(LangD) X(RcB) X(RcD)                                                                 \
    X(robot_r) X(invm_r)                                                                                                    \
    X(box_hx) X(box_hy) X(box_m) X(box_I) X(invm_b) X(invI_b)                                                               \
    X(dyn_hx) X(dyn_hy) X(dyn_m) X(dyn_I) X(invm_d) X(invI_d)                                                               \
    X(obs_x) X(obs_y) X(obs_hx) X(obs_hy)                                                                                   \
    X(wall)                                                                                                                 \
    X(mu_rb) X(mu_rd) X(mu_ro) X(mu_rw) X(mu_bw) X(mu_dw) X(mu_bd) X(mu_bo) X(mu_do)                                        \
    X(rad_b) X(rad_d) X(rad_o)

#define M3_COUNT_FIELD(name) +1
static_assert(0 M3_POINT_SCENE_ROW_FIELDS(M3_COUNT_FIELD) == POINT_SCENE_ROW_WORDS, "the table's words");
// every member of PointSceneRT is either in the table or one of the 11 uniform ones (substeps and iters among them)
static_assert(sizeof(PointSceneRT) == (POINT_SCENE_ROW_WORDS + 11) * sizeof(float), "PointSceneRT grew: table or uniform?");
#undef M3_COUNT_FIELD

// host: row i of the table from the row's scene (make_point_scene_rt with the handle's dt / substeps / solver_iters)
inline void point_scene_row_pack(const PointSceneRT& s, float* table, int Kl, int i) {
    float* p = table + i;
    int w = 0;
#define M3_PACK_FIELD(name) p[(size_t)(w++) * Kl] = s.name;
    M3_POINT_SCENE_ROW_FIELDS(M3_PACK_FIELD)
#undef M3_PACK_FIELD
}

// device (and the host build): the scene of environment i -- the uniform members from `uni`, the rest from row i
__host__ __device__ __forceinline__ PointSceneRT point_scene_row_load(const PointSceneRT& uni, const float* table, int Kl, int i) {
    PointSceneRT s = uni;
    const float* p = table + i;
    int w = 0;
#define M3_LOAD_FIELD(name) s.name = p[(size_t)(w++) * Kl];
    M3_POINT_SCENE_ROW_FIELDS(M3_LOAD_FIELD)
#undef M3_LOAD_FIELD
    return s;
}

}  // namespace m3
