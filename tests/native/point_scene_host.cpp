// Host build of the product's csrc/planar_dyn.hpp through the RUN-TIME scene type PointSceneRT (m3_set_point_scene) for the
// CPU tests (tests/test_point_scene_cpu.py): the device code of the point_env dynamics with the arena as run-time values, lane
// by lane, against the oracle with the same scene -- without a GPU.
//   g++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off -Itests/native/shim point_scene_host.cpp -o libpoint_scene_host.so
#include "../../m3p2i_aip_amd/csrc/planar_dyn.hpp"

namespace {
void load(const float* w, m3::PointWorld& p) {   // oracle row (31 floats): 3 bodies x (x y c s vx vy w) | fext R, B | fc R, B, D
    p.rx = w[0]; p.ry = w[1]; p.rvx = w[4]; p.rvy = w[5];
    p.B = {w[7], w[8], w[9], w[10], w[11], w[12], w[13]};
    p.D = {w[14], w[15], w[16], w[17], w[18], w[19], w[20]};
    p.fRx = w[21]; p.fRy = w[22]; p.fBx = w[23]; p.fBy = w[24];
    p.fcRx = w[25]; p.fcRy = w[26]; p.fcBx = w[27]; p.fcBy = w[28]; p.fcDx = w[29]; p.fcDy = w[30];
}
void store(const m3::PointWorld& p, float* w, bool all_forces) {
    w[0] = p.rx; w[1] = p.ry; w[4] = p.rvx; w[5] = p.rvy;
    const m3::Box* b[2] = {&p.B, &p.D};
    for (int i = 0; i < 2; ++i) {
        float* o = w + 7 + 7 * i;
        o[0] = b[i]->x; o[1] = b[i]->y; o[2] = b[i]->c; o[3] = b[i]->s; o[4] = b[i]->vx; o[5] = b[i]->vy; o[6] = b[i]->w;
    }
    w[21] = p.fRx; w[22] = p.fRy; w[23] = p.fBx; w[24] = p.fBy;
    w[29] = p.fcDx; w[30] = p.fcDy;
    if (all_forces) { w[25] = p.fcRx; w[26] = p.fcRy; w[27] = p.fcBx; w[28] = p.fcBy; }
}
template <class SC>
void run(const SC& sc, float* worlds, int n, const float* u, int mode) {
    for (int i = 0; i < n; ++i) {
        m3::PointWorld p;
        load(worlds + 31 * (long long)i, p);
        if (mode == 0) m3::point_step<true>(sc, p, u[2 * i], u[2 * i + 1]);
        else m3::point_step<false>(sc, p, u[2 * i], u[2 * i + 1], true);
        store(p, worlds + 31 * (long long)i, mode == 0);
    }
}
}  // namespace

// n worlds (rows of 31 floats, the oracle's layout), one step each with controls u[n][2], in the arena `scene` (28 floats,
// m3_point_scene).  mode 0: point_step<true> (step mode), mode 1: point_step<false> (the rollout's instance dispatch).
extern "C" void psh_step_rt(const float* scene, float dt, int substeps, int iters, float* worlds, int n, const float* u, int mode) {
    m3_point_scene p;
    __builtin_memcpy(&p, scene, sizeof(p));
    run(m3::make_point_scene_rt(p, dt, substeps, iters), worlds, n, u, mode);
}
// the same through the compile-time scene type (the default arena)
extern "C" void psh_step_ct(float dt, int substeps, int iters, float* worlds, int n, const float* u, int mode) {
    m3::PointScene sc;
    m3::make_point_scene(sc, dt, substeps, iters);
    run(sc, worlds, n, u, mode);
}
extern "C" void psh_default_scene(float* out) { __builtin_memcpy(out, &m3::POINT_SCENE_DEFAULT, sizeof(m3_point_scene)); }
extern "C" int psh_scene_floats() { return (int)(sizeof(m3_point_scene) / sizeof(float)); }
extern "C" float psh_bounding_radius(float hx, float hy) { return m3::point_bounding_radius(hx, hy); }
// the broad-phase radii the run-time scene carries: box, dyn-obs, obstacle
extern "C" void psh_radii(const float* scene, float* out) {
    m3_point_scene p;
    __builtin_memcpy(&p, scene, sizeof(p));
    const m3::PointSceneRT s = m3::make_point_scene_rt(p, 0.05f, 2, 6);
    out[0] = s.rad_b; out[1] = s.rad_d; out[2] = s.rad_o;
}
