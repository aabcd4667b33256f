// Host build of the product's csrc/panda_dyn.hpp THROUGH THE RUN-TIME SCENE (PandaSceneRT, csrc/panda_scene.hpp:
// make_panda_scene_rt) for the CPU tests (tests/test_panda_scene_cpu.py): the device code of the panda_env world with the
// workspace of m3_set_panda_scene, lane by lane, against the oracle in the same workspace -- without a GPU.
//   g++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off -Itests/native/shim panda_scene_host.cpp -o libpanda_scene_host.so
#include "../../m3p2i_aip_amd/csrc/panda_scene.hpp"

#include <cstring>
#include <vector>

namespace {
// oracle row (84 floats, m3o_panda_world): q9 qd9 | cubeA13 cubeB13 obs13 (pos3 quat4 vel3 angvel3) | held | rel_p3 rel_q4 |
// awake2 | f_table3 f_shelf3 f_cubeB3 | warm_t4 warm_l4
void load_body(const float* b, m3::Body& o) {
    for (int i = 0; i < 3; ++i) { o.p[i] = b[i]; o.v[i] = b[7 + i]; o.w[i] = b[10 + i]; }
    for (int i = 0; i < 4; ++i) o.q[i] = b[3 + i];
}
void store_body(const m3::Body& o, float* b) {
    for (int i = 0; i < 3; ++i) { b[i] = o.p[i]; b[7 + i] = o.v[i]; b[10 + i] = o.w[i]; }
    for (int i = 0; i < 4; ++i) b[3 + i] = o.q[i];
}
void load(const float* w, m3::PandaWorld& p) {
    for (int i = 0; i < 9; ++i) { p.q[i] = w[i]; p.qd[i] = w[9 + i]; }
    load_body(w + 18, p.A);
    load_body(w + 31, p.B);
    for (int i = 0; i < 3; ++i) { p.obs_p[i] = w[44 + i]; p.obs_v[i] = w[51 + i]; p.rel_p[i] = w[58 + i]; }
    for (int i = 0; i < 4; ++i) { p.rel_q[i] = w[61 + i]; p.warm_t[i] = w[76 + i]; p.warm_l[i] = w[80 + i]; }
    p.held = w[57];
    p.awake[0] = w[65]; p.awake[1] = w[66];
    for (int i = 0; i < 3; ++i) { p.f_table[i] = w[67 + i]; p.f_shelf[i] = w[70 + i]; p.f_cubeB[i] = w[73 + i]; }
}
void store(const m3::PandaWorld& p, float* w) {
    for (int i = 0; i < 9; ++i) { w[i] = p.q[i]; w[9 + i] = p.qd[i]; }
    store_body(p.A, w + 18);
    store_body(p.B, w + 31);
    for (int i = 0; i < 3; ++i) { w[44 + i] = p.obs_p[i]; w[51 + i] = p.obs_v[i]; w[58 + i] = p.rel_p[i]; }
    for (int i = 0; i < 4; ++i) { w[61 + i] = p.rel_q[i]; w[76 + i] = p.warm_t[i]; w[80 + i] = p.warm_l[i]; }
    w[57] = p.held;
    w[65] = p.awake[0]; w[66] = p.awake[1];
    for (int i = 0; i < 3; ++i) { w[67 + i] = p.f_table[i]; w[70 + i] = p.f_shelf[i]; w[73 + i] = p.f_cubeB[i]; }
}
// the kinematics a rollout carries from one substep to the next (panda_dyn.hpp: FkCarry), per world, from the load on
std::vector<m3::FkCarry<1>> g_fk;

template <class SC>
void step_all(const SC& sc, float* worlds, int n, const float* u, float* obs, int mode, float* hp, float* trav) {
    float corner[m3::PANDA_STORE_FLOATS];
    const m3::CornerStore cs{corner, 1};
    for (int i = 0; i < n; ++i) {
        m3::PandaWorld p;
        load(worlds + 84 * (long long)i, p);
        m3::PandaObs o;
        m3::FkCarry<1> local;
        local.valid = false;
        m3::FkCarry<1>* fk = ((int)g_fk.size() == n) ? &g_fk[i] : &local;
        if (mode == 0) m3::panda_step<true, false>(sc, p, u + 9 * i, o, cs);
        else if (mode == 1) m3::panda_step<true, true>(sc, p, u + 9 * i, o, cs, hp + 3 * i, trav + i, fk);
        else m3::panda_step<false, true>(sc, p, u + 9 * i, o, cs, hp + 3 * i, trav + i, fk);
        store(p, worlds + 84 * (long long)i);
        for (int j = 0; j < 3; ++j) { obs[10 * i + j] = o.left[j]; obs[10 * i + 7 + j] = o.right[j]; }
        for (int j = 0; j < 4; ++j) obs[10 * i + 3 + j] = o.left_q[j];
    }
}
template <class SC>
void infer_all(const SC& sc, float* worlds, int n, float* hp) {
    g_fk.assign(n, m3::FkCarry<1>());
    for (int i = 0; i < n; ++i) {
        g_fk[i].valid = false;
        m3::PandaWorld p;
        load(worlds + 84 * (long long)i, p);
        m3::panda_infer_held(sc, p, hp + 3 * i);
        store(p, worlds + 84 * (long long)i);
    }
}
m3_panda_scene scene_of(const float* f21) {
    m3_panda_scene s;
    std::memcpy(&s, f21, sizeof(s));
    return s;
}
}  // namespace

// n worlds, one step each with controls u[n][9]; obs[n][10] = left pos3, left quat4, right pos3.  mode 0: panda_step<FORCES,
// !LAZY> (step mode); 1: <FORCES, LAZY> (the pick rollout); 2: <!FORCES, LAZY> (reach / place rollouts).  scene21: the 21
// floats of m3_panda_scene -> PandaSceneRT; null: the compile-time PandaScene.
extern "C" void pss_step(const float* scene21, float dt, int substeps, float* worlds, int n, const float* u, float* obs, int mode,
                         float* hp, float* trav) {
    if (scene21) step_all(m3::make_panda_scene_rt(scene_of(scene21), dt, substeps), worlds, n, u, obs, mode, hp, trav);
    else {
        m3::PandaScene sc;
        m3::make_panda_scene(sc, dt, substeps);
        step_all(sc, worlds, n, u, obs, mode, hp, trav);
    }
}
// world load: the grasp / sleep state inferred from the geometry + the hand origin for the lazy kinematics
extern "C" void pss_infer_held(const float* scene21, float dt, int substeps, float* worlds, int n, float* hp) {
    if (scene21) infer_all(m3::make_panda_scene_rt(scene_of(scene21), dt, substeps), worlds, n, hp);
    else {
        m3::PandaScene sc;
        m3::make_panda_scene(sc, dt, substeps);
        infer_all(sc, worlds, n, hp);
    }
}
// the 11 link poses (pos3 quat4 each) of joint values q[9] in the scene's base
extern "C" void pss_fk(const float* scene21, const float* q, float* links77) {
    const m3::PandaSceneRT sc = m3::make_panda_scene_rt(scene_of(scene21), 0.01f, 2);
    m3::Frame hand;
    float pl[3], pr[3];
    m3::panda_fk<true>(sc, q, hand, pl, pr, links77);
}
extern "C" void pss_default_scene(float* out21) { std::memcpy(out21, &m3::PANDA_SCENE_DEFAULT, sizeof(m3_panda_scene)); }
