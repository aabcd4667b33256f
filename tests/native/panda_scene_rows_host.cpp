// Host program of the per-row workspaces (m3_set_panda_scene_rows / m3_set_panda_rollout_scenes) for
// tests/test_panda_scene_rows_cpu.py: the product's csrc/panda_scene_rows.hpp, panda_scene.hpp and panda_dyn.hpp compiled by g++,
// one lane per "wavefront".  It packs the workspaces into the word-major table as the setters do (make_panda_scene_rt,
// panda_scene_row_pack), rebuilds each row's PandaSceneRT as the kernels of rollout_panda_rows.hip do (panda_scene_row_load on
// the handle's pscene_rt), checks that against make_panda_scene_rt of the row byte for byte, and loads and steps every world in
// its row's workspace as k_psim_pull_v / k_psim_step_v do -- against the oracle in that workspace, without a GPU.  A program
// with its own main, so that it also runs under -fsanitize=address,undefined as it is.
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -Itests/native/shim panda_scene_rows_host.cpp -o panda_scene_rows_host
//   panda_scene_rows_host IN OUT
// IN  (binary, 4-byte words): int n, steps, n_scenes, substeps; float dt; float scenes[n_scenes][21] (m3_panda_scene);
//     int scene_of_row[n]; float worlds[n][84] (the oracle's rows); float u[steps][n][9]
// OUT: float scenes_rt[n][74] (each row's PandaSceneRT as read back from the table); float worlds[1 + steps][n][84] after the
//     load (grasp and sleep state inferred) and after each step.  Exit status 1 if a row read back differs from
//     make_panda_scene_rt of it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../m3p2i_aip_amd/csrc/panda_scene.hpp"
#include "../../m3p2i_aip_amd/csrc/panda_scene_rows.hpp"

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
template <class T>
bool rd(std::FILE* f, T* p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }
template <class T>
bool wr(std::FILE* f, const T* p, size_t n) { return n == 0 || std::fwrite(p, sizeof(T), n, f) == n; }
constexpr int RT_WORDS = (int)(sizeof(m3::PandaSceneRT) / sizeof(float));
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    int head[4];
    float dt;
    if (!rd(in, head, 4) || !rd(in, &dt, 1)) { std::fprintf(stderr, "short header\n"); return 2; }
    const int n = head[0], steps = head[1], n_scenes = head[2], substeps = head[3];
    if (n <= 0 || n > 1 << 20 || steps < 0 || steps > 1 << 10 || n_scenes <= 0 || n_scenes > 1 << 10 || substeps <= 0) {
        std::fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<m3_panda_scene> scenes(n_scenes);
    std::vector<int> scene_of(n);
    std::vector<float> worlds((size_t)n * 84), u((size_t)steps * n * 9);
    if (!rd(in, scenes.data(), scenes.size()) || !rd(in, scene_of.data(), scene_of.size()) || !rd(in, worlds.data(), worlds.size()) ||
        !rd(in, u.data(), u.size())) {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    std::fclose(in);
    for (int i = 0; i < n; ++i)
        if (scene_of[i] < 0 || scene_of[i] >= n_scenes) { std::fprintf(stderr, "row %d: no such scene\n", i); return 2; }
    for (int k = 0; k < n_scenes; ++k) {
        const std::string fault = m3::panda_scene_fault(scenes[k]);
        if (!fault.empty()) { std::fprintf(stderr, "scene %d: %s\n", k, fault.c_str()); return 2; }
    }

    // the table as the setters upload it: [PANDA_SCENE_ROW_WORDS][n]
    std::vector<float> table((size_t)m3::PANDA_SCENE_ROW_WORDS * n);
    for (int i = 0; i < n; ++i)
        m3::panda_scene_row_pack(m3::make_panda_scene_rt(scenes[scene_of[i]], dt, substeps), table.data(), n, i);
    // the handle's own pscene_rt, of which the kernels read the uniform members only: a workspace that is none of the rows'
    // (every field of the default times 1.37), so a workspace word that did not come from the table would show
    m3_panda_scene other = m3::PANDA_SCENE_DEFAULT;
    float of[m3::PANDA_SCENE_FLOATS];
    std::memcpy(of, &other, sizeof(of));
    for (int k = 0; k < m3::PANDA_SCENE_FLOATS; ++k) of[k] *= 1.37f;
    std::memcpy(&other, of, sizeof(of));
    const m3::PandaSceneRT uni = m3::make_panda_scene_rt(other, dt, substeps);

    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    int bad_rows = 0;
    for (int i = 0; i < n; ++i) {
        const m3::PandaSceneRT got = m3::panda_scene_row_scene(uni, table.data(), n, i);
        const m3::PandaSceneRT want = m3::make_panda_scene_rt(scenes[scene_of[i]], dt, substeps);
        if (std::memcmp(&got, &want, sizeof(got)) != 0) {
            if (!bad_rows) std::fprintf(stderr, "row %d: the scene read back from the table is not make_panda_scene_rt of the row\n", i);
            ++bad_rows;
        }
        float words[RT_WORDS];
        std::memcpy(words, &got, sizeof(got));
        if (!wr(out, words, (size_t)RT_WORDS)) { std::perror("write"); return 2; }
    }

    std::vector<float> corner(m3::PANDA_STORE_FLOATS);
    const m3::CornerStore cs{corner.data(), 1};
    for (int i = 0; i < n; ++i) {   // one lane of k_psim_pull_v
        const m3::PandaSceneRT sc = m3::panda_scene_row_scene(uni, table.data(), n, i);
        m3::PandaWorld p;
        load(worlds.data() + 84 * (size_t)i, p);
        float hp[3];
        m3::panda_infer_held(sc, p, hp);
        store(p, worlds.data() + 84 * (size_t)i);
    }
    if (!wr(out, worlds.data(), worlds.size())) { std::perror("write"); return 2; }
    for (int t = 0; t < steps; ++t) {
        for (int i = 0; i < n; ++i) {   // one lane of k_psim_step_v
            const m3::PandaSceneRT sc = m3::panda_scene_row_scene(uni, table.data(), n, i);
            m3::PandaWorld p;
            load(worlds.data() + 84 * (size_t)i, p);
            m3::PandaObs o;
            m3::panda_step(sc, p, u.data() + ((size_t)t * n + i) * 9, o, cs);
            store(p, worlds.data() + 84 * (size_t)i);
        }
        if (!wr(out, worlds.data(), worlds.size())) { std::perror("write"); return 2; }
    }
    if (std::fclose(out) != 0) { std::perror("close"); return 2; }
    if (bad_rows) { std::fprintf(stderr, "%d of %d rows differ\n", bad_rows, n); return 1; }
    std::printf("panda_scene_rows_host: ok (%d rows, %d steps)\n", n, steps);
    return 0;
}
