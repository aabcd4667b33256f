// Host program of the two workspace tables of a run-time lockstep panda episode set (m3_panda_episodes_create_ex with
// M3_PANDA_EPISODES_RUNTIME) for tests/test_panda_episodes_runtime_cpu.py: the product's csrc/panda_episode_tables.hpp,
// panda_scene_rows.hpp, panda_scene.hpp and panda_dyn.hpp compiled by g++, one lane per "wavefront".  It fills the planning-side
// and the world-side table as m3_api.hip does (panda_episode_table_refresh), rebuilds each row's PandaSceneRT as the kernels of
// rollout_panda_episodes_rt.hip do (panda_scene_row_scene on the world's pscene_rt) and checks it against make_panda_scene_rt
// of the row byte for byte; checks that a refresh packs exactly the rows that changed; then runs the two lane bodies on every
// episode -- the pre kernel's (load the world's row, infer the grasp state, one step under the kept targets) in the episode's
// PLANNING row, the post kernel's (one step per tick under the tick's targets) in its WORLD row -- for the oracle comparison in
// those workspaces, without a GPU.  A program with its own main, so that it also runs under -fsanitize=address,undefined.
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -Itests/native/shim panda_episode_tables_host.cpp -o panda_episode_tables_host
//   panda_episode_tables_host IN OUT
// IN  (binary, 4-byte words): int n, steps, n_scenes, substeps; float dt; float scenes[n_scenes][21] (m3_panda_scene);
//     int plan_of[n]; int world_of[n]; float worlds[n][84] (the oracle's rows); float kept[n][9]; float u[steps][n][9]
// OUT: float plan_rt[n][74], world_rt[n][74] (each row's PandaSceneRT as read back from its table); float pre[n][84] (the pre
//     lane's world after its step); float post[steps][n][84] (the post lane's world after each tick's step, from `worlds`).
//     Exit status 1 if a row read back differs from make_panda_scene_rt of it or a refresh packed other rows than the changed.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../m3p2i_aip_amd/csrc/panda_episode_tables.hpp"

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
    std::vector<int> of[2] = {std::vector<int>(n), std::vector<int>(n)};   // 0 the planning side, 1 the world side
    std::vector<float> worlds((size_t)n * 84), kept_u((size_t)n * 9), u((size_t)steps * n * 9);
    if (!rd(in, scenes.data(), scenes.size()) || !rd(in, of[0].data(), of[0].size()) || !rd(in, of[1].data(), of[1].size()) ||
        !rd(in, worlds.data(), worlds.size()) || !rd(in, kept_u.data(), kept_u.size()) || !rd(in, u.data(), u.size())) {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    std::fclose(in);
    for (int side = 0; side < 2; ++side)
        for (int i = 0; i < n; ++i)
            if (of[side][i] < 0 || of[side][i] >= n_scenes) { std::fprintf(stderr, "row %d: no such scene\n", i); return 2; }
    for (int k = 0; k < n_scenes; ++k) {
        const std::string fault = m3::panda_scene_fault(scenes[k]);
        if (!fault.empty()) { std::fprintf(stderr, "scene %d: %s\n", k, fault.c_str()); return 2; }
    }

    // the two tables as create fills them: [PANDA_SCENE_ROW_WORDS][n] each, every row packed
    std::vector<float> table[2];
    std::vector<m3_panda_scene> kept[2];
    int bad = 0;
    for (int side = 0; side < 2; ++side) {
        table[side].assign((size_t)m3::PANDA_SCENE_ROW_WORDS * n, -7.0f);
        kept[side].assign(n, m3::PANDA_SCENE_DEFAULT);
        const int packed = m3::panda_episode_table_refresh(table[side].data(), kept[side].data(), true, n, dt, substeps,
                                                           [&](int e) -> const m3_panda_scene& { return scenes[of[side][e]]; });
        if (packed != n) { std::fprintf(stderr, "side %d: the first fill packed %d of %d rows\n", side, packed, n); ++bad; }
        // nothing changed: nothing packed, the table stays
        const std::vector<float> before = table[side];
        const int again = m3::panda_episode_table_refresh(table[side].data(), kept[side].data(), false, n, dt, substeps,
                                                          [&](int e) -> const m3_panda_scene& { return scenes[of[side][e]]; });
        if (again != 0 || before != table[side]) { std::fprintf(stderr, "side %d: an unchanged refresh packed %d rows\n", side, again); ++bad; }
    }
    // the world's own pscene_rt, of which the kernels read the uniform members only: a workspace that is none of the rows'
    // (every field of the default times 1.37), so a workspace word that did not come from the table would show
    m3_panda_scene other = m3::PANDA_SCENE_DEFAULT;
    float ofl[m3::PANDA_SCENE_FLOATS];
    std::memcpy(ofl, &other, sizeof(ofl));
    for (int k = 0; k < m3::PANDA_SCENE_FLOATS; ++k) ofl[k] *= 1.37f;
    std::memcpy(&other, ofl, sizeof(ofl));
    const m3::PandaSceneRT uni = m3::make_panda_scene_rt(other, dt, substeps);

    {   // one row changes (the last: to `other`, then back): exactly that row is packed, no other word of the table moves
        const int e1 = n - 1;
        const std::vector<float> before = table[0];
        int packed = m3::panda_episode_table_refresh(table[0].data(), kept[0].data(), false, n, dt, substeps,
                                                     [&](int e) -> const m3_panda_scene& { return e == e1 ? other : scenes[of[0][e]]; });
        const m3::PandaSceneRT got = m3::panda_scene_row_scene(uni, table[0].data(), n, e1);
        if (packed != 1 || std::memcmp(&got, &uni, sizeof(got)) != 0) { std::fprintf(stderr, "a changed row: packed %d\n", packed); ++bad; }
        for (int w = 0; w < m3::PANDA_SCENE_ROW_WORDS; ++w)
            for (int e = 0; e < n; ++e)
                if (e != e1 && std::memcmp(&table[0][(size_t)w * n + e], &before[(size_t)w * n + e], sizeof(float)) != 0) ++bad;
        packed = m3::panda_episode_table_refresh(table[0].data(), kept[0].data(), false, n, dt, substeps,
                                                 [&](int e) -> const m3_panda_scene& { return scenes[of[0][e]]; });
        if (packed != 1 || before != table[0]) { std::fprintf(stderr, "the row changed back: packed %d\n", packed); ++bad; }
    }

    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    int bad_rows = 0;
    for (int side = 0; side < 2; ++side)
        for (int i = 0; i < n; ++i) {
            const m3::PandaSceneRT got = m3::panda_scene_row_scene(uni, table[side].data(), n, i);
            const m3::PandaSceneRT want = m3::make_panda_scene_rt(scenes[of[side][i]], dt, substeps);
            if (std::memcmp(&got, &want, sizeof(got)) != 0) {
                if (!bad_rows) std::fprintf(stderr, "side %d row %d: the scene read back from the table is not make_panda_scene_rt of the row\n", side, i);
                ++bad_rows;
            }
            float words[RT_WORDS];
            std::memcpy(words, &got, sizeof(got));
            if (!wr(out, words, (size_t)RT_WORDS)) { std::perror("write"); return 2; }
        }

    std::vector<float> corner(m3::PANDA_STORE_FLOATS);
    const m3::CornerStore cs{corner.data(), 1};
    {   // one lane of k_panda_episodes_pre_v per episode: the PLANNING table's row
        std::vector<float> pre = worlds;
        for (int i = 0; i < n; ++i) {
            const m3::PandaSceneRT sc = m3::panda_scene_row_scene(uni, table[0].data(), n, i);
            m3::PandaWorld p;
            load(pre.data() + 84 * (size_t)i, p);
            float hp[3];
            m3::panda_infer_held(sc, p, hp);
            m3::PandaObs o;
            m3::panda_step(sc, p, kept_u.data() + (size_t)i * 9, o, cs);
            store(p, pre.data() + 84 * (size_t)i);
        }
        if (!wr(out, pre.data(), pre.size())) { std::perror("write"); return 2; }
    }
    for (int t = 0; t < steps; ++t) {   // one lane of k_panda_episodes_post_v per episode and tick: the WORLD table's row
        for (int i = 0; i < n; ++i) {
            const m3::PandaSceneRT sc = m3::panda_scene_row_scene(uni, table[1].data(), n, i);
            m3::PandaWorld p;
            load(worlds.data() + 84 * (size_t)i, p);
            m3::PandaObs o;
            m3::panda_step(sc, p, u.data() + ((size_t)t * n + i) * 9, o, cs);
            store(p, worlds.data() + 84 * (size_t)i);
        }
        if (!wr(out, worlds.data(), worlds.size())) { std::perror("write"); return 2; }
    }
    if (std::fclose(out) != 0) { std::perror("close"); return 2; }
    if (bad_rows || bad) { std::fprintf(stderr, "%d of %d rows differ, %d refresh faults\n", bad_rows, 2 * n, bad); return 1; }
    std::printf("panda_episode_tables_host: ok (%d episodes, %d steps)\n", n, steps);
    return 0;
}
