// Host program of the per-environment arenas (m3_set_point_scene_rows) for tests/test_point_scene_rows_cpu.py: the product's
// csrc/point_scene_rows.hpp and planar_dyn.hpp compiled by g++, one lane per "wavefront".  It packs the arenas into the
// word-major table as m3_set_point_scene_rows does (make_point_scene_rt, point_scene_row_pack), rebuilds each row's PointSceneRT
// as the kernels k_sim_step_sv / k_episodes_post_sv do (point_scene_row_load on the handle's scene_rt) and steps every world in
// its row's arena -- against the oracle with that arena, without a GPU.  A program with its own main, so that it also runs under
// -fsanitize=address,undefined as it is.
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -Itests/native/shim point_scene_rows_host.cpp -o point_scene_rows_host
//   point_scene_rows_host IN OUT
// IN  (binary, 4-byte words): int n, steps, n_arenas, substeps, iters; float dt; float arenas[n_arenas][28] (m3_point_scene);
//     int arena_of_row[n]; float worlds[n][31] (the oracle's rows); float u[steps][n][2]
// OUT: float worlds[steps][n][31] after each step
#include <cstdio>
#include <vector>

#include "../../m3p2i_aip_amd/csrc/point_scene_rows.hpp"

namespace {
void load(const float* w, m3::PointWorld& p) {   // oracle row (31 floats): 3 bodies x (x y c s vx vy w) | fext R, B | fc R, B, D
    p.rx = w[0]; p.ry = w[1]; p.rvx = w[4]; p.rvy = w[5];
    p.B = {w[7], w[8], w[9], w[10], w[11], w[12], w[13]};
    p.D = {w[14], w[15], w[16], w[17], w[18], w[19], w[20]};
    p.fRx = w[21]; p.fRy = w[22]; p.fBx = w[23]; p.fBy = w[24];
    p.fcRx = w[25]; p.fcRy = w[26]; p.fcBx = w[27]; p.fcBy = w[28]; p.fcDx = w[29]; p.fcDy = w[30];
}
void store(const m3::PointWorld& p, float* w) {
    w[0] = p.rx; w[1] = p.ry; w[4] = p.rvx; w[5] = p.rvy;
    const m3::Box* b[2] = {&p.B, &p.D};
    for (int i = 0; i < 2; ++i) {
        float* o = w + 7 + 7 * i;
        o[0] = b[i]->x; o[1] = b[i]->y; o[2] = b[i]->c; o[3] = b[i]->s; o[4] = b[i]->vx; o[5] = b[i]->vy; o[6] = b[i]->w;
    }
    w[21] = p.fRx; w[22] = p.fRy; w[23] = p.fBx; w[24] = p.fBy;
    w[25] = p.fcRx; w[26] = p.fcRy; w[27] = p.fcBx; w[28] = p.fcBy; w[29] = p.fcDx; w[30] = p.fcDy;
}
template <class T>
bool rd(std::FILE* f, T* p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    int head[5];
    float dt;
    if (!rd(in, head, 5) || !rd(in, &dt, 1)) { std::fprintf(stderr, "short header\n"); return 2; }
    const int n = head[0], steps = head[1], n_arenas = head[2], substeps = head[3], iters = head[4];
    if (n <= 0 || n > 1 << 20 || steps <= 0 || steps > 1 << 10 || n_arenas <= 0 || n_arenas > 1 << 10) {
        std::fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<m3_point_scene> arenas(n_arenas);
    std::vector<int> arena_of(n);
    std::vector<float> worlds((size_t)n * 31), u((size_t)steps * n * 2);
    if (!rd(in, arenas.data(), arenas.size()) || !rd(in, arena_of.data(), arena_of.size()) || !rd(in, worlds.data(), worlds.size()) ||
        !rd(in, u.data(), u.size())) {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    std::fclose(in);
    for (int i = 0; i < n; ++i)
        if (arena_of[i] < 0 || arena_of[i] >= n_arenas) { std::fprintf(stderr, "row %d: no such arena\n", i); return 2; }

    // the table as m3_set_point_scene_rows uploads it: [POINT_SCENE_ROW_WORDS][n]
    std::vector<float> table((size_t)m3::POINT_SCENE_ROW_WORDS * n);
    for (int i = 0; i < n; ++i)
        m3::point_scene_row_pack(m3::make_point_scene_rt(arenas[arena_of[i]], dt, substeps, iters), table.data(), n, i);
    // the handle's own scene_rt, of which the kernels read the uniform members only: an arena that is none of the rows' (every
    // field of the default times 1.37), so a per-arena member that did not come from the table would show
    m3_point_scene other = m3::POINT_SCENE_DEFAULT;
    float* of = reinterpret_cast<float*>(&other);
    for (int k = 0; k < 28; ++k) of[k] *= 1.37f;
    const m3::PointSceneRT uni = m3::make_point_scene_rt(other, dt, substeps, iters);

    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    for (int t = 0; t < steps; ++t) {
        for (int i = 0; i < n; ++i) {   // one lane of k_sim_step_sv
            const m3::PointSceneRT sc = m3::point_scene_row_load(uni, table.data(), n, i);
            m3::PointWorld p;
            load(worlds.data() + 31 * (size_t)i, p);
            const float* uu = u.data() + ((size_t)t * n + i) * 2;
            m3::point_step<true>(sc, p, uu[0], uu[1]);
            store(p, worlds.data() + 31 * (size_t)i);
        }
        if (std::fwrite(worlds.data(), sizeof(float), worlds.size(), out) != worlds.size()) { std::perror("write"); return 2; }
    }
    std::fclose(out);
    return 0;
}
