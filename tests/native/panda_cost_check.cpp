// Stand-alone check (its own main) of the weighted panda_cost of csrc/panda_dyn.hpp through its host build
// (panda_cost_host.cpp).  Built twice by tests/test_panda_cost_weights_cpu.py -- plain and with -fsanitize=address,undefined --
// and run directly, on the CPU only.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -Itests/native/shim panda_cost_check.cpp -o panda_cost_check
//   panda_cost_check [rows.bin]      rows.bin: 7 goal floats, then n rows of 30 floats (oracle.panda.make_obs); without it a
//                                    small built-in table
// Over the rows, for reach / pick / place x single / multi-modal: the weighted form at the default weights equals the literal
// form bit for bit; all-zero weights give (+/-)0; negated weights give the negated cost bit for bit (with the collision test's
// shelf_force kept: it is inside the test, not a factor of the cost); a NaN weight shows in exactly the tasks that read it.
// One checksum line per table, so that the plain and the sanitized build can be compared.
#include "panda_cost_host.cpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int fails = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } \
    } while (0)

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv) {
    std::vector<float> goal(7), rows;
    if (argc > 1) {
        std::FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
        std::vector<float> all;
        float buf[256];
        size_t got;
        while ((got = std::fread(buf, sizeof(float), 256, f)) > 0) all.insert(all.end(), buf, buf + got);
        std::fclose(f);
        if (all.size() < 7 + 30 || (all.size() - 7) % 30 != 0) { std::printf("bad size %zu\n", all.size()); return 2; }
        goal.assign(all.begin(), all.begin() + 7);
        rows.assign(all.begin() + 7, all.end());
    } else {
        const float g[7] = {0.2f, 0.2f, 1.115f, 0.0f, 0.0f, 0.0f, 1.0f};
        goal.assign(g, g + 7);
        for (int i = 0; i < 9; ++i) {      // unit quaternions about z / x, a gripper above a cube, forces around the threshold
            const float a = 0.3f * (float)i, s = std::sin(a), c = std::cos(a);
            const float r[30] = {0.10f + 0.01f * i, -0.02f, 1.30f, 0.0f, 0.0f, s, c, 0.10f + 0.01f * i, 0.03f + 0.005f * i, 1.30f,
                                 0.2f, -0.2f + 0.02f * i, 1.06f, s, 0.0f, 0.0f, c, 0.2f, -0.2f, 1.06f, 0.0f, 0.0f, -s, c,
                                 0.01f * i, 0.0f, (i % 3 == 1) ? 0.03f : 0.0f, 0.0f, 0.0f, (i % 4 == 3) ? 0.2f : 0.0f};
            rows.insert(rows.end(), r, r + 30);
        }
    }
    const int n = (int)(rows.size() / 30);
    float dflt[7];
    pcw_default_weights(dflt);
    CHECK(dflt[0] == 10.0f && dflt[1] == 3.0f && dflt[2] == 10.0f && dflt[3] == 15.0f && dflt[4] == 1000.0f && dflt[5] == 4.0f && dflt[6] == 2.0f);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // which weights each task reads: reach 0 1, pick 2 3 4 5, place 6
    const int reads[3][7] = {{1, 1, 0, 0, 0, 0, 0}, {0, 0, 1, 1, 1, 1, 0}, {0, 0, 0, 0, 0, 0, 1}};
    std::vector<float> lit(n), got(n);
    for (int task = 4; task <= 6; ++task) {
        for (int mm = 0; mm <= 1; ++mm) {
            const int half = n / 2;
            pcw_cost(nullptr, task, mm, half, goal.data(), 0.05f, 0.5f, rows.data(), n, 0, lit.data());
            // the defaults
            pcw_cost(dflt, task, mm, half, goal.data(), 0.05f, 0.5f, rows.data(), n, 0, got.data());
            uint32_t sum = 0;
            for (int i = 0; i < n; ++i) { CHECK(bits(got[i]) == bits(lit[i])); CHECK(std::isfinite(lit[i])); sum = sum * 31u + bits(got[i]); }
            std::printf("task %d mm %d defaults %08x\n", task, mm, sum);
            // zero weights (shelf_force too: nothing of the shelf stand is in the test then)
            const float zero[7] = {0, 0, 0, 0, 0, 0, 0};
            pcw_cost(zero, task, mm, half, goal.data(), 0.05f, 0.5f, rows.data(), n, 0, got.data());
            for (int i = 0; i < n; ++i) CHECK(got[i] == 0.0f);
            // negated outer weights: the negated cost, bit for bit
            float neg[7];
            for (int j = 0; j < 7; ++j) neg[j] = (j == 5) ? dflt[j] : -dflt[j];
            pcw_cost(neg, task, mm, half, goal.data(), 0.05f, 0.5f, rows.data(), n, 0, got.data());
            sum = 0;
            for (int i = 0; i < n; ++i) { CHECK(bits(got[i]) == bits(-lit[i]) || (lit[i] == 0.0f && got[i] == 0.0f)); sum = sum * 31u + bits(got[i]); }
            std::printf("task %d mm %d negated %08x\n", task, mm, sum);
            // a NaN in one weight: NaN costs in the tasks that read it (the collision weight: in the rows that collide; the
            // shelf stand's: the test is false, no penalty), the literal bits elsewhere
            for (int j = 0; j < 7; ++j) {
                float w[7];
                std::memcpy(w, dflt, sizeof(w));
                w[j] = nan;
                pcw_cost(w, task, mm, half, goal.data(), 0.05f, 0.5f, rows.data(), n, 0, got.data());
                int n_nan = 0;
                for (int i = 0; i < n; ++i) {
                    n_nan += std::isnan(got[i]) ? 1 : 0;
                    if (!reads[task - 4][j]) CHECK(bits(got[i]) == bits(lit[i]));
                    else if (j != 4 && j != 5) CHECK(std::isnan(got[i]));
                    else CHECK(std::isnan(got[i]) || std::isfinite(got[i]));
                }
                std::printf("task %d mm %d nan %d: %d\n", task, mm, j, n_nan);
            }
        }
    }
    if (fails == 0) std::printf("panda_cost_check: ok\n");
    return fails == 0 ? 0 : 1;
}
