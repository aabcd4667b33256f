// Host program of m3_batch_command's table layout for tests/test_batch_table_layout_cpu.py: the product's
// csrc/batch_table_layout.hpp compiled by g++ (it has no HIP dependency).  For several sets of entry sizes -- first the
// library's own (m3_internal.hpp pins the three rollout entries with static_asserts) -- it runs the layout over every split
// (n_plain, n_weighted, n_scene) with a sum of at most 12 and over max_handles in {1, 2, 3, 7, 12} and checks: every section
// starts on a multiple of 16, no two sections overlap, the order is plain / weighted / scene / update, and the total never
// exceeds what m3_batch_create sizes a slot with for that max_handles; the same for the single section of a panda_env table.
// Then the capacity against the maximum over ALL splits by enumeration (max_handles up to 40: more than the 16 per section
// batch_table_capacity looks at).  A program with its own main, so that it also runs under -fsanitize=address,undefined as it is.
//   g++ -O2 -std=c++17 batch_table_layout_host.cpp -o batch_table_layout_host && ./batch_table_layout_host
#include <cstdio>

#include "../../m3p2i_aip_amd/csrc/batch_table_layout.hpp"

namespace {
long checks = 0;
int failures = 0;
void expect(bool ok, const char* what, const m3::BatchTableSizes& z, int a, int b, int c, int max_handles) {
    ++checks;
    if (ok) return;
    if (++failures <= 20)
        std::fprintf(stderr, "FAIL %s: sizes %zu/%zu/%zu panda %zu update %zu, split (%d, %d, %d), max_handles %d\n", what,
                     z.entry[0], z.entry[1], z.entry[2], z.panda_entry, z.update, a, b, c, max_handles);
}
}  // namespace

int main() {
    const m3::BatchTableSizes sets[] = {
        {{584, 616, 760}, 1080, 544},   // the library's
        {{760, 616, 584}, 1080, 544},   // the largest entry first
        {{584, 760, 616}, 24, 8},       // ... in the middle; a small panda entry, an update entry that is no multiple of 16
        {{4, 12, 20}, 4, 4},            // multiples of 4 only: gaps of 4, 8 and 12
        {{1, 3, 7}, 5, 1},              // no alignment of their own at all
        {{16, 32, 48}, 64, 16},         // no gaps
    };
    const int maxes[] = {1, 2, 3, 7, 12};
    for (const m3::BatchTableSizes& z : sets) {
        for (int a = 0; a <= 12; ++a)
            for (int b = 0; a + b <= 12; ++b)
                for (int c = 0; a + b + c <= 12; ++c) {
                    const int n[3] = {a, b, c};
                    const m3::BatchTableLayout l = m3::batch_table_layout(z, n);
                    const size_t start[4] = {l.off[0], l.off[1], l.off[2], l.upd_off};
                    expect(l.off[0] == 0, "the plain section starts the table", z, a, b, c, 0);
                    for (int v = 0; v < 4; ++v) expect(start[v] % 16 == 0, "section start is a multiple of 16", z, a, b, c, 0);
                    // order and no overlap: a section ends where or before the next one starts
                    for (int v = 0; v < 3; ++v)
                        expect(start[v] + (size_t)n[v] * z.entry[v] <= start[v + 1], "sections in order, not overlapping", z, a, b, c, 0);
                    expect(l.total == l.upd_off + (size_t)(a + b + c) * z.update, "the update section ends the table", z, a, b, c, 0);
                    for (int m : maxes)
                        if (a + b + c <= m)
                            expect(l.total <= m3::batch_table_capacity(z, m), "total within the slot", z, a, b, c, m);
                }
        for (int m : maxes)
            for (int n = 0; n <= m; ++n) {
                const m3::BatchTableLayout l = m3::batch_table_layout_panda(z, n);
                expect(l.upd_off % 16 == 0 && (size_t)n * z.panda_entry <= l.upd_off, "panda: update section aligned, behind the entries", z, n, 0, 0, m);
                expect(l.total == l.upd_off + (size_t)n * z.update && l.total <= m3::batch_table_capacity(z, m), "panda: total within the slot", z, n, 0, 0, m);
            }
        // the capacity is the worst case, not merely a bound
        for (int m = 1; m <= 40; ++m) {
            size_t worst = m3::batch_table_layout_panda(z, m).total;
            for (int a = 0; a <= m; ++a)
                for (int b = 0; a + b <= m; ++b) {
                    const int n[3] = {a, b, m - a - b};
                    worst = std::max(worst, m3::batch_table_layout(z, n).total);
                }
            expect(worst == m3::batch_table_capacity(z, m), "capacity equals the maximum over all splits", z, -1, -1, -1, m);
        }
    }
    std::printf("%ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
