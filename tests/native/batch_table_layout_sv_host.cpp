// Host program of the four-section point_env table of m3_batch_command (a batch created with
// M3_BATCH_SECTION_POINT_ROLLOUT_SCENES) for tests/test_batch_point_rollout_scenes_cpu.py: the product's
// csrc/batch_table_layout.hpp compiled by g++ (no HIP dependency).  Entry sizes as m3_internal.hpp pins them (584 / 616 / 760,
// per-sample 768) and an UpdateArgs that is no multiple of 16, so that every alignment gap shows.
// Over every split (plain, weighted, scene, per-sample) with a sum of at most 12 and max_handles in {1, 2, 3, 7, 12}: every
// section starts on a multiple of 16, the order is plain / weighted / scene / per-sample / update, sections do not overlap,
// the total ends the update section and stays within the slot's capacity; with no per-sample handle the offsets and the
// total are the three-section function's.  Then the capacity against the maximum over all splits by enumeration, and with
// the per-sample size left at 0 the capacity of a batch without the section.
// A program with its own main, so that it also runs under -fsanitize=address,undefined as it is.
//   g++ -O2 -std=c++17 batch_table_layout_sv_host.cpp -o batch_table_layout_sv_host && ./batch_table_layout_sv_host
#include <cstdio>

#include "../../m3p2i_aip_amd/csrc/batch_table_layout.hpp"

namespace {
long checks = 0;
int failures = 0;
void expect(bool ok, const char* what, const int n[4], int max_handles) {
    ++checks;
    if (ok) return;
    if (++failures <= 20)
        std::fprintf(stderr, "FAIL %s: split %d/%d/%d/%d, max_handles %d\n", what, n ? n[0] : -1, n ? n[1] : -1, n ? n[2] : -1,
                     n ? n[3] : -1, max_handles);
}
}  // namespace

int main() {
    static_assert(m3::BATCH_ROLLOUT_SECTIONS == 3 && m3::BATCH_POINT_SECTIONS == 4, "");
    // (the initialiser of the two older host programs: the new member is left at its default)
    const m3::BatchTableSizes plain{{584, 616, 760}, 1080, 200};
    expect(plain.point_entry_sv == 0 && plain.panda_entry_rt == 0, "the members with a default are 0", nullptr, 0);
    m3::BatchTableSizes flagged = plain;
    flagged.point_entry_sv = 768;
    m3::BatchTableSizes both = flagged;   // (with the panda run-time section as well)
    both.panda_entry_rt = 1200;
    const size_t size[4] = {584, 616, 760, 768};
    const int maxes[] = {1, 2, 3, 7, 12};
    for (int max_handles : maxes) {
        const size_t cap = m3::batch_table_capacity(flagged, max_handles);
        size_t worst = m3::batch_table_layout_panda(flagged, max_handles).total;
        for (int a = 0; a <= 12; ++a)
            for (int b = 0; a + b <= 12; ++b)
                for (int c = 0; a + b + c <= 12; ++c)
                    for (int d = 0; a + b + c + d <= 12; ++d) {
                        const int n[4] = {a, b, c, d};
                        const int sum = a + b + c + d;
                        const m3::BatchTableLayout4 l = m3::batch_table_layout4(flagged, n);
                        bool aligned = l.upd_off % 16 == 0, ordered = l.off[0] == 0, disjoint = true;
                        for (int v = 0; v < 4; ++v) {
                            aligned = aligned && l.off[v] % 16 == 0;
                            const size_t end = l.off[v] + (size_t)n[v] * size[v];
                            const size_t next = v < 3 ? l.off[v + 1] : l.upd_off;
                            ordered = ordered && l.off[v] <= next;
                            disjoint = disjoint && end <= next;
                        }
                        expect(aligned, "every section starts on a multiple of 16", n, max_handles);
                        expect(ordered, "plain / weighted / scene / per-sample / update", n, max_handles);
                        expect(disjoint, "sections do not overlap", n, max_handles);
                        expect(l.total == l.upd_off + (size_t)sum * 200, "the update section ends the table", n, max_handles);
                        if (sum <= max_handles) {
                            expect(l.total <= cap, "the table stays within the slot", n, max_handles);
                            worst = std::max(worst, l.total);
                        }
                        if (d == 0) {
                            const m3::BatchTableLayout o = m3::batch_table_layout(flagged, n);
                            expect(o.off[0] == l.off[0] && o.off[1] == l.off[1] && o.off[2] == l.off[2] && o.upd_off == l.upd_off &&
                                       o.total == l.total,
                                   "without per-sample handles: the three-section layout", n, max_handles);
                            const m3::BatchTableLayout p = m3::batch_table_layout(plain, n);
                            expect(p.upd_off == o.upd_off && p.total == o.total, "... which does not read the new size", n, max_handles);
                        }
                    }
        expect(worst == cap, "capacity equals the maximum over all splits", nullptr, max_handles);
    }
    // the capacity by enumeration for more sizes, and what the section costs
    for (int m = 1; m <= 40; ++m) {
        size_t worst3 = m3::batch_table_layout_panda(plain, m).total, worst4 = worst3;
        for (int a = 0; a <= m; ++a)
            for (int b = 0; a + b <= m; ++b) {
                const int k[3] = {a, b, m - a - b};
                worst3 = std::max(worst3, m3::batch_table_layout(plain, k).total);
                for (int c = 0; a + b + c <= m; ++c) {
                    const int k4[4] = {a, b, c, m - a - b - c};
                    worst4 = std::max(worst4, m3::batch_table_layout4(flagged, k4).total);
                }
            }
        expect(m3::batch_table_capacity(plain, m) == worst3, "size 0: the capacity of a batch without the section", nullptr, m);
        expect(m3::batch_table_capacity(flagged, m) == worst4, "capacity equals the maximum over all splits", nullptr, m);
        expect(worst3 <= worst4, "the section never shrinks a slot", nullptr, m);
        expect(m3::batch_table_capacity(flagged, m) <= m3::batch_table_capacity(both, m), "nor does the panda section beside it", nullptr, m);
    }
    std::printf("%ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
