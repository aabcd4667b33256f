// Host program of the five-section point_env table of m3_batch_command (a batch created with M3_BATCH_SECTION_POINT_PRIORS) for
// tests/test_batch_prior_samples_cpu.py: the product's csrc/batch_table_layout.hpp compiled by g++ (no HIP dependency).  Entry
// sizes as m3_internal.hpp pins them (584 / 616 / 760, per-sample 768, priors 872) and an UpdateArgs that is no multiple of 16,
// so that every alignment gap shows.
// Over every split (plain, weighted, scene, per-sample, priors) with a sum of at most 10 and max_handles in {1, 2, 3, 7, 10}:
// every section starts on a multiple of 16, the order is plain / weighted / scene / per-sample / priors / update, sections do
// not overlap, the total ends the update section and stays within the slot's capacity; with no handle in the fifth section the
// offsets and the total are the four-section function's.  Then the capacity against the maximum over all splits by enumeration;
// with the new size at 0 every function returns what it returned without it; and a batch with the priors section but without
// the per-sample one.
// A program with its own main, so that it also runs under -fsanitize=address,undefined as it is.
//   g++ -O2 -std=c++17 batch_table_layout_pr_host.cpp -o batch_table_layout_pr_host && ./batch_table_layout_pr_host
#include <cstdio>

#include "../../m3p2i_aip_amd/csrc/batch_table_layout.hpp"

namespace {
long checks = 0;
int failures = 0;
void expect(bool ok, const char* what, const int n[5], int max_handles) {
    ++checks;
    if (ok) return;
    if (++failures <= 20)
        std::fprintf(stderr, "FAIL %s: split %d/%d/%d/%d/%d, max_handles %d\n", what, n ? n[0] : -1, n ? n[1] : -1, n ? n[2] : -1,
                     n ? n[3] : -1, n ? n[4] : -1, max_handles);
}
// the largest table of exactly m handles, by enumeration of every five-section split
size_t worst5(const m3::BatchTableSizes& z, int m) {
    size_t worst = 0;
    for (int a = 0; a <= m; ++a)
        for (int b = 0; a + b <= m; ++b)
            for (int c = 0; a + b + c <= m; ++c)
                for (int d = 0; a + b + c + d <= m; ++d) {
                    const int k[5] = {a, b, c, d, m - a - b - c - d};
                    worst = std::max(worst, m3::batch_table_layout5(z, k).total);
                }
    return worst;
}
}  // namespace

int main() {
    static_assert(m3::BATCH_ROLLOUT_SECTIONS == 3 && m3::BATCH_POINT_SECTIONS == 4 && m3::BATCH_POINT_SECTIONS5 == 5, "");
    // (the initialiser of the older host programs: the new members are left at their defaults)
    const m3::BatchTableSizes plain{{584, 616, 760}, 1080, 200};
    expect(plain.point_entry_pr == 0 && plain.point_entry_sv == 0 && plain.panda_entry_rt == 0, "the members with a default are 0", nullptr, 0);
    m3::BatchTableSizes sv = plain;
    sv.point_entry_sv = 768;
    m3::BatchTableSizes flagged = sv;       // both point sections
    flagged.point_entry_pr = 872;
    m3::BatchTableSizes pr_only = plain;    // the priors section without the per-sample one
    pr_only.point_entry_pr = 872;
    const size_t size[5] = {584, 616, 760, 768, 872};
    const int maxes[] = {1, 2, 3, 7, 10};
    for (int max_handles : maxes) {
        const size_t cap = m3::batch_table_capacity(flagged, max_handles);
        size_t worst = m3::batch_table_layout_panda(flagged, max_handles).total;
        for (int a = 0; a <= 10; ++a)
            for (int b = 0; a + b <= 10; ++b)
                for (int c = 0; a + b + c <= 10; ++c)
                    for (int d = 0; a + b + c + d <= 10; ++d)
                        for (int e = 0; a + b + c + d + e <= 10; ++e) {
                            const int n[5] = {a, b, c, d, e};
                            const int sum = a + b + c + d + e;
                            const m3::BatchTableLayout5 l = m3::batch_table_layout5(flagged, n);
                            bool aligned = l.upd_off % 16 == 0, ordered = l.off[0] == 0, disjoint = true;
                            for (int v = 0; v < 5; ++v) {
                                aligned = aligned && l.off[v] % 16 == 0;
                                const size_t end = l.off[v] + (size_t)n[v] * size[v];
                                const size_t next = v < 4 ? l.off[v + 1] : l.upd_off;
                                ordered = ordered && l.off[v] <= next;
                                disjoint = disjoint && end <= next;
                            }
                            expect(aligned, "every section starts on a multiple of 16", n, max_handles);
                            expect(ordered, "plain / weighted / scene / per-sample / priors / update", n, max_handles);
                            expect(disjoint, "sections do not overlap", n, max_handles);
                            expect(l.total == l.upd_off + (size_t)sum * 200, "the update section ends the table", n, max_handles);
                            if (sum <= max_handles) {
                                expect(l.total <= cap, "the table stays within the slot", n, max_handles);
                                worst = std::max(worst, l.total);
                            }
                            if (e == 0) {
                                const m3::BatchTableLayout4 o = m3::batch_table_layout4(flagged, n);
                                expect(o.off[0] == l.off[0] && o.off[1] == l.off[1] && o.off[2] == l.off[2] && o.off[3] == l.off[3] &&
                                           o.upd_off == l.upd_off && o.total == l.total,
                                       "without handles with priors: the four-section layout", n, max_handles);
                                const m3::BatchTableLayout4 p = m3::batch_table_layout4(sv, n);
                                expect(p.upd_off == o.upd_off && p.total == o.total, "... which does not read the new size", n, max_handles);
                                // the new size at 0: the five-section function is the four-section one
                                const m3::BatchTableLayout5 z = m3::batch_table_layout5(sv, n);
                                expect(z.off[3] == p.off[3] && z.off[4] == p.upd_off && z.upd_off == p.upd_off && z.total == p.total,
                                       "size 0: the five-section layout is the four-section one", n, max_handles);
                            }
                            if (d == 0) {   // a batch with the priors section only: the fourth section takes no room
                                const m3::BatchTableLayout5 q = m3::batch_table_layout5(pr_only, n);
                                expect(q.off[4] == q.off[3] && q.off[4] % 16 == 0 && q.upd_off >= q.off[4] + (size_t)e * 872 &&
                                           q.total <= m3::batch_table_capacity(pr_only, sum > 0 ? sum : 1),
                                       "the priors section without the per-sample one", n, max_handles);
                            }
                        }
        expect(worst == cap, "capacity equals the maximum over all splits", nullptr, max_handles);
    }
    // the capacity by enumeration for more sizes, what the section costs, and the new size at 0
    for (int m = 1; m <= 24; ++m) {
        expect(m3::batch_table_capacity(flagged, m) == std::max(worst5(flagged, m), m3::batch_table_layout_panda(flagged, m).total),
               "capacity equals the maximum over all splits", nullptr, m);
        expect(m3::batch_table_capacity(pr_only, m) == std::max(worst5(pr_only, m), m3::batch_table_layout_panda(pr_only, m).total),
               "... of a batch with the priors section only", nullptr, m);
        expect(m3::batch_table_capacity(sv, m) == std::max(worst5(sv, m), m3::batch_table_layout_panda(sv, m).total),
               "size 0: the capacity of a batch without the section", nullptr, m);
        expect(m3::batch_table_capacity(sv, m) <= m3::batch_table_capacity(flagged, m) &&
                   m3::batch_table_capacity(plain, m) <= m3::batch_table_capacity(pr_only, m),
               "the section never shrinks a slot", nullptr, m);
    }
    std::printf("%ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
