// Host program of the two-section panda_env table of m3_batch_command (a batch created with M3_BATCH_PANDA_RUNTIME) for
// tests/test_batch_panda_runtime_cpu.py: the product's csrc/batch_table_layout.hpp compiled by g++ (no HIP dependency).
// Arguments: sizeof BatchPandaEntry, sizeof BatchPandaEntryRT, sizeof UpdateArgs and their three alignments, as
// tests/native/batch_panda_entry_sizes.hip prints them.  For n = 1, 5 and 64 handles and every split (n - r literal, r run-time)
// it checks: the literal section starts the table, the run-time section follows it without overlap, each section starts on a
// multiple of its entry's alignment, the update section follows both, the total ends the update section and stays within what
// m3_batch_create_ex sizes a slot with for max_handles = n (and for a larger batch), and with r = 0 every offset and the total
// equal the layout of a batch without the flag.  Then the capacity against the maximum over all splits by enumeration.
// A program with its own main, so that it also runs under -fsanitize=address,undefined as it is.
//   g++ -O2 -std=c++17 batch_table_layout_rt_host.cpp -o batch_table_layout_rt_host && ./batch_table_layout_rt_host 1080 ...
#include <cstdio>
#include <cstdlib>

#include "../../m3p2i_aip_amd/csrc/batch_table_layout.hpp"

namespace {
long checks = 0;
int failures = 0;
void expect(bool ok, const char* what, int n, int r) {
    ++checks;
    if (ok) return;
    if (++failures <= 20) std::fprintf(stderr, "FAIL %s: %d handles, %d of them run-time\n", what, n, r);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s sizeof_entry sizeof_entry_rt sizeof_update alignof_entry alignof_entry_rt alignof_update\n", argv[0]);
        return 2;
    }
    size_t v[6];
    for (int i = 0; i < 6; ++i) v[i] = (size_t)std::strtoull(argv[i + 1], nullptr, 10);
    const size_t entry = v[0], entry_rt = v[1], update = v[2], a_entry = v[3], a_rt = v[4], a_update = v[5];
    if (!entry || !entry_rt || !update || !a_entry || !a_rt || !a_update) return 2;
    m3::BatchTableSizes plain{{584, 616, 760}, entry, update};   // (a batch without the flag: the member is left at its default)
    m3::BatchTableSizes flagged = plain;
    flagged.panda_entry_rt = entry_rt;
    expect(plain.panda_entry_rt == 0, "the unflagged sizes have no run-time entry", 0, 0);
    const int ns[] = {1, 5, 64};
    for (int n : ns) {
        const m3::BatchTableLayout old = m3::batch_table_layout_panda(plain, n);
        for (int r = 0; r <= n; ++r) {
            const int lit = n - r;
            const m3::BatchTableLayout l = m3::batch_table_layout_panda(flagged, lit, r);
            expect(l.off[0] == 0, "the literal section starts the table", n, r);
            expect(l.off[0] + (size_t)lit * entry <= l.off[1], "the run-time section is behind the literal one", n, r);
            expect(l.off[1] + (size_t)r * entry_rt <= l.upd_off, "the update section is behind the run-time one", n, r);
            expect(l.off[0] % a_entry == 0 && l.off[1] % a_rt == 0 && l.upd_off % a_update == 0, "each section is aligned for its entry", n, r);
            expect(l.off[1] % 16 == 0 && l.upd_off % 16 == 0, "sections start on multiples of 16", n, r);
            expect(l.total == l.upd_off + (size_t)n * update, "the update section ends the table", n, r);
            expect(l.total <= m3::batch_table_capacity(flagged, n), "the table stays within the slot", n, r);
            expect(l.total <= m3::batch_table_capacity(flagged, n + 3), "... and within a larger batch's", n, r);
            if (r == 0) {
                expect(l.off[0] == old.off[0] && l.upd_off == old.upd_off && l.total == old.total,
                       "without run-time entries: the unflagged layout", n, r);
                const m3::BatchTableLayout same = m3::batch_table_layout_panda(plain, n, 0);
                expect(same.upd_off == old.upd_off && same.total == old.total, "the default argument is no run-time entries", n, r);
                expect(old.upd_off == m3::align16((size_t)n * entry) && old.total == old.upd_off + (size_t)n * update,
                       "the unflagged layout is the single-section one", n, r);
            }
        }
    }
    // the capacity is the worst case over the panda splits and the point splits, not merely a bound
    for (int m = 1; m <= 70; ++m) {
        size_t worst = 0;
        for (int r = 0; r <= m; ++r) worst = std::max(worst, m3::batch_table_layout_panda(flagged, m - r, r).total);
        for (int a = 0; a <= m; ++a)
            for (int b = 0; a + b <= m; ++b) {
                const int k[3] = {a, b, m - a - b};
                worst = std::max(worst, m3::batch_table_layout(flagged, k).total);
            }
        expect(worst == m3::batch_table_capacity(flagged, m), "capacity equals the maximum over all splits", m, -1);
        expect(m3::batch_table_capacity(plain, m) <= m3::batch_table_capacity(flagged, m), "the flag never shrinks a slot", m, -1);
    }
    std::printf("%ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
