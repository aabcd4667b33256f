// batch_table_layout.hpp -- where the sections of m3_batch_command's argument table lie (host only; no HIP dependency, so that
// tests/native/batch_table_layout_host.cpp can run it on its own).
//
// A point_env table: one section of rollout entries per variant (PointVariant: plain, weighted, scene -- each variant has an
// entry type of its own), in that order, in a batch created with the per-sample section then the section of the handles with an
// arena per sample (batch_table_layout4), then the handles' UpdateArgs.  A panda_env table: the section of literal rollout
// entries, in a batch created with M3_BATCH_PANDA_RUNTIME then the section of run-time entries (handles with a run-time
// workspace, tuned weights or a workspace per sample: a larger entry type), then the UpdateArgs.  Every section starts on a
// multiple of 16 bytes; a section without handles takes no room.
#pragma once
#include <algorithm>
#include <cstddef>

namespace m3 {

constexpr int BATCH_ROLLOUT_SECTIONS = 3;   // (POINT_VARIANTS, m3_internal.hpp)
struct BatchTableSizes {
    size_t entry[BATCH_ROLLOUT_SECTIONS];   // bytes of one rollout entry of each point_env variant
    size_t panda_entry, update;             // ... of a panda_env rollout entry, of one UpdateArgs
    size_t panda_entry_rt = 0;              // ... of a panda_env run-time entry; 0: a batch without M3_BATCH_PANDA_RUNTIME, whose
                                            // panda tables have the literal section only (with a default: may be left out)
    size_t point_entry_sv = 0;              // ... of a point_env per-sample entry (a handle with an arena per sample); 0: a batch
                                            // without that section, whose point tables have the three variants' sections only
                                            // (with a default: may be left out)
    size_t point_entry_pr = 0;              // ... of a point_env priors entry (a handle with prior samples); 0: a batch without
                                            // that section, whose point tables end with the per-sample section (last and with a
                                            // default: may be left out)
};
struct BatchTableLayout {
    size_t off[BATCH_ROLLOUT_SECTIONS];   // start of each rollout section (panda_env: 0 the literal, 1 the run-time entries)
    size_t upd_off;                       // start of the update section
    size_t total;                         // bytes of the table (what is copied to the device)
};
constexpr size_t align16(size_t n) { return (n + 15) / 16 * 16; }

// n[v]: handles of variant v in this call
inline BatchTableLayout batch_table_layout(const BatchTableSizes& z, const int n[BATCH_ROLLOUT_SECTIONS]) {
    BatchTableLayout l{};
    size_t end = 0, handles = 0;
    for (int v = 0; v < BATCH_ROLLOUT_SECTIONS; ++v) {
        l.off[v] = align16(end);
        end = l.off[v] + (size_t)n[v] * z.entry[v];
        handles += (size_t)n[v];
    }
    l.upd_off = align16(end);
    l.total = l.upd_off + handles * z.update;
    return l;
}
// The point_env table of a batch with the per-sample section: the three variants' sections, then the per-sample entries (n[3]
// of them), then the UpdateArgs.  Without per-sample handles the offsets and the total are those of batch_table_layout.
constexpr int BATCH_POINT_SECTIONS = BATCH_ROLLOUT_SECTIONS + 1;
struct BatchTableLayout4 {
    size_t off[BATCH_POINT_SECTIONS];   // start of each rollout section
    size_t upd_off, total;              // as BatchTableLayout's
};
inline size_t batch_point_entry(const BatchTableSizes& z, int v) { return v < BATCH_ROLLOUT_SECTIONS ? z.entry[v] : z.point_entry_sv; }
inline BatchTableLayout4 batch_table_layout4(const BatchTableSizes& z, const int n[BATCH_POINT_SECTIONS]) {
    BatchTableLayout4 l{};
    size_t end = 0, handles = 0;
    for (int v = 0; v < BATCH_POINT_SECTIONS; ++v) {
        l.off[v] = align16(end);   // (an empty fourth section starts where the update section does)
        end = l.off[v] + (size_t)n[v] * batch_point_entry(z, v);
        handles += (size_t)n[v];
    }
    l.upd_off = align16(end);
    l.total = l.upd_off + handles * z.update;
    return l;
}
// The point_env table of a batch with the priors section: the four sections above, then the entries of the handles with prior
// samples (n[4] of them), then the UpdateArgs.  Without such handles the offsets and the total are those of batch_table_layout4.
constexpr int BATCH_POINT_SECTIONS5 = BATCH_POINT_SECTIONS + 1;
struct BatchTableLayout5 {
    size_t off[BATCH_POINT_SECTIONS5];   // start of each rollout section
    size_t upd_off, total;               // as BatchTableLayout's
};
inline size_t batch_point_entry5(const BatchTableSizes& z, int v) { return v < BATCH_POINT_SECTIONS ? batch_point_entry(z, v) : z.point_entry_pr; }
inline BatchTableLayout5 batch_table_layout5(const BatchTableSizes& z, const int n[BATCH_POINT_SECTIONS5]) {
    BatchTableLayout5 l{};
    size_t end = 0, handles = 0;
    for (int v = 0; v < BATCH_POINT_SECTIONS5; ++v) {
        l.off[v] = align16(end);   // (an empty section starts where the next one does)
        end = l.off[v] + (size_t)n[v] * batch_point_entry5(z, v);
        handles += (size_t)n[v];
    }
    l.upd_off = align16(end);
    l.total = l.upd_off + handles * z.update;
    return l;
}
// n: handles with a literal entry, n_rt: with a run-time entry (only in a batch whose sizes have panda_entry_rt).  Without
// run-time entries the offsets and the total are those of the single-section table.
inline BatchTableLayout batch_table_layout_panda(const BatchTableSizes& z, int n, int n_rt = 0) {
    BatchTableLayout l{};
    l.off[1] = align16((size_t)n * z.panda_entry);
    l.off[2] = l.off[1] + (size_t)n_rt * z.panda_entry_rt;   // (no third section: where the second one ends)
    l.upd_off = align16(l.off[2]);
    l.total = l.upd_off + ((size_t)n + (size_t)n_rt) * z.update;
    return l;
}

// The largest total of any call with up to max_handles handles: what m3_batch_create gives a slot.  A handle more never makes
// a table smaller, so only the splits of exactly max_handles count.  Moving 16 handles from a section into the one with the
// largest entries keeps every alignment gap (16 entries are a multiple of 16 bytes) and does not shrink the table: the worst
// split has fewer than 16 handles in each of the other sections.  The same holds for the two sections of a panda_env table and
// for the four of a point_env table with the per-sample section (point_entry_sv != 0; without it nothing below is added).
inline size_t batch_table_capacity(const BatchTableSizes& z, int max_handles) {
    const int big = (int)(std::max_element(z.entry, z.entry + BATCH_ROLLOUT_SECTIONS) - z.entry);
    const int o1 = (big + 1) % BATCH_ROLLOUT_SECTIONS, o2 = (big + 2) % BATCH_ROLLOUT_SECTIONS;
    size_t worst = batch_table_layout_panda(z, max_handles).total;
    if (z.panda_entry_rt != 0)
        for (int a = 0; a < 16 && a <= max_handles; ++a)
            worst = std::max({worst, batch_table_layout_panda(z, a, max_handles - a).total,
                              batch_table_layout_panda(z, max_handles - a, a).total});
    for (int a = 0; a < 16 && a <= max_handles; ++a)
        for (int b = 0; b < 16 && a + b <= max_handles; ++b) {
            int n[BATCH_ROLLOUT_SECTIONS];
            n[o1] = a; n[o2] = b; n[big] = max_handles - a - b;
            worst = std::max(worst, batch_table_layout(z, n).total);
        }
    if (z.point_entry_sv != 0) {
        int big4 = 0;
        for (int v = 1; v < BATCH_POINT_SECTIONS; ++v)
            if (batch_point_entry(z, v) > batch_point_entry(z, big4)) big4 = v;
        const int p1 = (big4 + 1) % BATCH_POINT_SECTIONS, p2 = (big4 + 2) % BATCH_POINT_SECTIONS, p3 = (big4 + 3) % BATCH_POINT_SECTIONS;
        for (int a = 0; a < 16 && a <= max_handles; ++a)
            for (int b = 0; b < 16 && a + b <= max_handles; ++b)
                for (int c = 0; c < 16 && a + b + c <= max_handles; ++c) {
                    int n[BATCH_POINT_SECTIONS];
                    n[p1] = a; n[p2] = b; n[p3] = c; n[big4] = max_handles - a - b - c;
                    worst = std::max(worst, batch_table_layout4(z, n).total);
                }
    }
    // (the five sections of a point_env table with the priors section, by the same argument; point_entry_pr == 0 adds nothing)
    if (z.point_entry_pr != 0) {
        int big5 = 0;
        for (int v = 1; v < BATCH_POINT_SECTIONS5; ++v)
            if (batch_point_entry5(z, v) > batch_point_entry5(z, big5)) big5 = v;
        int o[BATCH_POINT_SECTIONS5 - 1];
        for (int r = 1; r < BATCH_POINT_SECTIONS5; ++r) o[r - 1] = (big5 + r) % BATCH_POINT_SECTIONS5;
        for (int a = 0; a < 16 && a <= max_handles; ++a)
            for (int b = 0; b < 16 && a + b <= max_handles; ++b)
                for (int c = 0; c < 16 && a + b + c <= max_handles; ++c)
                    for (int d = 0; d < 16 && a + b + c + d <= max_handles; ++d) {
                        int n[BATCH_POINT_SECTIONS5];
                        n[o[0]] = a; n[o[1]] = b; n[o[2]] = c; n[o[3]] = d; n[big5] = max_handles - a - b - c - d;
                        worst = std::max(worst, batch_table_layout5(z, n).total);
                    }
    }
    return worst;
}

}  // namespace m3
