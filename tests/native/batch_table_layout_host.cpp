// Host program of m3_batch_command's table layout: the product's csrc/batch_table_layout.hpp compiled by g++ (it has no HIP
// dependency), one mode per Python test that runs it --
//   sections   tests/test_batch_table_layout_cpu.py: the three always-present point_env sections and the literal panda_env one,
//              for several sets of entry sizes (first the library's own, which m3_internal.hpp pins with static_asserts)
//   rt S...    tests/test_batch_panda_runtime_cpu.py: the two panda_env sections of a batch created with the run-time section
//   sv         tests/test_batch_point_rollout_scenes_cpu.py: the point_env table with the per-sample section
//   pr         tests/test_batch_prior_samples_cpu.py: ... with the priors section, with and without the per-sample one
//   frozen S...  the one layout and the one capacity against the header as it stood before the sections were described once
//              (transcribed below, namespace before), on the library's entry sizes
// S...: sizeof BatchPandaEntry, BatchPandaEntryRT, UpdateArgs and their three alignments, as tests/native/batch_panda_entry_sizes.hip
// prints them.  Every mode checks, over every split of a few handles over the sections: every section starts on a multiple of
// 16, the sections lie in their order and do not overlap, the update section ends the table, the total stays within the slot
// (and a larger batch's); without handles of a section the offsets and the total are those of a batch created without it; a
// section never shrinks a slot; and the capacity equals the maximum over ALL splits by enumeration (for more handles than the
// 16 per section batch_table_capacity looks at).  A program with its own main, so that it also runs under
// -fsanitize=address,undefined as it is.
//   g++ -O2 -std=c++17 batch_table_layout_host.cpp -o batch_table_layout_host && ./batch_table_layout_host sections
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../m3p2i_aip_amd/csrc/batch_table_layout.hpp"

// ---- csrc/batch_table_layout.hpp as it stood at deafd63 (three layout functions, a hand-rolled panda layout, a capacity of
// nested loops), its comments left out: what the `frozen` mode compares the one layout with ----
namespace before {
using m3::align16;
constexpr int BATCH_ROLLOUT_SECTIONS = 3;
struct BatchTableSizes {
    size_t entry[BATCH_ROLLOUT_SECTIONS];
    size_t panda_entry, update;
    size_t panda_entry_rt = 0;
    size_t point_entry_sv = 0;
    size_t point_entry_pr = 0;
};
struct BatchTableLayout {
    size_t off[BATCH_ROLLOUT_SECTIONS];
    size_t upd_off;
    size_t total;
};
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
constexpr int BATCH_POINT_SECTIONS = BATCH_ROLLOUT_SECTIONS + 1;
struct BatchTableLayout4 {
    size_t off[BATCH_POINT_SECTIONS];
    size_t upd_off, total;
};
inline size_t batch_point_entry(const BatchTableSizes& z, int v) { return v < BATCH_ROLLOUT_SECTIONS ? z.entry[v] : z.point_entry_sv; }
inline BatchTableLayout4 batch_table_layout4(const BatchTableSizes& z, const int n[BATCH_POINT_SECTIONS]) {
    BatchTableLayout4 l{};
    size_t end = 0, handles = 0;
    for (int v = 0; v < BATCH_POINT_SECTIONS; ++v) {
        l.off[v] = align16(end);
        end = l.off[v] + (size_t)n[v] * batch_point_entry(z, v);
        handles += (size_t)n[v];
    }
    l.upd_off = align16(end);
    l.total = l.upd_off + handles * z.update;
    return l;
}
constexpr int BATCH_POINT_SECTIONS5 = BATCH_POINT_SECTIONS + 1;
struct BatchTableLayout5 {
    size_t off[BATCH_POINT_SECTIONS5];
    size_t upd_off, total;
};
inline size_t batch_point_entry5(const BatchTableSizes& z, int v) { return v < BATCH_POINT_SECTIONS ? batch_point_entry(z, v) : z.point_entry_pr; }
inline BatchTableLayout5 batch_table_layout5(const BatchTableSizes& z, const int n[BATCH_POINT_SECTIONS5]) {
    BatchTableLayout5 l{};
    size_t end = 0, handles = 0;
    for (int v = 0; v < BATCH_POINT_SECTIONS5; ++v) {
        l.off[v] = align16(end);
        end = l.off[v] + (size_t)n[v] * batch_point_entry5(z, v);
        handles += (size_t)n[v];
    }
    l.upd_off = align16(end);
    l.total = l.upd_off + handles * z.update;
    return l;
}
inline BatchTableLayout batch_table_layout_panda(const BatchTableSizes& z, int n, int n_rt = 0) {
    BatchTableLayout l{};
    l.off[1] = align16((size_t)n * z.panda_entry);
    l.off[2] = l.off[1] + (size_t)n_rt * z.panda_entry_rt;
    l.upd_off = align16(l.off[2]);
    l.total = l.upd_off + ((size_t)n + (size_t)n_rt) * z.update;
    return l;
}
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
}  // namespace before

namespace {
using m3::BatchTableLayout;
using m3::BatchTableShape;
long checks = 0;
int failures = 0;
// n: the split (nullptr: none), max_handles: -1 none
void expect(bool ok, const char* what, const BatchTableShape& z, const int* n, int max_handles) {
    ++checks;
    if (ok) return;
    if (++failures > 20) return;
    std::fprintf(stderr, "FAIL %s: sizes", what);
    for (int v = 0; v < z.n_sections; ++v) std::fprintf(stderr, " %zu", z.entry[v]);
    std::fprintf(stderr, " update %zu, split", z.update);
    for (int v = 0; n && v < z.n_sections; ++v) std::fprintf(stderr, " %d", n[v]);
    std::fprintf(stderr, ", max_handles %d\n", max_handles);
}
// the library's point_env entry sizes (m3_internal.hpp's static_asserts), sections plain / weighted / scene / per-sample / priors
constexpr size_t PLAIN = 584, WEIGHTED = 616, SCENE = 760, PER_SAMPLE = 768, PRIORS = 872;
BatchTableShape point_shape(size_t sv, size_t pr, size_t update) { return {5, {PLAIN, WEIGHTED, SCENE, sv, pr}, update}; }
BatchTableShape panda_shape(size_t entry, size_t rt, size_t update) { return {2, {entry, rt}, update}; }
// what m3_batch_create sizes a slot with
size_t slot(const BatchTableShape& point, const BatchTableShape& panda, int max_handles) {
    return std::max(m3::batch_table_capacity(point, max_handles), m3::batch_table_capacity(panda, max_handles));
}
int sum(const BatchTableShape& z, const int* n) {
    int s = 0;
    for (int v = 0; v < z.n_sections; ++v) s += n[v];
    return s;
}
// f(n) for every split of up to (exact: exactly) m handles over z's sections
template <class F>
void splits(const BatchTableShape& z, int m, bool exact, F&& f, int v = 0, int* n = nullptr) {
    int first[m3::BATCH_MAX_SECTIONS] = {};
    if (!n) n = first;
    if (v == z.n_sections - 1) {
        for (n[v] = exact ? m : 0; n[v] <= m; ++n[v]) f(n);
        return;
    }
    for (n[v] = 0; n[v] <= m; ++n[v]) splits(z, m - n[v], exact, f, v + 1, n);
}
// the largest table of exactly m handles, by enumeration
size_t worst_split(const BatchTableShape& z, int m) {
    size_t worst = 0;
    splits(z, m, true, [&](const int* n) { worst = std::max(worst, m3::batch_table_layout(z, n).total); });
    return worst;
}
// one split: aligned, in order, disjoint, ended by the update section
void check_split(const BatchTableShape& z, const int* n, const BatchTableLayout& l) {
    bool aligned = l.upd_off % 16 == 0, ordered = l.off[0] == 0, disjoint = true;
    for (int v = 0; v < z.n_sections; ++v) {
        const size_t next = v + 1 < z.n_sections ? l.off[v + 1] : l.upd_off;
        aligned = aligned && l.off[v] % 16 == 0;
        ordered = ordered && l.off[v] <= next;
        disjoint = disjoint && l.off[v] + (size_t)n[v] * z.entry[v] <= next;
    }
    expect(aligned, "every section starts on a multiple of 16", z, n, -1);
    expect(ordered, "the first section starts the table, the sections lie in their order, the update section last", z, n, -1);
    expect(disjoint, "sections do not overlap", z, n, -1);
    expect(l.total == l.upd_off + (size_t)sum(z, n) * z.update, "the update section ends the table", z, n, -1);
}
// the same offsets (of the sections both have), update offset and total
bool same(const BatchTableLayout& x, const BatchTableLayout& y, int sections) {
    bool ok = x.upd_off == y.upd_off && x.total == y.total;
    for (int v = 0; v < sections; ++v) ok = ok && x.off[v] == y.off[v];
    return ok;
}
// every split of up to `most` handles over z's sections, and the slot (of z and `other`, the batch's other environment) for
// each max_handles of maxes; then the capacity of z by enumeration up to cap_to handles
void check_shape(const BatchTableShape& z, const BatchTableShape& other, int most, const int* maxes, int n_maxes, int cap_to) {
    splits(z, most, false, [&](const int* n) {
        const BatchTableLayout l = m3::batch_table_layout(z, n);
        check_split(z, n, l);
        for (int i = 0; i < n_maxes; ++i)
            if (sum(z, n) <= maxes[i]) {
                expect(l.total <= m3::batch_table_capacity(z, maxes[i]), "total within the shape's capacity", z, n, maxes[i]);
                expect(l.total <= slot(z, other, maxes[i]), "total within the slot", z, n, maxes[i]);
            }
    });
    for (int m = 1; m <= cap_to; ++m)
        expect(m3::batch_table_capacity(z, m) == worst_split(z, m), "capacity equals the maximum over all splits", z, nullptr, m);
}

// ---- sections: the always-present sections, for several sets of entry sizes ----
void mode_sections() {
    struct Sizes { size_t entry[3], panda, update; };
    const Sizes sets[] = {
        {{584, 616, 760}, 1080, 544},   // the library's
        {{760, 616, 584}, 1080, 544},   // the largest entry first
        {{584, 760, 616}, 24, 8},       // ... in the middle; a small panda entry, an update entry that is no multiple of 16
        {{4, 12, 20}, 4, 4},            // multiples of 4 only: gaps of 4, 8 and 12
        {{1, 3, 7}, 5, 1},              // no alignment of their own at all
        {{16, 32, 48}, 64, 16},         // no gaps
    };
    const int maxes[] = {1, 2, 3, 7, 12};
    for (const Sizes& s : sets) {
        const BatchTableShape three{3, {s.entry[0], s.entry[1], s.entry[2]}, s.update};
        const BatchTableShape five{5, {s.entry[0], s.entry[1], s.entry[2], 0, 0}, s.update};   // (as a batch created without a bit has it)
        const BatchTableShape panda{2, {s.panda, 0}, s.update}, panda_one{1, {s.panda}, s.update};
        check_shape(three, panda, 12, maxes, 5, 40);
        check_shape(panda_one, three, 12, maxes, 5, 40);
        // the sections a batch was created without take no room and change nothing
        splits(three, 12, false, [&](const int* n) {
            expect(same(m3::batch_table_layout(five, n), m3::batch_table_layout(three, n), 3), "absent sections change no offset", five, n, -1);
        });
        for (int m = 1; m <= 40; ++m) {
            expect(m3::batch_table_capacity(five, m) == m3::batch_table_capacity(three, m) && m3::batch_table_capacity(five, m) == worst_split(five, m),
                   "absent sections change no capacity", five, nullptr, m);
            expect(m3::batch_table_capacity(panda, m) == m3::batch_table_capacity(panda_one, m) && m3::batch_table_capacity(panda, m) == worst_split(panda, m),
                   "absent sections change no capacity", panda, nullptr, m);
        }
    }
}

// ---- rt: the two panda_env sections ----
void mode_rt(const size_t v[6]) {
    const size_t entry = v[0], entry_rt = v[1], update = v[2], a_entry = v[3], a_rt = v[4], a_update = v[5];
    const BatchTableShape plain = panda_shape(entry, 0, update), flagged = panda_shape(entry, entry_rt, update);
    const BatchTableShape single{1, {entry}, update}, point = point_shape(0, 0, update);
    const int ns[] = {1, 5, 64};
    for (int n : ns) {
        const int all_literal[2] = {n, 0};
        const BatchTableLayout old = m3::batch_table_layout(plain, all_literal);
        for (int r = 0; r <= n; ++r) {
            const int k[2] = {n - r, r};
            const BatchTableLayout l = m3::batch_table_layout(flagged, k);
            check_split(flagged, k, l);
            expect(l.off[0] == 0, "the literal section starts the table", flagged, k, n);
            expect(l.off[0] + (size_t)k[0] * entry <= l.off[1], "the run-time section is behind the literal one", flagged, k, n);
            expect(l.off[1] + (size_t)r * entry_rt <= l.upd_off, "the update section is behind the run-time one", flagged, k, n);
            expect(l.off[0] % a_entry == 0 && l.off[1] % a_rt == 0 && l.upd_off % a_update == 0, "each section is aligned for its entry", flagged, k, n);
            expect(l.total <= slot(point, flagged, n), "the table stays within the slot", flagged, k, n);
            expect(l.total <= slot(point, flagged, n + 3), "... and within a larger batch's", flagged, k, n);
            if (r == 0) {
                expect(same(l, old, 1), "without run-time entries: the unflagged layout", flagged, k, n);
                expect(same(m3::batch_table_layout(single, all_literal), old, 1) && old.upd_off == m3::align16((size_t)n * entry) &&
                           old.total == old.upd_off + (size_t)n * update,
                       "the unflagged layout is the single-section one", plain, k, n);
            }
        }
    }
    // the slot is the worst case over the panda splits and the point splits, not merely a bound
    for (int m = 1; m <= 70; ++m) {
        expect(m3::batch_table_capacity(flagged, m) == worst_split(flagged, m), "capacity equals the maximum over all splits", flagged, nullptr, m);
        expect(m3::batch_table_capacity(plain, m) == worst_split(single, m), "... of a batch without the flag: the single section's", plain, nullptr, m);
        expect(slot(point, plain, m) <= slot(point, flagged, m), "the flag never shrinks a slot", flagged, nullptr, m);
    }
    for (int m = 1; m <= 40; ++m)
        expect(slot(point, flagged, m) == std::max(worst_split(point, m), worst_split(flagged, m)), "the slot equals the maximum over all splits", point, nullptr, m);
}

// ---- sv: the point_env table with the per-sample section (an UpdateArgs that is no multiple of 16: every gap shows) ----
void mode_sv() {
    const BatchTableShape plain = point_shape(0, 0, 200), flagged = point_shape(PER_SAMPLE, 0, 200);
    const BatchTableShape three{3, {PLAIN, WEIGHTED, SCENE}, 200}, four{4, {PLAIN, WEIGHTED, SCENE, PER_SAMPLE}, 200};
    const BatchTableShape panda = panda_shape(1080, 0, 200), panda_rt = panda_shape(1080, 1200, 200);
    const int maxes[] = {1, 2, 3, 7, 12};
    check_shape(four, panda, 12, maxes, 5, 40);
    splits(four, 12, false, [&](const int* n) {
        const BatchTableLayout l = m3::batch_table_layout(flagged, n);
        expect(same(l, m3::batch_table_layout(four, n), 4) && l.off[4] == l.upd_off, "the absent priors section changes no offset", flagged, n, -1);
        if (n[3] == 0) {
            expect(same(l, m3::batch_table_layout(three, n), 3), "without per-sample handles: the three-section layout", flagged, n, -1);
            expect(same(l, m3::batch_table_layout(plain, n), 5), "... and that of a batch created without the section", flagged, n, -1);
        }
    });
    // the capacity by enumeration for more sizes, and what the section costs
    for (int m = 1; m <= 40; ++m) {
        expect(m3::batch_table_capacity(plain, m) == worst_split(three, m), "size 0: the capacity of a batch without the section", plain, nullptr, m);
        expect(m3::batch_table_capacity(flagged, m) == worst_split(four, m), "capacity equals the maximum over all splits", flagged, nullptr, m);
        expect(slot(flagged, panda, m) == std::max(worst_split(four, m), worst_split(panda, m)), "the slot equals the maximum over all splits", flagged, nullptr, m);
        expect(slot(plain, panda, m) <= slot(flagged, panda, m), "the section never shrinks a slot", flagged, nullptr, m);
        expect(slot(flagged, panda, m) <= slot(flagged, panda_rt, m), "nor does the panda section beside it", flagged, nullptr, m);
    }
}

// ---- pr: ... with the priors section, with and without the per-sample one ----
void mode_pr() {
    const BatchTableShape plain = point_shape(0, 0, 200), sv = point_shape(PER_SAMPLE, 0, 200);
    const BatchTableShape flagged = point_shape(PER_SAMPLE, PRIORS, 200), pr_only = point_shape(0, PRIORS, 200);
    const BatchTableShape four{4, {PLAIN, WEIGHTED, SCENE, PER_SAMPLE}, 200};
    const BatchTableShape panda = panda_shape(1080, 0, 200);
    const int maxes[] = {1, 2, 3, 7, 10};
    check_shape(flagged, panda, 10, maxes, 5, 24);
    splits(flagged, 10, false, [&](const int* n) {
        const BatchTableLayout l = m3::batch_table_layout(flagged, n);
        if (n[4] == 0) {
            expect(same(l, m3::batch_table_layout(four, n), 4), "without handles with priors: the four-section layout", flagged, n, -1);
            const BatchTableLayout z = m3::batch_table_layout(sv, n);
            expect(same(l, z, 5) && z.off[4] == z.upd_off, "... and that of a batch created without the section", flagged, n, -1);
        }
        if (n[3] == 0) {   // a batch with the priors section only: the fourth section takes no room
            const BatchTableLayout q = m3::batch_table_layout(pr_only, n);
            const int s = sum(pr_only, n);
            check_split(pr_only, n, q);
            expect(q.off[4] == q.off[3] && q.upd_off >= q.off[4] + (size_t)n[4] * PRIORS && q.total <= slot(pr_only, panda, s > 0 ? s : 1),
                   "the priors section without the per-sample one", pr_only, n, -1);
        }
    });
    // the capacity by enumeration for more sizes, what the section costs, and the section's size at 0
    for (int m = 1; m <= 24; ++m) {
        expect(slot(flagged, panda, m) == std::max(worst_split(flagged, m), worst_split(panda, m)), "the slot equals the maximum over all splits", flagged, nullptr, m);
        expect(m3::batch_table_capacity(pr_only, m) == worst_split(pr_only, m), "... of a batch with the priors section only", pr_only, nullptr, m);
        expect(m3::batch_table_capacity(sv, m) == worst_split(sv, m) && m3::batch_table_capacity(sv, m) == worst_split(four, m),
               "size 0: the capacity of a batch without the section", sv, nullptr, m);
        expect(slot(sv, panda, m) <= slot(flagged, panda, m) && slot(plain, panda, m) <= slot(pr_only, panda, m), "the section never shrinks a slot", flagged, nullptr, m);
    }
}

// ---- frozen: offsets, update offset, total and slot size against the header as it stood, for all 8 combinations of the section
// bits, every split of up to 12 handles and max_handles 1 .. 40 ----
void mode_frozen(const size_t v[6]) {
    const size_t entry = v[0], entry_rt = v[1], update = v[2];
    for (int bits = 0; bits < 8; ++bits) {
        const size_t rt = (bits & 1) ? entry_rt : 0, sv = (bits & 2) ? PER_SAMPLE : 0, pr = (bits & 4) ? PRIORS : 0;
        before::BatchTableSizes old{{PLAIN, WEIGHTED, SCENE}, entry, update};
        old.panda_entry_rt = rt; old.point_entry_sv = sv; old.point_entry_pr = pr;
        const BatchTableShape point = point_shape(sv, pr, update), panda = panda_shape(entry, rt, update);
        splits(point, 12, false, [&](const int* n) {
            const BatchTableLayout l = m3::batch_table_layout(point, n);
            const before::BatchTableLayout5 o = before::batch_table_layout5(old, n);
            bool ok = l.upd_off == o.upd_off && l.total == o.total;
            for (int s = 0; s < 5; ++s) ok = ok && l.off[s] == o.off[s];
            expect(ok, "point_env: the five-section layout as it stood", point, n, bits);
            if (n[4] == 0) {
                const before::BatchTableLayout4 o4 = before::batch_table_layout4(old, n);
                expect(l.off[0] == o4.off[0] && l.off[1] == o4.off[1] && l.off[2] == o4.off[2] && l.off[3] == o4.off[3] &&
                           l.upd_off == o4.upd_off && l.total == o4.total, "point_env: the four-section layout as it stood", point, n, bits);
            }
            if (n[4] == 0 && n[3] == 0) {
                const before::BatchTableLayout o3 = before::batch_table_layout(old, n);
                expect(l.off[0] == o3.off[0] && l.off[1] == o3.off[1] && l.off[2] == o3.off[2] && l.upd_off == o3.upd_off && l.total == o3.total,
                       "point_env: the three-section layout as it stood", point, n, bits);
            }
        });
        splits(panda, 12, false, [&](const int* n) {
            const BatchTableLayout l = m3::batch_table_layout(panda, n);
            const before::BatchTableLayout o = before::batch_table_layout_panda(old, n[0], n[1]);
            expect(l.off[0] == 0 && l.off[1] == o.off[1] && l.upd_off == o.upd_off && l.total == o.total, "panda_env: the layout as it stood", panda, n, bits);
        });
        for (int m = 1; m <= 40; ++m)
            expect(slot(point, panda, m) == before::batch_table_capacity(old, m), "the slot's size as it stood", point, nullptr, m);
    }
}
}  // namespace

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    const bool sized = !std::strcmp(mode, "rt") || !std::strcmp(mode, "frozen");
    size_t v[6] = {};
    if (sized) {
        if (argc != 8) {
            std::fprintf(stderr, "usage: %s %s sizeof_entry sizeof_entry_rt sizeof_update alignof_entry alignof_entry_rt alignof_update\n", argv[0], mode);
            return 2;
        }
        for (int i = 0; i < 6; ++i)
            if (!(v[i] = (size_t)std::strtoull(argv[i + 2], nullptr, 10))) return 2;
    }
    if (!std::strcmp(mode, "sections")) mode_sections();
    else if (!std::strcmp(mode, "rt")) mode_rt(v);
    else if (!std::strcmp(mode, "sv")) mode_sv();
    else if (!std::strcmp(mode, "pr")) mode_pr();
    else if (!std::strcmp(mode, "frozen")) mode_frozen(v);
    else {
        std::fprintf(stderr, "usage: %s sections | rt S... | sv | pr | frozen S...\n", argv[0]);
        return 2;
    }
    std::printf("%ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
