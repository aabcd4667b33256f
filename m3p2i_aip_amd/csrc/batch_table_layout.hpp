// batch_table_layout.hpp -- where the sections of m3_batch_command's argument table lie (host only; no HIP dependency, so that
// tests/native/batch_table_layout_host.cpp can run it on its own).
//
// A table is an ordered list of sections of rollout entries, one entry type each, then the handles' UpdateArgs.  Every section
// starts on a multiple of 16 bytes; a section without handles takes no room.  Which sections an environment's table has, and
// in which order, is m3_api.hip's section table.
#pragma once
#include <algorithm>
#include <cstddef>

namespace m3 {

constexpr int BATCH_MAX_SECTIONS = 8;
struct BatchTableShape {
    int n_sections;
    size_t entry[BATCH_MAX_SECTIONS];   // bytes of one rollout entry of each section; 0: a section the batch was created without
    size_t update;                      // ... of one UpdateArgs
};
struct BatchTableLayout {
    size_t off[BATCH_MAX_SECTIONS];   // start of each rollout section (an empty one starts where the next one does)
    size_t upd_off;                   // start of the update section
    size_t total;                     // bytes of the table (what is copied to the device)
};
constexpr size_t align16(size_t n) { return (n + 15) / 16 * 16; }

// n[v]: handles of section v in this call
inline BatchTableLayout batch_table_layout(const BatchTableShape& z, const int n[]) {
    BatchTableLayout l{};
    size_t end = 0, handles = 0;
    for (int v = 0; v < z.n_sections; ++v) {
        l.off[v] = align16(end);
        end = l.off[v] + (size_t)n[v] * z.entry[v];
        handles += (size_t)n[v];
    }
    l.upd_off = align16(end);
    l.total = l.upd_off + handles * z.update;
    return l;
}

// The largest total of any call with up to max_handles handles: what m3_batch_create sizes a slot for (the larger of its two
// environments' shapes).  A handle more never makes a table smaller, so only the splits of exactly max_handles count.  Moving
// 16 handles from a section into the one with the largest entries keeps every alignment gap (16 entries are a multiple of 16
// bytes) and does not shrink the table: the worst split has fewer than 16 handles in each of the other sections, and none in
// a section of size 0.  batch_table_worst tries those splits from section v on, `left` handles still to place.
inline size_t batch_table_worst(const BatchTableShape& z, int big, int v, int left, int n[]) {
    if (v == z.n_sections) {
        n[big] = left;
        return batch_table_layout(z, n).total;
    }
    if (v == big || z.entry[v] == 0) return batch_table_worst(z, big, v + 1, left, n);
    size_t worst = 0;
    for (n[v] = 0; n[v] < 16 && n[v] <= left; ++n[v]) worst = std::max(worst, batch_table_worst(z, big, v + 1, left - n[v], n));
    return worst;
}
inline size_t batch_table_capacity(const BatchTableShape& z, int max_handles) {
    const int big = (int)(std::max_element(z.entry, z.entry + z.n_sections) - z.entry);
    int n[BATCH_MAX_SECTIONS] = {};
    return batch_table_worst(z, big, 0, max_handles, n);
}

}  // namespace m3
