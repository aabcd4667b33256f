// owned_blocks_check.cpp -- the ledger of m3p2i_aip_amd/csrc/owned_blocks.hpp bound to malloc / free, stand-alone (its own main;
// tests/test_owned_blocks_cpu.py builds it plain and with -fsanitize=address,undefined and runs it directly).  The release
// function records every call: each block must be released exactly once and by the function of its kind.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "owned_blocks.hpp"

using namespace m3;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::printf("owned_blocks_check: line %d: %s\n", __LINE__, #cond);      \
            return 1;                                                               \
        }                                                                           \
    } while (0)

static std::map<void*, BlockKind> g_live;                     // what was handed out and not released yet, with its kind
static std::vector<std::pair<BlockKind, void*>> g_released;   // every call of the release function, in order
static int g_bad = 0;                                         // releases of a block not live, or with another kind than its own

static void recording_release(BlockKind kind, void* p) {
    auto it = g_live.find(p);
    if (it == g_live.end() || it->second != kind) ++g_bad;
    else g_live.erase(it);
    g_released.push_back({kind, p});
    std::free(p);
}

static void* make(BlockKind kind, size_t bytes = 24) {
    void* p = std::malloc(bytes);
    if (p) g_live[p] = kind;
    return p;
}

// an allocator that fails on request: call number fail_at (1-based; 0: never)
struct FakeAlloc {
    int fail_at = 0, calls = 0;
    BlockKind kind = BLOCK_DEVICE;
    void* operator()() { return ++calls == fail_at ? nullptr : make(kind); }
};

static void* failing_grow(void*, size_t) { return nullptr; }

// the shape of ensure_sim / refresh_wave_order / upload_scene_rows: three views, allocated as one group on first use
struct Obj {
    OwnedBlocks mem{&recording_release, 8};
    int* order = nullptr;
    void* scratch = nullptr;
    float* sorted = nullptr;
};
static bool ensure(Obj& o, FakeAlloc& a) {
    if (o.order) return true;
    BlockGroup g(o.mem);
    a.kind = BLOCK_HOST;
    if (!own_block(o.mem, BLOCK_HOST, o.order, a)) return false;
    a.kind = BLOCK_PINNED;
    if (!own_block(o.mem, BLOCK_PINNED, o.scratch, a)) return false;
    a.kind = BLOCK_DEVICE;
    if (!own_block(o.mem, BLOCK_DEVICE, o.sorted, a)) return false;
    g.keep = true;
    return true;
}

int main() {
    const long long live0 = g_owned_blocks_live.load();
    {   // release_all: reverse order of adoption, each by its kind; twice is harmless
        OwnedBlocks l(&recording_release, 4);
        const BlockKind kinds[5] = {BLOCK_DEVICE, BLOCK_PINNED, BLOCK_HOST, BLOCK_EVENT, BLOCK_IPC};
        void* p[5];
        for (int i = 0; i < 5; ++i) CHECK(l.adopt(kinds[i], p[i] = make(kinds[i])));   // (the fifth grows the ledger)
        CHECK(l.size() == 5 && g_owned_blocks_live.load() == live0 + 5);
        l.release_all();
        CHECK(g_released.size() == 5 && l.size() == 0 && g_owned_blocks_live.load() == live0);
        for (int i = 0; i < 5; ++i) CHECK(g_released[i] == std::make_pair(kinds[4 - i], p[4 - i]));
        l.release_all();
        CHECK(g_released.size() == 5 && g_bad == 0 && g_live.empty());
    }
    g_released.clear();
    {   // release of one block, with a view: the view is nulled, the others stay; an unknown pointer is refused
        OwnedBlocks l(&recording_release, 4);
        float *a = nullptr, *b = nullptr, *c = nullptr;
        CHECK(l.adopt(BLOCK_DEVICE, static_cast<float*>(make(BLOCK_DEVICE)), a) && a);
        CHECK(l.adopt(BLOCK_PINNED, static_cast<float*>(make(BLOCK_PINNED)), b) && b);
        CHECK(l.adopt(BLOCK_DEVICE, static_cast<float*>(make(BLOCK_DEVICE)), c) && c);
        void* was_b = b;
        int other = 0;
        CHECK(!l.release(&other) && g_released.empty());
        CHECK(l.release(b) && b == nullptr && a && c && l.size() == 2);
        CHECK(g_released.size() == 1 && g_released[0] == std::make_pair(BLOCK_PINNED, was_b));
        CHECK(!l.release(was_b) && g_released.size() == 1);
        {   // ... and through the scope guard: every exit of the scope frees the temporary
            ScopedBlock<int> tmp(l);
            CHECK(own_block(l, BLOCK_DEVICE, tmp.p, [] { return make(BLOCK_DEVICE); }) && tmp.p && l.size() == 3);
        }
        CHECK(l.size() == 2 && g_released.size() == 2 && g_owned_blocks_live.load() == live0 + 2);
    }   // (the destructor releases what is left)
    CHECK(g_released.size() == 4 && g_bad == 0 && g_live.empty() && g_owned_blocks_live.load() == live0);
    g_released.clear();
    {   // rollback frees exactly the blocks since the mark, newest first, and no others
        OwnedBlocks l(&recording_release, 8);
        void* p[5];
        for (int i = 0; i < 2; ++i) CHECK(l.adopt(BLOCK_DEVICE, p[i] = make(BLOCK_DEVICE)));
        const size_t m = l.mark();
        for (int i = 2; i < 5; ++i) CHECK(l.adopt(BLOCK_PINNED, p[i] = make(BLOCK_PINNED)));
        l.rollback(m);
        CHECK(l.size() == 2 && g_released.size() == 3);
        for (int i = 0; i < 3; ++i) CHECK(g_released[i] == std::make_pair(BLOCK_PINNED, p[4 - i]));
        CHECK(g_live.count(p[0]) == 1 && g_live.count(p[1]) == 1 && g_owned_blocks_live.load() == live0 + 2);
        l.rollback(m);   // nothing since the mark: nothing happens
        CHECK(g_released.size() == 3);
    }
    CHECK(g_released.size() == 5 && g_bad == 0 && g_live.empty() && g_owned_blocks_live.load() == live0);
    g_released.clear();
    {   // adopt with growth failing: the block is released by its kind, the view stays null, the ledger is as it was
        OwnedBlocks l(&recording_release, 2);
        l.grow = &failing_grow;
        int *a = nullptr, *b = nullptr, *c = nullptr;
        CHECK(own_block(l, BLOCK_HOST, a, [] { return make(BLOCK_HOST); }));
        CHECK(own_block(l, BLOCK_HOST, b, [] { return make(BLOCK_HOST); }));
        void* lost = make(BLOCK_EVENT);
        CHECK(!l.adopt(BLOCK_EVENT, static_cast<int*>(lost), c) && c == nullptr && l.size() == 2);
        CHECK(g_released.size() == 1 && g_released[0] == std::make_pair(BLOCK_EVENT, lost));
        CHECK(!l.adopt(BLOCK_IPC, make(BLOCK_IPC)) && g_released.size() == 2 && g_released[1].first == BLOCK_IPC);
        CHECK(g_owned_blocks_live.load() == live0 + 2 && a && b);
    }
    CHECK(g_released.size() == 4 && g_bad == 0 && g_live.empty() && g_owned_blocks_live.load() == live0);
    {   // a ledger whose reservation failed holds nothing and still never leaks
        OwnedBlocks l(&recording_release, 0);
        l.grow = &failing_grow;
        CHECK(!l.adopt(BLOCK_DEVICE, make(BLOCK_DEVICE)) && l.size() == 0 && g_live.empty());
    }
    // the k-th allocation of a three-block group fails, k = 1, 2, 3: no block of the group is left, all three views are null,
    // blocks from before the group are untouched; the next call starts from a clean state and succeeds
    for (int k = 1; k <= 3; ++k) {
        g_released.clear();
        Obj o;
        void* before = nullptr;
        CHECK(own_block(o.mem, BLOCK_DEVICE, before, [] { return make(BLOCK_DEVICE); }));
        FakeAlloc fa;
        fa.fail_at = k;
        CHECK(!ensure(o, fa) && fa.calls == k);
        CHECK(o.order == nullptr && o.scratch == nullptr && o.sorted == nullptr);
        CHECK(o.mem.size() == 1 && before && g_live.size() == 1 && g_live.count(before) == 1);
        CHECK((int)g_released.size() == k - 1 && g_owned_blocks_live.load() == live0 + 1);
        FakeAlloc ok;
        CHECK(ensure(o, ok) && ok.calls == 3 && o.order && o.scratch && o.sorted && o.mem.size() == 4);
        CHECK(ensure(o, ok) && ok.calls == 3 && o.mem.size() == 4);   // a second call allocates nothing
        o.mem.release_all();
        CHECK(o.order == nullptr && o.scratch == nullptr && o.sorted == nullptr && before == nullptr);
        CHECK((int)g_released.size() == k - 1 + 4 && g_bad == 0 && g_live.empty());
    }
    CHECK(g_owned_blocks_live.load() == live0);
    std::printf("owned_blocks_check: ok\n");
    return 0;
}
