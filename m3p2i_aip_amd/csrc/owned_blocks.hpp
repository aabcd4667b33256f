// owned_blocks.hpp -- the ledger that owns the memory of a C object (m3_handle, m3_batch, m3_episodes, m3_panda_episodes).
// Host only, no HIP header: the one function that releases a block by kind comes from outside (m3_api.hip binds it to HIP,
// tests/native/owned_blocks_check.cpp to malloc / free).  The objects' named pointers are non-owning VIEWS of ledger entries: a
// block comes to life through own_block (allocate, adopt, write the view) and dies in release / rollback / release_all, which
// null the view again.  Nothing is adopted on a command, rollout, tick or step path.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdlib>

namespace m3 {

enum BlockKind { BLOCK_DEVICE, BLOCK_PINNED, BLOCK_HOST, BLOCK_EVENT, BLOCK_IPC };   // hipFree | hipHostFree | std::free | hipEventDestroy | hipIpcCloseMemHandle
using BlockRelease = void (*)(BlockKind, void*);

// blocks held by all ledgers of the process (m3_owned_blocks_live)
inline std::atomic<long long> g_owned_blocks_live{0};

class OwnedBlocks {
public:
    // capacity is reserved here, so that adopt does not have to grow on any path of the library
    explicit OwnedBlocks(BlockRelease release, size_t reserve = 16) : release_(release) { (void)grow_to(reserve); }
    ~OwnedBlocks() { release_all(); std::free(e_); }
    OwnedBlocks(const OwnedBlocks&) = delete;
    OwnedBlocks& operator=(const OwnedBlocks&) = delete;

    // takes p over, never leaks it: if the ledger cannot grow, p is released here and the answer is false.  With a view: the
    // object's pointer to the block (it must live as long as the entry), written here and nulled when the block is released
    bool adopt(BlockKind kind, void* p) { return adopt_entry({p, kind, nullptr, nullptr}); }
    template <class T> bool adopt(BlockKind kind, T* p, T*& view) {
        view = nullptr;
        if (!adopt_entry({p, kind, &view, [](void* v) { *static_cast<T**>(v) = nullptr; }})) return false;
        view = p;
        return true;
    }
    // frees one block early (false: not held)
    bool release(void* p) {
        for (size_t i = n_; i-- > 0;)
            if (e_[i].p == p) {
                const Entry e = e_[i];
                for (size_t j = i + 1; j < n_; ++j) e_[j - 1] = e_[j];
                --n_;
                drop(e);
                return true;
            }
        return false;
    }
    // the all-or-nothing group: rollback frees everything adopted since the mark, newest first
    size_t mark() const { return n_; }
    void rollback(size_t mark) { while (n_ > mark) drop(e_[--n_]); }
    void release_all() { rollback(0); }   // reverse order of adoption; twice is harmless
    size_t size() const { return n_; }

    void* (*grow)(void*, size_t) = std::realloc;   // (the stand-alone check lets it fail)

private:
    struct Entry { void* p; BlockKind kind; void* view; void (*null_view)(void*); };
    bool grow_to(size_t cap) {
        void* q = cap ? grow(e_, cap * sizeof(Entry)) : nullptr;
        if (!q) return false;
        e_ = static_cast<Entry*>(q);
        cap_ = cap;
        return true;
    }
    bool adopt_entry(const Entry& e) {
        if (n_ == cap_ && !grow_to(cap_ ? 2 * cap_ : 16)) { release_(e.kind, e.p); return false; }
        e_[n_++] = e;
        g_owned_blocks_live.fetch_add(1, std::memory_order_relaxed);
        return true;
    }
    void drop(const Entry& e) {
        if (e.view) e.null_view(e.view);
        release_(e.kind, e.p);
        g_owned_blocks_live.fetch_sub(1, std::memory_order_relaxed);
    }
    BlockRelease release_;
    Entry* e_ = nullptr;
    size_t n_ = 0, cap_ = 0;
};

// THE way a block comes to life: alloc() gives the pointer (null: failed), the ledger adopts it, the view is written.  False:
// nothing is held and the view is null
template <class T, class Alloc> bool own_block(OwnedBlocks& l, BlockKind kind, T*& view, Alloc&& alloc) {
    view = nullptr;
    void* p = alloc();
    return p && l.adopt(kind, static_cast<T*>(p), view);
}

// blocks that live or die together (a lazily allocated group, the four timing events): unless keep is set, every exit frees what
// was adopted since the guard was made and nulls its views -- a later call starts from a clean state
struct BlockGroup {
    OwnedBlocks& l;
    size_t mark;
    bool keep = false;
    explicit BlockGroup(OwnedBlocks& l_) : l(l_), mark(l_.mark()) {}
    ~BlockGroup() { if (!keep) l.rollback(mark); }
};

// a temporary: adopted like any block, released at the end of the scope whichever exit is taken
template <class T> struct ScopedBlock {
    OwnedBlocks& l;
    T* p = nullptr;
    explicit ScopedBlock(OwnedBlocks& l_) : l(l_) {}
    ~ScopedBlock() { if (p) l.release(p); }
};

}  // namespace m3
