// seq_arena.h — where the driver's per-sequence maps (slam_map.h) keep their small blocks: the observation lists of the map points, the point table and
// the dense per-point arrays.
//
// Two levels.  SlabPool (one per process) maps 2 MiB-aligned anonymous slabs, asks for transparent huge pages on them (madvise(MADV_HUGEPAGE); a refusal is
// not an error, OSLAM_MAP_HUGEPAGES=0 skips the request) and hands out fixed chunks under a mutex that is entered once per chunk.  SeqArena (one per Map)
// carves blocks out of its chunks: bump allocation plus one free list per size class, and NO lock — a sequence is only ever touched by one thread at a time
// (every host stage is a parallel_for over sequences).  A sequence's blocks so lie in its own chunks instead of being interleaved with the blocks of thousands
// of other sequences by the allocator's per-thread arenas, carry no allocator header, and freeing one never takes a lock another worker may hold.
// A reset or destroyed arena gives its chunks back to the pool's free list; nothing is unmapped during a run (page faults of memory given back and taken
// again cost more than the memory is worth).
//
// -DOSLAM_ARENA_PASSTHROUGH forwards every block to malloc / free (each with its exact size) so that a sanitizer build sees block bounds.
// Product code: never includes oracle/.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <type_traits>

#ifndef OSLAM_ARENA_PASSTHROUGH
#include <sys/mman.h>
#endif

#ifndef OSLAM_ARENA_CHUNK_KB
#define OSLAM_ARENA_CHUNK_KB 16   // chunk-tail waste is bounded by one chunk per sequence: 16 KiB x 8192 sequences = 0.13 GB per rank (resident with huge pages)
#endif

namespace oslam_drv {

constexpr size_t kArenaChunk = (size_t)OSLAM_ARENA_CHUNK_KB << 10;
constexpr size_t kArenaSlab = (size_t)64 << 20;       // one mmap = 64 MiB = 32 huge pages
constexpr size_t kArenaHuge = (size_t)2 << 20;
constexpr size_t kArenaChunkHead = 64;                // a chunk's first line holds its link; blocks start behind it

struct ArenaChunk { ArenaChunk* next; };

struct SlabPoolStats { size_t slabs, chunks_carved, chunks_free, madvise_failed; bool hugepages; };

#ifndef OSLAM_ARENA_PASSTHROUGH
class SlabPool {
public:
    static SlabPool& instance() { static SlabPool p; return p; }
    ArenaChunk* take() {
        std::lock_guard<std::mutex> g(mu_);
        if (free_) { ArenaChunk* c = free_; free_ = c->next; nFree_--; return c; }
        if (cur_ == end_) {
            // over-map by one huge page and cut the region to 2 MiB alignment
            char* raw = (char*)mmap(nullptr, kArenaSlab + kArenaHuge, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
            if (raw == (char*)MAP_FAILED) throw std::bad_alloc();
            char* al = (char*)(((uintptr_t)raw + kArenaHuge - 1) & ~(uintptr_t)(kArenaHuge - 1));
            if (al > raw) munmap(raw, (size_t)(al - raw));
            if (al + kArenaSlab < raw + kArenaSlab + kArenaHuge) munmap(al + kArenaSlab, (size_t)(raw + kArenaHuge - al));
            if (huge_ && madvise(al, kArenaSlab, MADV_HUGEPAGE) != 0) nMadvFail_++;
            cur_ = al; end_ = al + kArenaSlab; nSlabs_++;
        }
        ArenaChunk* c = (ArenaChunk*)cur_;
        cur_ += kArenaChunk; nCarved_++;
        return c;
    }
    void give(ArenaChunk* head, ArenaChunk* tail, size_t n) {   // a linked run of n chunks
        std::lock_guard<std::mutex> g(mu_);
        tail->next = free_; free_ = head; nFree_ += n;
    }
    SlabPoolStats stats() {
        std::lock_guard<std::mutex> g(mu_);
        return SlabPoolStats{nSlabs_, nCarved_, nFree_, nMadvFail_, huge_};
    }
private:
    SlabPool() { const char* e = getenv("OSLAM_MAP_HUGEPAGES"); huge_ = !(e && e[0] == '0'); }
    std::mutex mu_;
    ArenaChunk* free_ = nullptr;
    char *cur_ = nullptr, *end_ = nullptr;
    size_t nSlabs_ = 0, nCarved_ = 0, nFree_ = 0, nMadvFail_ = 0;
    bool huge_ = true;
};
#endif

class SeqArena {
public:
    // Size classes, in units of 16 bytes: 1, 2, 3, 4, 6, 8, 12, 16, ... (powers of two and 1.5 x powers of two: an observation list of capacity 2^k is
    // 24 * 2^k bytes = the class 3 * 2^(k-1) exactly).  Blocks of 1 KiB and more start on a cache line.
    static constexpr int kClasses = 24;
    static size_t class_units(int c) { return c == 0 ? 1 : (c & 1) ? (size_t)1 << ((c + 1) / 2) : (size_t)3 << (c / 2 - 1); }
    static size_t class_bytes(int c) { return class_units(c) << 4; }
    static int class_of(size_t bytes) {
        const size_t u = (bytes + 15) >> 4;
        if (u <= 1) return 0;
        const int p = 63 - __builtin_clzll((unsigned long long)u);
        if (u == (size_t)1 << p) return 2 * p - 1;
        if (u <= (size_t)3 << (p - 1)) return 2 * p;
        return 2 * p + 1;
    }
    static constexpr size_t kMaxSmall = kArenaChunk / 2;   // larger blocks (none in practice) are tracked malloc blocks

    SeqArena() = default;
    SeqArena(const SeqArena&) = delete;
    SeqArena& operator=(const SeqArena&) = delete;
    SeqArena(SeqArena&& o) noexcept { steal(o); }
    SeqArena& operator=(SeqArena&& o) noexcept { if (this != &o) { release(); steal(o); } return *this; }
    ~SeqArena() { release(); }

    void* alloc(size_t bytes) {
#ifndef OSLAM_ARENA_PASSTHROUGH
        if (bytes <= kMaxSmall) {
            const int c = class_of(bytes);
            if (free_[c]) { void* p = free_[c]; free_[c] = *(void**)p; return p; }
            const size_t sz = class_bytes(c);
            if (void* p = bump(sz)) return p;
            // the current chunk is used up: the front of a larger free block (the tail of an earlier chunk, a list a point outgrew), the rest stays free
            for (int c2 = c + 1; c2 < kClasses; c2++)
                if (free_[c2]) {
                    char* b = (char*)free_[c2]; free_[c2] = *(void**)b;
                    recycle(b + sz, b + class_bytes(c2));
                    return b;
                }
            if (cur_) recycle(cur_, end_);
            ArenaChunk* ch = SlabPool::instance().take();
            ch->next = chunks_; chunks_ = ch; nChunks_++;
            if (!lastChunk_) lastChunk_ = ch;
            cur_ = (char*)ch + kArenaChunkHead; end_ = (char*)ch + kArenaChunk;
            return bump(sz);
        }
#endif
        return tracked_alloc(bytes);
    }
    void dealloc(void* p, size_t bytes) {   // bytes = what alloc was asked for
        if (!p) return;
#ifndef OSLAM_ARENA_PASSTHROUGH
        if (bytes <= kMaxSmall) { const int c = class_of(bytes); *(void**)p = free_[c]; free_[c] = p; return; }
#endif
        (void)bytes;
        tracked_free(p);
    }
    // every block is gone afterwards: the chunks go back to the pool
    void release() {
        while (big_) tracked_free((char*)big_ + sizeof(Big));
#ifndef OSLAM_ARENA_PASSTHROUGH
        if (chunks_) SlabPool::instance().give(chunks_, lastChunk_, nChunks_);
        chunks_ = lastChunk_ = nullptr; nChunks_ = 0; cur_ = end_ = nullptr;
        memset(free_, 0, sizeof(free_));
#endif
    }
    size_t chunks_held() const { return nChunks_; }

private:
    struct alignas(64) Big { Big *prev, *next; };   // header of a tracked malloc block (one line: the block behind it starts on a line as well)
    void* tracked_alloc(size_t bytes) {
        void* raw = nullptr;
        if (posix_memalign(&raw, 64, sizeof(Big) + bytes) != 0) throw std::bad_alloc();
        Big* b = (Big*)raw;
        b->prev = nullptr; b->next = big_;
        if (big_) big_->prev = b;
        big_ = b;
        return (char*)b + sizeof(Big);
    }
    void tracked_free(void* p) {
        Big* b = (Big*)((char*)p - sizeof(Big));
        if (b->prev) b->prev->next = b->next; else big_ = b->next;
        if (b->next) b->next->prev = b->prev;
        free(b);
    }
    void steal(SeqArena& o) {
        big_ = o.big_; o.big_ = nullptr;
        chunks_ = o.chunks_; lastChunk_ = o.lastChunk_; nChunks_ = o.nChunks_; cur_ = o.cur_; end_ = o.end_;
        memcpy(free_, o.free_, sizeof(free_));
        o.chunks_ = o.lastChunk_ = nullptr; o.nChunks_ = 0; o.cur_ = o.end_ = nullptr;
        memset(o.free_, 0, sizeof(o.free_));
    }
#ifndef OSLAM_ARENA_PASSTHROUGH
    void* bump(size_t sz) {
        if (!cur_) return nullptr;
        char* p = cur_;
        if (sz >= 1024) p = (char*)(((uintptr_t)p + 63) & ~(uintptr_t)63);
        if (p + sz > end_) return nullptr;
        if (p != cur_) recycle(cur_, p);
        cur_ = p + sz;
        return p;
    }
    // [b, e) (16-byte aligned, inside one chunk) will not be bumped over: cut it into free blocks, largest class first
    void recycle(char* b, char* e) {
        while (e - b >= 16) {
            size_t rem = (size_t)(e - b);
            if (rem > kMaxSmall) rem = kMaxSmall;
            int c = class_of(rem);
            if (class_bytes(c) > rem) c--;
            const size_t mis = (uintptr_t)b & 63;
            if (class_bytes(c) >= 1024 && mis) c = class_of(64 - mis);   // 16, 32 or 48 bytes up to the next line: exact classes
            *(void**)b = free_[c]; free_[c] = b;
            b += class_bytes(c);
        }
    }
#endif
    Big* big_ = nullptr;
    ArenaChunk *chunks_ = nullptr, *lastChunk_ = nullptr;
    size_t nChunks_ = 0;
    char *cur_ = nullptr, *end_ = nullptr;
    void* free_[kClasses] = {};
};

// Chunked array on an arena: element i lives at [i >> K][i & mask].  Growing appends a block; nothing is ever copied but the block table.  Elements are
// plain data (no constructors or destructors run); the memory belongs to the arena and goes back with it.
template <class T, int K>
struct ChunkVec {
    static_assert(std::is_trivially_copyable<T>::value && std::is_trivially_destructible<T>::value, "ChunkVec holds plain data");
    static constexpr size_t kMask = ((size_t)1 << K) - 1;
    T** blk = nullptr;
    uint32_t nblk = 0, capblk = 0;
    size_t n = 0;
    ChunkVec() = default;
    ChunkVec(const ChunkVec&) = delete;
    ChunkVec& operator=(const ChunkVec&) = delete;
    ChunkVec(ChunkVec&& o) noexcept : blk(o.blk), nblk(o.nblk), capblk(o.capblk), n(o.n) { o.blk = nullptr; o.nblk = o.capblk = 0; o.n = 0; }
    ChunkVec& operator=(ChunkVec&& o) noexcept {   // (the blocks of the overwritten array belong to its arena)
        if (this != &o) { blk = o.blk; nblk = o.nblk; capblk = o.capblk; n = o.n; o.blk = nullptr; o.nblk = o.capblk = 0; o.n = 0; }
        return *this;
    }
    T& operator[](size_t i) { return blk[i >> K][i & kMask]; }
    const T& operator[](size_t i) const { return blk[i >> K][i & kMask]; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    T& back() { return (*this)[n - 1]; }
    const T& back() const { return (*this)[n - 1]; }
    void push_back(SeqArena& a, const T& v) {
        if ((n >> K) == nblk) {
            if (nblk == capblk) {
                const uint32_t nc = capblk ? capblk * 2 : 4;
                T** nb = (T**)a.alloc(sizeof(T*) * nc);
                if (nblk) memcpy(nb, blk, sizeof(T*) * nblk);
                a.dealloc(blk, sizeof(T*) * capblk);
                blk = nb; capblk = nc;
            }
            blk[nblk++] = (T*)a.alloc(sizeof(T) << K);
        }
        memcpy(&blk[n >> K][n & kMask], &v, sizeof(T));
        n++;
    }
};

}  // namespace oslam_drv
