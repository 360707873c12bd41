// Ownership of device and pinned-host memory for the handles of the library: every hipMalloc / hipHostMalloc / hipFree / hipHostFree of csrc/ is in this file
// (but for the process-wide trace buffer of lba.hip).  A handle holds these as members and `delete h` releases them; nothing with static storage duration may
// own memory through them (a destructor must not call the runtime at process exit).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/oslam_hip.h"

namespace oslam {

void set_error(const char* fmt, ...);

// A pointer and its capacity in bytes, freed by the destructor.  Non-copyable; the two concrete types below are movable, so std::swap works on them.
// Nothing here waits for the device: a caller that may have work in flight on the block waits for it — in its own way — before it lets the block go.
class Block {
public:
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
    void* ptr() const { return p_; }
    template <class T> T* as() const { return static_cast<T*>(p_); }
    uint8_t* bytes() const { return as<uint8_t>(); }
    size_t cap() const { return cap_; }
    void release() {
        if (p_) (void)(pinned_ ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; cap_ = 0;
    }
    // Frees the block and allocates `bytes` anew: contents are lost.
    int alloc(size_t bytes) { return alloc_flags(bytes, 0); }
    // Grow-only: one compare while `need` fits, otherwise alloc(ncap) — the caller chooses the new capacity (the growth policies differ by site on purpose).
    int reserve(size_t need, size_t ncap) { return need <= cap_ ? OSLAM_OK : alloc(ncap); }
    int grow(size_t need, size_t slack) { return reserve(need, need + need / 2 + slack); }   // the usual policy: half as much again plus `slack` bytes

protected:
    explicit Block(bool pinned) : pinned_(pinned) {}
    ~Block() { release(); }
    void* detach() { void* p = p_; p_ = nullptr; cap_ = 0; return p; }
    void take(Block& o) { release(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }   // (o is of the same concrete type)
    int alloc_flags(size_t bytes, unsigned host_flags) {
        release();
        const hipError_t e = pinned_ ? hipHostMalloc(&p_, bytes, host_flags) : hipMalloc(&p_, bytes);
        if (e != hipSuccess) {
            p_ = nullptr;
            set_error("%s(%zu) failed: %s", pinned_ ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
            return OSLAM_E_HIP;
        }
        cap_ = bytes;
        return OSLAM_OK;
    }

private:
    void* p_ = nullptr;
    size_t cap_ = 0;
    const bool pinned_;
};

struct DeviceBuffer : Block {
    DeviceBuffer() : Block(false) {}
    DeviceBuffer(DeviceBuffer&& o) noexcept : Block(false) { take(o); }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { if (this != &o) take(o); return *this; }
private:
    friend class DeviceBlocks;   // (takes blocks over with detach())
};

struct PinnedBuffer : Block {
    PinnedBuffer() : Block(true) {}
    PinnedBuffer(PinnedBuffer&& o) noexcept : Block(true) { take(o); }
    PinnedBuffer& operator=(PinnedBuffer&& o) noexcept { if (this != &o) take(o); return *this; }
    int alloc_mapped(size_t bytes) { return alloc_flags(bytes, hipHostMallocMapped); }
};

// A pinned block mirrored by a device block of the same size: fill `h`, ONE host-to-device copy, kernels read `d`.
struct StagePair {
    PinnedBuffer h;
    DeviceBuffer d;
    size_t cap() const { return d.cap(); }
    int reserve(size_t need, size_t ncap) {
        if (need <= cap()) return OSLAM_OK;
        h.release(); d.release();
        const int rc = h.alloc(ncap);
        return rc ? rc : d.alloc(ncap);
    }
    int grow(size_t need, size_t slack) { return reserve(need, need + need / 2 + slack); }
};

// Device blocks whose addresses are uploaded to the device as ONE table: data() is a contiguous array of raw pointers, the blocks belong to this object.
class DeviceBlocks {
public:
    DeviceBlocks() = default;
    DeviceBlocks(const DeviceBlocks&) = delete;
    DeviceBlocks& operator=(const DeviceBlocks&) = delete;
    ~DeviceBlocks() { for (uint8_t* p : v_) if (p) (void)hipFree(p); }
    size_t size() const { return v_.size(); }
    void resize(size_t n) { v_.resize(n, nullptr); }   // (grows only)
    uint8_t* operator[](size_t i) const { return v_[i]; }
    uint8_t* const* data() const { return v_.data(); }
    void push_back(DeviceBuffer&& b) { v_.push_back(nullptr); put(v_.size() - 1, std::move(b)); }
    void put(size_t i, DeviceBuffer&& b) {   // entry i becomes b's block; the block it held is freed
        if (v_[i]) (void)hipFree(v_[i]);
        v_[i] = static_cast<uint8_t*>(b.detach());
    }
private:
    std::vector<uint8_t*> v_;
};

}  // namespace oslam
