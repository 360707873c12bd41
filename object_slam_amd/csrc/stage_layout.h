// Layout of the fields inside one staging block (a StagePair's pinned half and its device mirror, or a pinned download block) of the host-pointer entry
// points and of the driver's operator table.  A field's element type and count are stated ONCE, in add<T>(count); its offset, the memcpy into the pinned
// block, the typed device pointer and the memcpy out all follow from the Field that add returns.  Pure host arithmetic: no HIP, no runtime call, and it
// owns nothing (device_buffer.h owns the blocks).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace oslam {

template <class T> struct Field {
    size_t off, bytes;
    bool present;
    size_t end() const { return off + bytes; }
};

// Every field starts on a 256-byte boundary and advances the cursor by its size rounded up to 256; a field of zero bytes (n == 0, or an optional array
// the caller left out: present = false) takes no room and shares its offset with the next field.
class StageLayout {
public:
    template <class T> Field<T> add(size_t count, bool present = true) {
        const Field<T> f{total_, present ? count * sizeof(T) : 0, present};
        total_ += (f.bytes + 255) / 256 * 256;
        return f;
    }
    size_t total() const { return total_; }   // the block's size, and the offset the next field would get
private:
    size_t total_ = 0;
};

// host array -> pinned block, pinned block -> host array (both skip an empty field, whose array may be NULL)
template <class T> void put(const Field<T>& f, uint8_t* host_base, const T* src) { if (f.bytes) memcpy(host_base + f.off, src, f.bytes); }
template <class T> void get(const Field<T>& f, const uint8_t* host_base, T* dst) { if (f.bytes) memcpy(dst, host_base + f.off, f.bytes); }
// the field inside the block at `base` (the device mirror, or the pinned block for a partial copy-back); NULL for an optional array that is absent
template <class T> T* at(const Field<T>& f, uint8_t* base) { return f.present ? reinterpret_cast<T*>(base + f.off) : nullptr; }
// row b of a field laid out as rows of `stride` elements (slot-major: one row per slot, a job fills the row of its slot); NULL for an absent field
template <class T> T* row(const Field<T>& f, uint8_t* base, size_t stride, size_t b) { return f.present ? at(f, base) + stride * b : nullptr; }
// n elements between a host array and a part of a field in a pinned block (a row, a job's share of a packed field), either way: both sides have the
// field's element type and the length in bytes follows from it
template <class T> void copy_elems(T* dst, const T* src, size_t n) { if (n) memcpy(dst, src, n * sizeof(T)); }

}  // namespace oslam
