// scratch_layout.hpp — the one round-up and the carving cursor of the scratch arena (host only, no HIP dependency).
#pragma once
#include <cstddef>

namespace pg {

// x rounded up to a multiple of a (a power of two); 256 bytes is the arena's default region alignment
inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) & ~(a - 1); }

// One statement of a buffer's regions gives both its size and its pointers: a site writes its layout once, as a function of a
// Carve, and runs it twice.  With no base the cursor only measures (take returns nullptr, total() is the bytes to reserve);
// with a base the same calls return the regions, in the order taken, each at its alignment.  A region of zero elements takes
// no bytes and moves nothing (its pointer is where the cursor stands, not to be read).  Arrays that a copy or a kernel spans
// together are taken as ONE region and split by the site, never as neighbours: a neighbour may start after padding.
struct Carve {
    char* base = nullptr;
    size_t off = 0;
    template <class T>
    T* take(size_t count, size_t align = 256) {
        if (count) off = align_up(off, align);
        T* p = base ? (T*)(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
    void* bytes(size_t n, size_t align = 256) { return take<char>(n, align); }      // exactly n bytes (blocks a kernel strides by their size)
    size_t total() const { return off; }
};

}  // namespace pg
