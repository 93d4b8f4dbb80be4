// scratch_layout.hpp — the one round-up and the carving cursor of the scratch arena (host only, no HIP dependency).
#pragma once
#include <cstddef>
#include <cstdint>

namespace pg {

// kSlotDin (rank_din.hip): candidates of one run of a PG_MODEL_DIN call.  The slot holds at most this many staged rows of
// 512 B (64 MiB) and as many identity indices, whatever the call's size.  A larger call is served in successive runs of this
// many CANDIDATES — cut by candidate index, not by request: each run has its own offsets (the call's, clamped to the run and
// rebased) and is tiled on its own, so a request that straddles a boundary is attended and ranked in both runs, each with
// the request's whole sequence and user vector, and its scores land where one run would have put them.
constexpr uint32_t kDinRunItems = 1u << 17;
// kSlotMha (rank_mha.hip): a run of a PG_MODEL_MHA call is cut the same way and also covers at most this many REQUESTS, whose
// projected keys and values (512 positions x d_att x 2 x 4 B at most each) it keeps: 128 MiB at most beside the staged rows.
constexpr uint32_t kMhaRunReqs = 256;

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
