// Stand-alone check of pairec_amd/csrc/scratch_layout.hpp (built and run by test_scratch_layout_cpu.py; host only).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "scratch_layout.hpp"

using pg::Carve;

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                   \
        }                                                                 \
    } while (0)

struct Region {
    uintptr_t p;
    size_t bytes, align;
};

// a layout with every feature a site uses: default and 64-byte alignments, packed 4-byte neighbours, regions of zero elements
// (first, in the middle, last), a raw byte region of an odd size, a wide element type
struct Wide { uint64_t a, b; };
static void layout(Carve& c, size_t n, bool optional, std::vector<Region>* out) {
    auto note = [&](const void* p, size_t bytes, size_t align) { out->push_back({(uintptr_t)p, bytes, align}); };
    note(c.take<uint32_t>(0), 0, 256);
    note(c.take<float>(n), n * 4, 256);
    note(c.take<uint8_t>(n), n, 256);
    note(c.take<uint64_t>(optional ? n : 0), optional ? n * 8 : 0, 256);
    note(c.take<uint32_t>(3, 64), 12, 64);
    note(c.take<uint32_t>(5, 64), 20, 64);
    note(c.take<uint32_t>(7, 4), 28, 4);
    note(c.take<float>(0, 64), 0, 64);
    note(c.take<float>(1, 4), 4, 4);
    note(c.bytes(3 * n + 1), 3 * n + 1, 256);
    note(c.take<Wide>(n), n * 16, 256);
    note(c.take<double>(optional ? 2 : 0), optional ? 16 : 0, 256);
}

static void check(size_t n, bool optional, uintptr_t base) {
    std::vector<Region> m, r;
    Carve measure;
    layout(measure, n, optional, &m);
    for (const Region& x : m) CHECK(x.p == 0);               // measuring hands out no pointers
    Carve carve{(char*)base};
    layout(carve, n, optional, &r);
    CHECK(carve.total() == measure.total());
    CHECK(m.size() == r.size());
    uintptr_t end = base;
    for (const Region& x : r) {
        if (x.bytes == 0) {                                  // costs nothing: the cursor did not move
            CHECK(x.p == end);
            continue;
        }
        CHECK(x.p % x.align == 0);                           // (the base is 256-aligned, as hipMalloc's)
        CHECK(x.p >= end);                                   // declaration order, no overlap
        CHECK(x.p - end < x.align);                          // no more padding than the alignment asks for
        end = x.p + x.bytes;
    }
    CHECK(measure.total() == end - base);                    // the total is the end of the last region
    // a layout without its optional regions places the others exactly as if those were never written
    if (!optional) {
        Carve c{(char*)base};
        const uintptr_t a = (uintptr_t)c.take<float>(n), b = (uintptr_t)c.take<uint8_t>(n), d = (uintptr_t)c.take<uint32_t>(3, 64);
        CHECK(a == r[1].p && b == r[2].p && d == r[4].p);
    }
}

int main() {
    CHECK(pg::align_up(0) == 0 && pg::align_up(1) == 256 && pg::align_up(256) == 256 && pg::align_up(257) == 512);
    CHECK(pg::align_up(65, 64) == 128 && pg::align_up((size_t)5 << 32 | 1, (size_t)1 << 20) == ((size_t)5 << 32) + ((size_t)1 << 20));
    for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)257, (size_t)100003})
        for (int optional = 0; optional < 2; ++optional)
            for (uintptr_t base : {(uintptr_t)0x100, (uintptr_t)0x7f0000001000ull, (uintptr_t)0x200000300ull}) check(n, optional != 0, base);
    // pointers are base + the offsets measured
    Carve m;
    m.take<double>(10);
    const size_t second = pg::align_up(m.total(), 64);
    m.take<uint32_t>(4, 64);
    Carve c{(char*)0x4000};
    CHECK((uintptr_t)c.take<double>(10) == 0x4000);
    CHECK((uintptr_t)c.take<uint32_t>(4, 64) == 0x4000 + second && second == 128);
    CHECK(c.total() == m.total() && m.total() == 144);
    if (g_failed) return 1;
    std::printf("scratch_layout OK\n");
    return 0;
}
