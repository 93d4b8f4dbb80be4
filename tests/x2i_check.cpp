// x2i_check.cpp — csrc/x2i_host.hpp alone, as a stand-alone program (tests/test_x2i_san_cpu.py builds it plain and under the address
// and undefined-behaviour sanitizers): the upload validation on hostile CSR, the argument checks, and the host statement on small
// hand-worked tables and on the GPU tests' grid.
//
//   x2i_check                 the built-in checks; prints "x2i OK"
//   x2i_check DIR             ... and the grid: reads DIR/table.bin and DIR/requests.bin (tests/x2i_cases.py write_grid), writes
//                             DIR/answers.bin — per case rows uint64[nq][k], scores double[nq][k], counts uint32[nq], status uint32
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "x2i_host.hpp"

using namespace pg;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static bool valid(uint64_t n, const std::vector<uint64_t>& off, const std::vector<uint32_t>& ids, const std::vector<float>* sc, uint64_t max_len,
                  uint64_t limit) {
    std::string err;
    // exact-size copies on the heap: a read outside [offsets[0], offsets[n]) is the sanitizer's to find
    std::vector<uint32_t> i2(ids);
    i2.shrink_to_fit();
    std::vector<float> s2;
    if (sc) s2 = *sc;
    const bool ok = x2i_validate_lists("check", "key", "id", 7, n, off.data(), i2.data(), sc ? s2.data() : nullptr, max_len, limit, &err);
    CHECK(ok == err.empty());
    return ok;
}

static void hostile_csr() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> one3{1.0f, 1.0f, 1.0f};
    CHECK(valid(2, {0, 2, 3}, {1, 2, 0}, nullptr, 64, 3));
    CHECK(valid(2, {0, 2, 3}, {1, 2, 0}, &one3, 1024, 3));
    CHECK(valid(0, {5}, {}, nullptr, 64, 3));
    CHECK(valid(3, {1, 1, 1, 1}, {9}, nullptr, 64, 3));                 // empty lists: the id outside them is never read
    CHECK(!valid(2, {0, 3, 2}, {1, 2, 0}, nullptr, 64, 3));             // offsets that descend
    CHECK(!valid(2, {3, 0, 3}, {1, 2, 0}, nullptr, 64, 3));
    CHECK(!valid(2, {0, 2, ~0ull}, {1, 2}, nullptr, 64, 3));            // a list that would run to the end of memory: refused by its length
    CHECK(!valid(2, {~0ull - 1, ~0ull, 1}, {1, 2}, nullptr, 64, 3));    // offsets that wrap
    CHECK(!valid(2, {0, 2, 3}, {1, 3, 0}, nullptr, 64, 3));             // an id out of range
    CHECK(!valid(2, {0, 2, 3}, {1, 0xFFFFFFFFu, 0}, nullptr, 64, 3));
    CHECK(!valid(2, {0, 3, 3}, {1, 2, 1}, nullptr, 64, 3));             // an id twice in one list
    CHECK(valid(2, {0, 2, 3}, {1, 2, 1}, nullptr, 64, 3));              // ... across lists it is served
    std::vector<float> bad{1.0f, inf, 1.0f}, bad2{nan, 1.0f, 1.0f}, bad3{1.0f, 1.0f, -inf};
    CHECK(!valid(2, {0, 2, 3}, {1, 2, 0}, &bad, 1024, 3));
    CHECK(!valid(2, {0, 2, 3}, {1, 2, 0}, &bad2, 1024, 3));
    CHECK(!valid(2, {0, 2, 3}, {1, 2, 0}, &bad3, 1024, 3));
    // maximal lists
    std::vector<uint32_t> ids(1025);
    for (uint32_t i = 0; i < 1025; ++i) ids[i] = 1024 - i;
    std::vector<float> sc(1025, 0.5f);
    CHECK(valid(1, {0, 64}, std::vector<uint32_t>(ids.begin(), ids.begin() + 64), nullptr, kX2iMaxXPerItem, 2000));
    CHECK(!valid(1, {0, 65}, std::vector<uint32_t>(ids.begin(), ids.begin() + 65), nullptr, kX2iMaxXPerItem, 2000));
    std::vector<float> sc1024(sc.begin(), sc.begin() + 1024);
    CHECK(valid(1, {0, 1024}, std::vector<uint32_t>(ids.begin(), ids.begin() + 1024), &sc1024, kX2iMaxList, 2000));
    CHECK(!valid(1, {0, 1025}, ids, &sc, kX2iMaxList, 2000));
    CHECK(valid(1, {1, 1025}, ids, &sc, kX2iMaxList, 2000));            // offsets index the call's arrays from offsets[0]
}

static void arguments() {
    std::string err;
    uint32_t nmax = 0;
    uint32_t off[3] = {0, 1, 2}, trig[2] = {0, 1};
    double pref[2] = {1.0, 2.0}, out_s[4] = {};
    uint64_t out_r[4] = {};
    CHECK(x2i_check_args("c", trig, pref, off, 2, 2, nullptr, out_r, out_s, false, true, &nmax, &err) == PG_OK && nmax == 0);
    CHECK(x2i_check_args("c", trig, pref, nullptr, 2, 2, nullptr, out_r, out_s, false, true, &nmax, &err) == PG_ERR_INVALID);
    CHECK(x2i_check_args("c", trig, pref, off, 0, 2, nullptr, out_r, out_s, false, true, &nmax, &err) == PG_ERR_INVALID);
    CHECK(x2i_check_args("c", trig, pref, off, 257, 2, nullptr, out_r, out_s, false, true, &nmax, &err) == PG_ERR_INVALID);
    CHECK(x2i_check_args("c", trig, pref, off, 2, 0, nullptr, out_r, out_s, false, true, &nmax, &err) == PG_ERR_UNSUPPORTED);
    CHECK(x2i_check_args("c", trig, pref, off, 2, 16385, nullptr, out_r, out_s, false, true, &nmax, &err) == PG_ERR_UNSUPPORTED);
    uint32_t desc[3] = {2, 1, 2}, many[2] = {0, 257};
    CHECK(x2i_check_args("c", trig, pref, desc, 2, 2, nullptr, out_r, out_s, false, true, &nmax, &err) == PG_ERR_INVALID);
    CHECK(x2i_check_args("c", trig, pref, many, 1, 2, nullptr, out_r, out_s, false, false, &nmax, &err) == PG_ERR_UNSUPPORTED);
    pref[1] = std::numeric_limits<double>::infinity();
    CHECK(x2i_check_args("c", trig, pref, off, 2, 2, nullptr, out_r, out_s, false, true, &nmax, &err) == PG_ERR_INVALID);
    CHECK(x2i_check_args("c", trig, pref, off, 2, 2, nullptr, out_r, out_s, false, false, &nmax, &err) == PG_OK);   // device memory: a precondition
    pref[1] = 2.0;
    uint32_t xo[3] = {0, 4096, 4097}, xbig[3] = {0, 4097, 4097};
    std::vector<uint64_t> ex(4097, 5);
    pg_x2i_opts o{1, 0, ex.data(), xo};
    CHECK(x2i_check_args("c", trig, pref, off, 2, 16384 - 4096, &o, out_r, out_s, false, true, &nmax, &err) == PG_OK && nmax == 4096);
    CHECK(x2i_check_args("c", trig, pref, off, 2, 16384 - 4095, &o, out_r, out_s, false, true, &nmax, &err) == PG_ERR_UNSUPPORTED);
    o.excl_offsets = xbig;
    CHECK(x2i_check_args("c", trig, pref, off, 2, 2, &o, out_r, out_s, false, true, &nmax, &err) == PG_ERR_UNSUPPORTED);
    o.excl_offsets = nullptr;
    CHECK(x2i_check_args("c", trig, pref, off, 2, 2, &o, out_r, out_s, false, true, &nmax, &err) == PG_ERR_INVALID);   // rows without offsets
    CHECK(x2i_check_args("c", nullptr, nullptr, nullptr, 2, 2, nullptr, out_r, out_s, true, false, &nmax, &err) == PG_OK);
}

// the hand-worked example of tests/test_x2i_cpu.py: four triggers (prefer 2, 1, 3, 1), three X (A = 2, B = 0, C = 1)
static void hand_worked() {
    const uint64_t rows = 20;
    std::vector<uint64_t> io(rows + 1, 6);
    io[0] = 0, io[1] = 1, io[2] = 3, io[3] = 5;
    const uint32_t ii[6] = {2, 2, 0, 0, 1, 1};
    const uint64_t xo[4] = {0, 2, 5, 8};                                 // B, C, A by id
    const uint32_t xr[8] = {11, 12, 10, 3, 13, 10, 0, 11};
    const float xs[8] = {0.25f, 1.0f, 0.5f, 2.0f, 0.25f, 0.5f, 1.0f, 1.0f};
    const uint32_t trig[4] = {0, 1, 2, 3}, off[2] = {0, 4};
    const double pref[4] = {2.0, 1.0, 3.0, 1.0};
    uint64_t r[6];
    double s[6];
    uint32_t c;
    CHECK(x2i_recall_host(rows, 1000, 3, io.data(), ii, xo, xr, xs, trig, pref, off, 1, 6, nullptr, r, s, &c) == kX2iNone);
    CHECK(c == 4 && r[0] == 1011 && r[1] == 1012 && r[2] == 1010 && r[3] == 1013 && r[4] == ~0ull && r[5] == ~0ull);
    CHECK(s[0] == 1.0 && s[1] == 1.0 && s[2] == 0.875 && s[3] == 0.25 && s[4] == -std::numeric_limits<double>::infinity());
    pg_x2i_opts o{1, 1, nullptr, nullptr};
    CHECK(x2i_recall_host(rows, 1000, 3, io.data(), ii, xo, xr, xs, trig, pref, off, 1, 3, &o, r, s, &c) == kX2iNone);
    CHECK(c == 3 && r[0] == 1012 && r[1] == 1011 && r[2] == 1010 && s[0] == 4.0 && s[1] == 3.0 && s[2] == 2.0);
    const uint64_t ex[3] = {1011, 5, 1000};
    const uint32_t exo[2] = {0, 3};
    pg_x2i_opts o2{1, 0, ex, exo};
    CHECK(x2i_recall_host(rows, 1000, 3, io.data(), ii, xo, xr, xs, trig, pref, off, 1, 2, &o2, r, s, nullptr) == kX2iNone);
    CHECK(r[0] == 1012 && r[1] == 1010);
    // a non-finite X sum is dropped; nothing but trigger items answers 0
    const double huge[4] = {1e308, 1e308, 0.0, 0.0};
    const uint32_t off2[2] = {0, 2};
    CHECK(x2i_recall_host(rows, 0, 3, io.data(), ii, xo, xr, xs, trig, huge, off2, 1, 6, nullptr, r, s, &c) == kX2iNone);
    CHECK(c == 2 && r[0] == 12 && r[1] == 11 && s[0] == 1.0 && s[1] == 0.25);   // A = inf is gone, B = 1e308 stays
}

// more than kX2iMaxX distinct X, more than kX2iMaxPairs pairs: reported, the other requests answered
static void limits() {
    const uint32_t n_x = 1200;
    const uint64_t rows = 2000;
    std::vector<uint64_t> io(rows + 1), xo(n_x + 1);
    std::vector<uint32_t> ii, xr;
    std::vector<float> xs;
    for (uint64_t r = 0; r < rows; ++r) {                                // rows 0 .. 17 name 64 X each, the others none
        io[r] = ii.size();
        if (r < 18)
            for (uint32_t j = 0; j < 64; ++j) ii.push_back((uint32_t)(r * 64 + j));
    }
    io[rows] = ii.size();
    for (uint32_t x = 0; x < n_x; ++x) {                                 // X 0 .. 63 list 1024 items, X 64 one, the others two
        xo[x] = xr.size();
        const uint32_t len = x < 64 ? 1024 : x == 64 ? 1 : 2;
        for (uint32_t j = 0; j < len; ++j) {
            xr.push_back(100 + (x * 7 + j) % 1900);
            xs.push_back(1.0f);
        }
    }
    xo[n_x] = xr.size();
    std::string err;
    CHECK(x2i_validate_lists("c", "row", "x id", 0, rows, io.data(), ii.data(), nullptr, kX2iMaxXPerItem, n_x, &err));
    CHECK(x2i_validate_lists("c", "X", "item row", 0, n_x, xo.data(), xr.data(), xs.data(), kX2iMaxList, rows, &err));
    std::vector<uint32_t> trig;
    std::vector<double> pref;
    std::vector<uint32_t> off{0};
    auto request = [&](uint32_t first, uint32_t n) {
        for (uint32_t i = 0; i < n; ++i) {
            trig.push_back(first + i);
            pref.push_back(1.0 + i);
        }
        off.push_back((uint32_t)trig.size());
    };
    request(0, 1);          // 64 X of 1024: 65536 pairs, served
    request(0, 2);          // more pairs
    request(1, 16);         // 1024 distinct X, served
    request(1, 17);         // 1088 distinct X
    request(0, 17);         // both limits: the X limit is tested first
    const uint32_t nq = 5, k = 8;
    std::vector<uint64_t> r(nq * k);
    std::vector<double> s(nq * k);
    uint32_t c[nq];
    const uint32_t st = x2i_recall_host(rows, 0, n_x, io.data(), ii.data(), xo.data(), xr.data(), xs.data(), trig.data(), pref.data(), off.data(),
                                        nq, k, nullptr, r.data(), s.data(), c);
    CHECK(st == 1 * 2 + 1);
    CHECK(c[0] == 8 && c[1] == 0 && c[2] == 8 && c[3] == 0 && c[4] == 0 && r[1 * k] == ~0ull);
    CHECK(x2i_limit_message("w", st).find("request 1 ") != std::string::npos);
    // the last two requests as a batch of their own: request 0 of it is beyond the X limit
    const uint32_t st2 = x2i_recall_host(rows, 0, n_x, io.data(), ii.data(), xo.data(), xr.data(), xs.data(), trig.data(), pref.data(),
                                         off.data() + 3, 2, k, nullptr, r.data(), s.data(), c);
    CHECK(st2 == 0 && c[0] == 0 && c[1] == 0);
    CHECK(x2i_limit_message("w", st2).find("distinct X") != std::string::npos);
}

template <class T>
static std::vector<T> read_vec(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        printf("FAILED: short read\n");
        exit(2);
    }
    return v;
}

static void grid(const std::string& dir) {
    FILE* f = fopen((dir + "/table.bin").c_str(), "rb");
    FILE* rq = fopen((dir + "/requests.bin").c_str(), "rb");
    FILE* out = fopen((dir + "/answers.bin").c_str(), "wb");
    if (!f || !rq || !out) {
        printf("FAILED: cannot open the grid's files in %s\n", dir.c_str());
        exit(2);
    }
    const auto head = read_vec<uint64_t>(f, 3);
    const uint64_t rows = head[0], row_offset = head[1];
    const uint32_t n_x = (uint32_t)head[2];
    const auto io = read_vec<uint64_t>(f, rows + 1);
    const auto xo = read_vec<uint64_t>(f, (size_t)n_x + 1);
    const auto ii = read_vec<uint32_t>(f, io[rows]);
    const auto xr = read_vec<uint32_t>(f, xo[n_x]);
    const auto xs = read_vec<float>(f, xo[n_x]);
    fclose(f);
    std::string err;
    CHECK(x2i_validate_lists("grid", "row", "x id", 0, rows, io.data(), ii.data(), nullptr, kX2iMaxXPerItem, n_x, &err));
    CHECK(x2i_validate_lists("grid", "X", "item row", 0, n_x, xo.data(), xr.data(), xs.data(), kX2iMaxList, rows, &err));
    uint32_t h[5];
    int ncases = 0;
    while (fread(h, 4, 5, rq) == 5) {
        const uint32_t nq = h[0], k = h[1];
        const auto off = read_vec<uint32_t>(rq, (size_t)nq + 1);
        const auto trig = read_vec<uint32_t>(rq, h[4]);
        const auto pref = read_vec<double>(rq, h[4]);
        pg_x2i_opts o{(int)h[2], (int)h[3], nullptr, nullptr};
        uint32_t nmax;
        CHECK(x2i_check_args("grid", trig.data(), pref.data(), off.data(), nq, k, &o, &nmax, &nmax, false, true, &nmax, &err) == PG_OK);
        std::vector<uint64_t> r((size_t)nq * k);
        std::vector<double> s((size_t)nq * k);
        std::vector<uint32_t> c(nq);
        const uint32_t st = x2i_recall_host(rows, row_offset, n_x, io.data(), ii.data(), xo.data(), xr.data(), xs.data(), trig.data(), pref.data(),
                                            off.data(), nq, k, &o, r.data(), s.data(), c.data());
        fwrite(r.data(), 8, r.size(), out);
        fwrite(s.data(), 8, s.size(), out);
        fwrite(c.data(), 4, c.size(), out);
        fwrite(&st, 4, 1, out);
        ++ncases;
    }
    fclose(rq);
    fclose(out);
    CHECK(ncases > 0);
    printf("grid: %d cases\n", ncases);
}

int main(int argc, char** argv) {
    hostile_csr();
    arguments();
    hand_worked();
    limits();
    if (argc > 1) grid(argv[1]);
    if (failures) {
        printf("%d checks FAILED\n", failures);
        return 1;
    }
    printf("x2i OK\n");
    return 0;
}
