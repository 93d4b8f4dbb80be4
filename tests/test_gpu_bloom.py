"""GPU tests of the exposure Bloom filter on the device (csrc/bloom.hip: pg_bloom_exists_dev, pg_bloom_filter_dev,
pg_bloom_add_dev, the slot calls and the one-request entries) against tests/bloom_ref.py: rows, counts, sources and masks exactly,
scores and planes as bit patterns, slot contents byte for byte through pg_bloom_slot_read.  The grid is tests/bloom_cases.py's
(the CPU test runs the host statements over the same cases); the cases only a device has room for — m = 2^32 - 1, forty slots of
2^30 bits — are here.  Every output buffer carries a guard region behind it."""
import numpy as np
import pytest

import bloom_cases as cases
import bloom_ref as ref
import pairec_amd as pa
import trim_ref
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

GUARD = 256
NO = ref.NO_SLOT


class Guarded:
    """device buffers with a guard behind every one: outputs are pre-filled, so an element the kernel skips shows as well"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def put(self, a):
        if a is None:
            return 0
        p = self.ctx.to_device(np.ascontiguousarray(a))
        self.bufs.append((p, None, 0))
        return p

    def out(self, a):
        if a is None:
            return 0
        p = self.ctx.malloc(a.nbytes + GUARD)
        self.ctx.h2d(p, np.full(a.nbytes + GUARD, 0xA5, np.uint8))
        self.bufs.append((p, a, a.nbytes))
        return p

    def fetch(self):
        self.ctx.synchronize()
        for p, a, nbytes in self.bufs:
            if a is None:
                continue
            raw = np.empty(nbytes + GUARD, np.uint8)
            self.ctx.d2h(raw, p)
            assert np.all(raw[nbytes:] == 0xA5), "a write behind an output"
            a.reshape(-1).view(np.uint8)[:] = raw[:nbytes]

    def free(self):
        for p, _, _ in self.bufs:
            self.ctx.free(p)


def empty_outs(lists):
    rows, score, source, count, p64, mask, p32 = lists
    nq, cap = rows.shape
    return [np.empty((nq, cap), np.uint64), np.empty((nq, cap), np.float64), None if source is None else np.empty((nq, cap), np.uint8),
            None if p64 is None else np.empty(p64.shape, np.float64), None if mask is None else np.empty((nq, cap), np.uint32),
            None if p32 is None else np.empty(p32.shape, np.float32), np.empty(nq, np.uint32)]


def filter_dev(ctx, g, b, keys, d_in, lists, d_slots):
    """one pg_bloom_filter_dev launch over uploaded lists → its (unfetched) outputs"""
    rows, score, source, count, p64, mask, p32 = lists
    nq, cap = rows.shape
    outs = empty_outs(lists)
    d_out = [g.out(a) for a in outs]
    ctx.bloom_filter_dev(b, keys, nq, cap, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], 0 if p64 is None else p64.shape[0], d_in[5], d_in[6],
                         0 if p32 is None else p32.shape[0], d_slots, *d_out)
    return tuple(outs)


@pytest.mark.parametrize("case", cases.GRID, ids=cases.IDS)
def test_grid(ctx, case):
    c = case.build()
    want_bs, want_ex, want_flt = c.expected()
    keys = pa.BloomKeys(ctx, c.keys)
    b = pa.Bloom(ctx, c.m, c.k, c.n_slots, c.seeds)
    g = Guarded(ctx)
    try:
        assert b.info() == {"m": c.m, "k": c.k, "n_slots": c.n_slots, "slot_bytes": (ref.nbytes(c.m) + 255) // 256 * 256}
        for s in range(c.n_slots):                                       # zeroed at creation
            assert not b.slot_read(s).any()
        d_slots = g.put(c.slots)
        ctx.bloom_add_dev(b, keys, c.nq, c.cap, g.put(c.add_lists[0]), g.put(c.add_lists[3]), d_slots)
        ctx.synchronize()
        for s in range(c.n_slots):                                       # the written slots and their neighbours, byte for byte
            assert np.array_equal(b.slot_read(s), want_bs[s]), s
        d_in = [g.put(a) for a in c.lists]
        ex = np.empty((c.nq, c.cap), np.uint8)
        ctx.bloom_exists_dev(b, keys, c.nq, c.cap, d_in[0], d_in[3], d_slots, g.out(ex))
        flt = filter_dev(ctx, g, b, keys, d_in, c.lists, d_slots)
        # users without history, named either way: the real entries come out bit for bit as they went in
        plain = [filter_dev(ctx, g, b, keys, d_in, c.lists, g.put(np.full(c.nq, s, np.uint32))) for s in (NO, c.n_slots, c.n_slots + 9)]
        g.fetch()
        assert np.array_equal(ex, want_ex), np.argwhere(ex != want_ex)[:4].tolist()
        trim_ref.same(flt, want_flt)
        for p in plain:
            trim_ref.same(p, ref.dimcap_ref.compact(ref.dimcap_ref.live_mask(c.lists[0], c.lists[3]), *c.lists))
        for s in range(c.n_slots):                                       # neither Exists nor the filter writes a slot
            assert np.array_equal(b.slot_read(s), want_bs[s]), s
        # the host-array entries are the same calls
        assert np.array_equal(ctx.bloom_exists(b, keys, c.lists[0], c.slots, c.lists[3]), want_ex)
        if c.cap <= 1025:
            trim_ref.same(ctx.bloom_filter(b, keys, c.slots, *c.lists), want_flt)
    finally:
        g.free()
        b.free()
        keys.free()


def test_stream_order(ctx):
    """add, filter, add, filter on one stream, one synchronise at the end: each filter sees exactly the adds enqueued before it"""
    rng = np.random.default_rng(5)
    m, k, nq, cap, S = 18706, 4, 3, 1025, 2500
    store = cases.key_store(rng, S)
    locs = ref.locations(store, m, k)
    slots = np.array([0, 1, 0], np.uint32)
    lists = cases.lists_of(rng, nq, cap, S, "some", True)
    adds = [cases.lists_of(rng, nq, cap, S, "none", True) for _ in range(2)]
    keys, b = pa.BloomKeys(ctx, store), pa.Bloom(ctx, m, k, 2)
    g = Guarded(ctx)
    try:
        d_in, d_slots = [g.put(a) for a in lists], g.put(slots)
        d_add = [(g.put(a[0]), g.put(a[3])) for a in adds]
        got = []
        for d_rows, d_count in d_add:
            ctx.bloom_add_dev(b, keys, nq, cap, d_rows, d_count, d_slots)
            got.append(filter_dev(ctx, g, b, keys, d_in, lists, d_slots))
        g.fetch()
        bs = ref.new_bitsets(m, 2)
        for a, out in zip(adds, got):
            ref.add(locs, 2, bs, a[0], slots, a[3])
            trim_ref.same(out, ref.bloom_filter(locs, 2, bs, slots, *lists))
        assert np.any(got[0][6] > got[1][6])                             # the second add took something away
        assert np.array_equal(b.slot_read(0), bs[0]) and np.array_equal(b.slot_read(1), bs[1])
    finally:
        g.free()
        b.free()
        keys.free()


def test_the_references_test_shape_on_the_device(ctx):
    """bloom_test.go:46-70 at m = 18 706, k = 4, end to end: the decimal keys built by the library, the add and Exists on the device"""
    m, k = pa.bloom_estimate(3000, 0.05)
    ids = list(range(10000000, 10003000)) + list(range(20000000, 20003000))
    keys, b = pa.BloomKeys(ctx, ids=ids), pa.Bloom(ctx, m, k, 1)
    try:
        rows = np.arange(6000, dtype=np.uint64)[None, :]
        slots = np.zeros(1, np.uint32)
        ctx.bloom_add(b, keys, rows[:, :3000], slots)
        got = ctx.bloom_exists(b, keys, rows, slots)
        locs = ref.locations(ref.decimal_keys(ids), m, k)
        bs = ref.new_bitsets(m, 1)
        ref.add(locs, 1, bs, rows[:, :3000], slots)
        assert np.array_equal(got, ref.exists(locs, 1, bs, rows, slots)) and np.array_equal(b.slot_read(0), bs[0])
        assert got[0, :3000].all() and int(got[0, 3000:].sum()) == 137
        o_r, o_s, o_src, cnt = ctx.bloom_filter_one(b, keys, rows[0], np.arange(6000, dtype=np.float64), 0)
        assert cnt == 3000 - 137 and o_src is None and np.array_equal(o_r[:cnt], rows[0, 3000:][got[0, 3000:] == 0])
        assert np.array_equal(o_s[:cnt], o_r[:cnt].astype(np.float64)) and np.all(o_r[cnt:] == cases.U64MAX)
    finally:
        b.free()
        keys.free()


@pytest.mark.parametrize("m", (1, 7, 8, 9, 33, 2049, 18706))
def test_redis_upload(ctx, m):
    """a slot written from the restatement's Redis bytes answers as the slot the device added to, and the two read back the same;
    a write ignores the bits at or above m and zeroes what it does not bring"""
    rng = np.random.default_rng(m)
    k, S, cap = 4, 400, 300
    store = cases.key_store(rng, S)
    locs = ref.locations(store, m, k)
    keys, b = pa.BloomKeys(ctx, store), pa.Bloom(ctx, m, k, 4)
    try:
        seen = rng.integers(0, S, (1, cap)).astype(np.uint64)
        bs = ref.new_bitsets(m, 4)
        ref.add(locs, 4, bs, seen, [1])
        b.slot_write(2, bs[1])
        ctx.bloom_add(b, keys, seen, np.array([1], np.uint32))
        assert np.array_equal(b.slot_read(1), bs[1]) and np.array_equal(b.slot_read(2), bs[1])
        assert not b.slot_read(0).any() and not b.slot_read(3).any()
        rows = np.arange(S + 20, dtype=np.uint64)[None, :].repeat(2, axis=0)
        got = ctx.bloom_exists(b, keys, rows, np.array([1, 2], np.uint32))
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[0:1], ref.exists(locs, 4, bs, rows[0:1], [1]))
        # all ones in: the bits of the bitset out; a shorter write zeroes the rest; a clear zeroes all
        ones = np.full(ref.nbytes(m), 0xFF, np.uint8)
        b.slot_write(0, ones)
        assert np.array_equal(b.slot_read(0), ref.masked_write(m, ones))
        assert np.array_equal(b.slot_read(1), bs[1])                      # the neighbour stays
        b.slot_write(0, ones[:ref.nbytes(m) // 2])
        assert np.array_equal(b.slot_read(0), ref.masked_write(m, ones[:ref.nbytes(m) // 2]))
        assert np.array_equal(b.slot_read(0, 1), ref.masked_write(m, ones[:ref.nbytes(m) // 2])[:1])
        b.slot_write(3, ones)
        b.slot_clear(3)
        assert not b.slot_read(3).any() and np.array_equal(b.slot_read(2), bs[1])
    finally:
        b.free()
        keys.free()


def test_largest_m(ctx):
    """m = 2^32 - 1: the last word of a 512 MiB slot, the 32-bit modulo"""
    m, k, S, cap = (1 << 32) - 1, 7, 500, 257
    rng = np.random.default_rng(32)
    store = cases.key_store(rng, S)
    locs = ref.locations(store, m, k, cases.EXPLICIT_SEEDS[:k])
    assert int(locs.max()) > (1 << 31)                                   # (locations in the upper half: a signed index would show)
    keys, b = pa.BloomKeys(ctx, store), pa.Bloom(ctx, m, k, 1, cases.EXPLICIT_SEEDS[:k])
    try:
        lists = cases.lists_of(rng, 2, cap, S, "none", True)
        add = cases.lists_of(rng, 2, cap, S, "none", False)
        slots = np.array([0, NO], np.uint32)
        bs = {0: np.zeros(ref.nbytes(m), np.uint8)}
        # the last bit of the bitset, written from the host, then the device's adds beside it
        last = np.zeros(ref.nbytes(m), np.uint8)
        last[-1] = 0xFF
        b.slot_write(0, last)
        bs[0][-1] = 0xFE
        ctx.bloom_add(b, keys, add[0], slots)
        ref.add(locs, 1, bs, add[0], slots)
        assert np.array_equal(b.slot_read(0), bs[0])
        assert np.array_equal(ctx.bloom_exists(b, keys, lists[0], slots, lists[3]), ref.exists(locs, 1, bs, lists[0], slots, lists[3]))
        trim_ref.same(ctx.bloom_filter(b, keys, slots, *lists), ref.bloom_filter(locs, 1, bs, slots, *lists))
    finally:
        b.free()
        keys.free()


def test_slot_offsets_past_4_gib(ctx):
    """forty slots of 2^30 bits: slot 31's offset is 31 * 128 MiB, slot 39's passes 4 GiB"""
    m, k, n_slots, S, cap = 1 << 30, 4, 40, 500, 300
    rng = np.random.default_rng(40)
    store = cases.key_store(rng, S)
    locs = ref.locations(store, m, k)
    keys, b = pa.BloomKeys(ctx, store), pa.Bloom(ctx, m, k, n_slots)
    try:
        assert b.info()["slot_bytes"] * 39 > (1 << 32)
        slots = np.array([0, 31, 39, 40], np.uint32)
        add = cases.lists_of(rng, 4, cap, S, "none", True)
        lists = cases.lists_of(rng, 4, cap, S, "some", False)
        bs = {s: np.zeros(ref.nbytes(m), np.uint8) for s in (0, 31, 39)}
        ctx.bloom_add(b, keys, add[0], slots, add[3])
        ref.add(locs, n_slots, bs, add[0], slots, add[3])
        for s in (0, 31, 39):
            assert np.array_equal(b.slot_read(s), bs[s]), s
        for s in (1, 30, 32, 38):                                        # the neighbours
            assert not b.slot_read(s).any(), s
        assert np.array_equal(ctx.bloom_exists(b, keys, lists[0], slots), ref.exists(locs, n_slots, bs, lists[0], slots))
        trim_ref.same(ctx.bloom_filter(b, keys, slots, *lists), ref.bloom_filter(locs, n_slots, bs, slots, *lists))
    finally:
        b.free()
        keys.free()


def test_one_request_entries(ctx):
    rng = np.random.default_rng(9)
    m, k, S = 2049, 7, 700
    store = cases.key_store(rng, S)
    locs = ref.locations(store, m, k)
    keys, b = pa.BloomKeys(ctx, store), pa.Bloom(ctx, m, k, 3)
    try:
        bs = ref.new_bitsets(m, 3)
        for n in (1, 64, 700, 2049, 16384):
            rows = rng.integers(0, S + 30, n).astype(np.uint64)
            rows[rng.random(n) < 0.05] = cases.U64MAX
            score, source = rng.standard_normal(n), rng.integers(0, 8, n).astype(np.uint8)
            seen = rng.integers(0, S + 30, max(1, n // 50)).astype(np.uint64)
            ctx.bloom_add_one(b, keys, seen, 1)
            ref.add(locs, 3, bs, seen[None, :], [1])
            assert np.array_equal(b.slot_read(1), bs[1]) and not b.slot_read(0).any() and not b.slot_read(2).any()
            for slot in (1, 0, NO, 3):
                assert np.array_equal(ctx.bloom_exists_one(b, keys, rows, slot), ref.exists(locs, 3, bs, rows[None, :], [slot])[0])
                want = ref.bloom_filter(locs, 3, bs, [slot], rows[None, :], score[None, :], source[None, :])
                o_r, o_s, o_src, cnt = ctx.bloom_filter_one(b, keys, rows, score, slot, source)
                assert cnt == want[6][0] and np.array_equal(o_r, want[0][0]) and np.array_equal(o_s.view(np.uint64), want[1][0].view(np.uint64))
                assert np.array_equal(o_src, want[2][0])
            o_r2, o_s2, none, cnt2 = ctx.bloom_filter_one(b, keys, rows, score, 1)
            assert none is None and cnt2 == ref.bloom_filter(locs, 3, bs, [1], rows[None, :], score[None, :])[6][0]
        o_r, o_s, o_src, cnt = ctx.bloom_filter_one(b, keys, np.zeros(0, np.uint64), np.zeros(0), 1)
        assert cnt == 0 and o_r.size == 0 and o_src is None
        assert ctx.bloom_exists_one(b, keys, np.zeros(0, np.uint64), 1).size == 0
        ctx.bloom_add_one(b, keys, np.zeros(0, np.uint64), 1)
        # a store with no keys at all, and one of empty keys only
        for empty in (pa.BloomKeys(ctx, []), pa.BloomKeys(ctx, [b"", b""])):
            try:
                rows = np.array([0, 1, 5], np.uint64)
                elocs = ref.locations([b""] * empty.rows, m, k) if empty.rows else np.zeros((0, k), np.int64)
                assert np.array_equal(ctx.bloom_exists_one(b, empty, rows, 1), ref.exists(elocs, 3, bs, rows[None, :], [1])[0])
            finally:
                empty.free()
    finally:
        b.free()
        keys.free()


def test_refusals_launch_nothing(ctx):
    rng = np.random.default_rng(1)
    m, k, S, nq, cap = 2049, 4, 100, 2, 16
    store = cases.key_store(rng, S)
    keys, b = pa.BloomKeys(ctx, store), pa.Bloom(ctx, m, k, 2)
    lists = (rng.integers(0, S, (nq, cap)).astype(np.uint64), rng.standard_normal((nq, cap)), rng.integers(0, 8, (nq, cap)).astype(np.uint8),
             None, rng.standard_normal((2, nq, cap)), None, None)
    outs = empty_outs(lists)
    g = Guarded(ctx)
    who = "pg_bloom_filter_dev: "
    try:
        d_in = [g.put(a) for a in lists]
        d_out = [g.out(a) for a in outs]
        d_slots = g.put(np.array([0, 1], np.uint32))

        def call(nq=nq, cap=cap, **kw):
            a = dict(d_rows=d_in[0], d_score=d_in[1], d_source=d_in[2], d_count=0, d_planes_f64=d_in[4], n_f64=2, d_source_mask=0, d_planes_f32=0,
                     n_f32=0, d_slots=d_slots, d_out_rows=d_out[0], d_out_score=d_out[1], d_out_source=d_out[2], d_out_planes_f64=d_out[3],
                     d_out_source_mask=0, d_out_planes_f32=0, d_out_count=d_out[6])
            a.update(kw)
            ctx.bloom_filter_dev(b, keys, nq, cap, **a)

        for kw, code, text in ((dict(d_rows=0), -1, "NULL argument"), (dict(d_out_count=0), -1, "NULL argument"),
                               (dict(nq=0), -1, "nq=0 must be in [1,256]"), (dict(nq=257), -1, "nq=257 must be in [1,256]"),
                               (dict(cap=0), -4, "cap=0 unsupported (1..16384)"), (dict(cap=16385), -4, "cap=16385 unsupported (1..16384)"),
                               (dict(d_slots=0), -1, "d_slots is needed (PG_BLOOM_NO_SLOT for a user without history)"),
                               (dict(d_out_source=0), -1, "d_source / d_source_mask and their outputs come in pairs"),
                               (dict(d_out_planes_f64=0), -1, "a carried plane set and its output come in pairs"),
                               (dict(n_f64=9), -1, "a carried plane set holds 1..8 planes"),
                               (dict(d_out_rows=d_in[0] + 64), -1, "an output overlaps its input"),
                               (dict(d_out_planes_f64=d_in[4] + 8 * nq * cap), -1, "an output overlaps its input"),
                               (dict(cap=0, d_out_source=0), -4, "cap=0 unsupported (1..16384)")):
            with pytest.raises(PgError) as ei:
                call(**kw)
            assert ei.value.code == code and str(ei.value).endswith(who + text), (kw, str(ei.value))
        for fn, args in ((ctx.bloom_exists_dev, (d_in[0], 0, d_slots, d_out[2])), (ctx.bloom_add_dev, (d_in[0], 0, d_slots))):
            for shape, code in (((257, 16), -1), ((0, 16), -1), ((2, 0), -4), ((2, 16385), -4)):
                with pytest.raises(PgError) as ei:
                    fn(b, keys, *shape, *args)
                assert ei.value.code == code
        # the slot calls name their slot on the host
        for f in (lambda: b.slot_write(2, np.zeros(4, np.uint8)), lambda: b.slot_read(2), lambda: b.slot_clear(2),
                  lambda: b.slot_write(0, np.zeros(ref.nbytes(m) + 1, np.uint8)), lambda: b.slot_read(0, ref.nbytes(m) + 1)):
            with pytest.raises(PgError) as ei:
                f()
            assert ei.value.code == -1
        # the objects' own limits
        for mk in ((0, 4), (1 << 32, 4), (64, 0), (64, 17)):
            with pytest.raises(PgError) as ei:
                pa.Bloom(ctx, mk[0], mk[1], 1)
            assert ei.value.code == -1
        with pytest.raises(PgError) as ei:
            pa.Bloom(ctx, 64, 4, 0)
        assert ei.value.code == -1
        with pytest.raises(PgError) as ei:
            pa.BloomKeys(ctx, [b"a" * 64, b"b" * 65])
        assert ei.value.code == -4 and "the key of row 1 is 65 bytes (at most 64)" in str(ei.value)
        # nothing was launched: every output byte and every guard is what it was, both slots are empty
        ctx.synchronize()
        for p, a, nbytes in g.bufs:
            if a is not None:
                raw = np.empty(nbytes + GUARD, np.uint8)
                ctx.d2h(raw, p)
                assert np.all(raw == 0xA5)
        assert not b.slot_read(0).any() and not b.slot_read(1).any()
        call()                                                           # the context still serves
        g.fetch()
        trim_ref.same(tuple(outs), ref.dimcap_ref.compact(ref.dimcap_ref.live_mask(lists[0], None), *lists))
    finally:
        g.free()
        b.free()
        keys.free()
