"""CPU tests of the exposure Bloom filter (csrc/bloom_host.hpp behind pg_bloom_*_host, pg_bloom_estimate and
pg_bloom_murmur3_host) against tests/bloom_ref.py: the public murmur3_x86_32 vectors, EstimateParameters, the reference's own test
shape, the host statements on the GPU tests' grid, Redis's byte order, and what the entry points refuse.  No GPU needed."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import bloom_cases as cases
import bloom_ref as ref
import pairec_amd as pa
import trim_ref
from pairec_amd import _lib
from pairec_amd._lib import PgError

HERE = os.path.dirname(os.path.abspath(__file__))

MURMUR_VECTORS = [(b"", 0, 0), (b"", 1, 0x514E28B7), (b"", 0xFFFFFFFF, 0x81F16F39), (b"test", 0, 0xBA6BD213),
                  (b"Hello, world!", 0, 0xC0363E43), (b"The quick brown fox jumps over the lazy dog", 0x9747B28C, 0x2FA826CD)]


def test_murmur_vectors():
    for key, seed, want in MURMUR_VECTORS:
        assert ref.murmur3(key, seed) == want, (key, seed)
        assert pa.bloom_murmur3_host(key, seed) == want, (key, seed)
        arr = np.frombuffer(key, np.uint8).reshape(1, len(key))
        assert int(ref.murmur3_same_length(arr, seed)[0]) == want
    rng = np.random.default_rng(3)
    for L in range(0, 70):                                              # every block count and tail, at seeds of both ends
        key = rng.integers(0, 256, L).astype(np.uint8).tobytes()
        for seed in (0, 2, 0xFFFFFFFF, int(rng.integers(0, 1 << 32))):
            assert pa.bloom_murmur3_host(key, seed) == ref.murmur3(key, seed), (L, seed)


def test_seed_zero_is_the_mirrors_hash32():
    """the seed-0 hash is the one the host mirror's hash32 pins (tests/golden/reference_known_answers.json: normalizer_test.go's
    murmur3.Sum32(key) % 100 cases, evaluated there by tests/test_feature_normalizer.py's own murmur3_32)"""
    from test_feature_normalizer import murmur3_32
    with open(os.path.join(HERE, "golden", "reference_known_answers.json")) as f:
        text = json.load(f)
    keys = set()

    def walk(x):
        if isinstance(x, dict):
            if x.get("expect_fn") == "murmur3_32_mod_100":
                keys.add(x["value"]["key"])
            for v in x.values():
                walk(v)
        elif isinstance(x, list):
            for v in x:
                walk(v)
    walk(text)
    assert keys
    for key in sorted(keys) + ["", "a", "test"]:
        assert pa.bloom_murmur3_host(key.encode(), 0) == murmur3_32(key.encode()) == ref.murmur3(key.encode(), 0), key


@pytest.mark.parametrize("n,p,m,k", [(1000000, 0.05, 6235225, 4), (4096, 0.01, 39261, 7), (3000, 0.05, 18706, 4)])
def test_estimates(n, p, m, k):
    assert pa.bloom_estimate(n, p) == (m, k) == ref.estimate(n, p)


def test_estimate_refuses():
    for n, p in ((0, 0.05), (10, 0.0), (10, 1.0), (10, -1.0), (10, float("nan"))):
        with pytest.raises(PgError) as ei:
            pa.bloom_estimate(n, p)
        assert ei.value.code == -1 and "pg_bloom_estimate: " in str(ei.value)
    L = _lib.load()
    assert L.pg_bloom_estimate(10, 0.5, None, None) == -1


def test_the_references_test_shape():
    """bloom_test.go:46-70 at m = 18 706, k = 4: every added string exists; of the second range the restatement flags 137"""
    m, k = pa.bloom_estimate(3000, 0.05)
    assert (m, k) == (18706, 4)
    keys = ref.decimal_keys(range(10000000, 10003000)) + ref.decimal_keys(range(20000000, 20003000))
    off, data = pa.bloom_pack_keys(keys)
    locs = ref.locations(keys, m, k)
    rows = np.arange(6000, dtype=np.uint64)[None, :]
    slots = np.zeros(1, np.uint32)
    bs, want_bs = ref.new_bitsets(m, 1), ref.new_bitsets(m, 1)
    pa.bloom_add_host(m, k, None, bs, off, data, rows[:, :3000], slots)
    ref.add(locs, 1, want_bs, rows[:, :3000], slots)
    assert np.array_equal(bs, want_bs)
    got = pa.bloom_exists_host(m, k, None, bs, off, data, rows, slots)
    want = ref.exists(locs, 1, want_bs, rows, slots)
    assert np.array_equal(got, want)
    assert got[0, :3000].all()
    flagged = int(got[0, 3000:].sum())
    assert 0.01 * 3000 <= flagged <= 0.20 * 3000                        # (a filter that keeps everything, or drops everything, fails here)
    assert flagged == 137


@pytest.mark.parametrize("case", cases.GRID, ids=cases.IDS)
def test_host_statement_on_the_grid(case):
    c = case.build()
    want_bs, want_ex, want_flt = c.expected()
    off, data = pa.bloom_pack_keys(c.keys)
    bs = ref.new_bitsets(c.m, c.n_slots)
    pa.bloom_add_host(c.m, c.k, c.seeds, bs, off, data, c.add_lists[0], c.slots, c.add_lists[3])
    assert np.array_equal(bs, want_bs)
    assert not bs[[0, 2, 4]].any()                                       # the written slots' neighbours
    assert np.array_equal(pa.bloom_exists_host(c.m, c.k, c.seeds, bs, off, data, c.lists[0], c.slots, c.lists[3]), want_ex)
    trim_ref.same(pa.bloom_filter_host(c.m, c.k, c.seeds, bs, off, data, c.slots, *c.lists), want_flt)
    # a user without history: the real entries come out bit for bit as they went in
    none = np.full(c.nq, ref.NO_SLOT, np.uint32)
    plain = pa.bloom_filter_host(c.m, c.k, c.seeds, bs, off, data, none, *c.lists)
    trim_ref.same(plain, ref.dimcap_ref.compact(ref.dimcap_ref.live_mask(c.lists[0], c.lists[3]), *c.lists))
    if c.m >= 18706 and c.cap >= 255:                                   # (the case means something: some are seen, some are not)
        live = ref.dimcap_ref.live_mask(c.lists[0], c.lists[3])
        assert 0 < int(want_ex.sum()) < int(live.sum())


def test_redis_byte_order():
    """bit 0 is 0x80 of byte 0; bit m - 1 lands in the last byte; a write ignores the bits at or above m"""
    for m in (1, 7, 8, 9, 31, 32, 33, 2049):
        keys = [b"x"]
        off, data = pa.bloom_pack_keys(keys)
        bs = ref.new_bitsets(m, 2)
        loc = int(ref.locations(keys, m, 1, [5])[0, 0])
        pa.bloom_add_host(m, 1, [5], bs, off, data, np.zeros((1, 1), np.uint64), np.array([1], np.uint32))
        want = np.zeros(ref.nbytes(m), np.uint8)
        want[loc >> 3] = 0x80 >> (loc & 7)
        assert np.array_equal(bs[1], want) and not bs[0].any(), m
        # the write: all ones in, the bits of the bitset out
        pa.bloom_slot_write_host(m, bs, 0, np.full(ref.nbytes(m), 0xFF, np.uint8))
        assert np.array_equal(bs[0], ref.masked_write(m, np.full(ref.nbytes(m), 0xFF, np.uint8))), m
        assert bs[0, 0] & 0x80 and bs[0, -1] & (0x80 >> ((m - 1) & 7)), m
        assert bs[0, -1] == ((0xFF00 >> (m % 8)) & 0xFF if m % 8 else 0xFF), m
        # a short write zeroes the rest
        pa.bloom_slot_write_host(m, bs, 0, np.zeros(0, np.uint8))
        assert not bs[0].any()
    m = 18706
    one = np.zeros(ref.nbytes(m), np.uint8)
    ref.set_bits(one, [0, m - 1])
    assert one[0] == 0x80 and one[-1] == 0x80 >> ((m - 1) & 7) and int(one.astype(np.int64).sum()) == one[0] + one[-1]


def test_argument_checks():
    L = _lib.load()
    keys = [b"abc", b"", b"defgh"]
    off, data = pa.bloom_pack_keys(keys)
    rows = np.zeros((1, 4), np.uint64)
    slots = np.zeros(1, np.uint32)
    bs = ref.new_bitsets(64, 2)
    out = np.zeros((1, 4), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                       # noqa: E731

    def exists(m=64, k=4, n_slots=2, bitsets=bs, key_rows=3, o=off, d=data, nq=1, cap=4, r=rows, sl=slots, out_=out):
        v = lambda a: None if a is None else p(a)                                    # noqa: E731
        rc = L.pg_bloom_exists_host(m, k, None, n_slots, v(bitsets), key_rows, v(o), v(d), nq, cap, v(r), None, v(sl), v(out_))
        return rc, L.pg_last_error().decode()

    assert exists() == (0, exists()[1])
    for kw, code, text in ((dict(o=None), -1, "NULL argument"), (dict(r=None), -1, "NULL argument"), (dict(sl=None), -1, "NULL argument"),
                           (dict(out_=None), -1, "NULL argument"), (dict(bitsets=None), -1, "NULL argument"),
                           (dict(m=0), -1, "m=0 must be in [1, 2^32 - 1]"), (dict(m=1 << 32), -1, "m=4294967296 must be in [1, 2^32 - 1]"),
                           (dict(k=0), -1, "k=0 must be in [1, 16]"), (dict(k=17), -1, "k=17 must be in [1, 16]"),
                           (dict(nq=0), -1, "nq=0 must be in [1,256]"), (dict(nq=257), -1, "nq=257 must be in [1,256]"),
                           (dict(cap=0), -4, "cap=0 unsupported (1..16384)"), (dict(cap=16385), -4, "cap=16385 unsupported (1..16384)")):
        rc, msg = exists(**kw)
        assert rc == code and msg == "pg_bloom_exists_host: " + text, (kw, rc, msg)
    # a 65-byte key; a 64-byte one is served
    long_off, long_data = pa.bloom_pack_keys([b"a" * 64, b"b" * 65])
    rc, msg = exists(key_rows=2, o=long_off, d=long_data)
    assert rc == -4 and msg == "pg_bloom_exists_host: the key of row 1 is 65 bytes (at most 64)"
    assert exists(key_rows=1, o=long_off, d=long_data)[0] == 0
    # offsets that descend
    bad = np.array([0, 5, 3, 8], np.uint64)
    rc, msg = exists(o=bad)
    assert rc == -1 and msg == "pg_bloom_exists_host: offsets descend at row 1"
    # the same refusals by the add and the filter
    assert L.pg_bloom_add_host(64, 17, None, 2, p(bs), 3, p(off), p(data), 1, 4, p(rows), None, p(slots)) == -1
    assert L.pg_last_error() == b"pg_bloom_add_host: k=17 must be in [1, 16]"
    assert L.pg_bloom_add_host(64, 4, None, 2, p(bs), 3, p(bad), p(data), 1, 4, p(rows), None, p(slots)) == -1
    assert not bs.any()
    with pytest.raises(PgError) as ei:
        pa.bloom_filter_host(0, 4, None, bs, off, data, slots, rows, np.zeros((1, 4)))
    assert ei.value.code == -1 and str(ei.value).endswith("pg_bloom_filter_host: m=0 must be in [1, 2^32 - 1]")
    with pytest.raises(PgError) as ei:
        pa.bloom_filter_host(64, 4, None, bs, long_off, long_data, slots, rows, np.zeros((1, 4)))
    assert ei.value.code == -4
    # a slot >= n_slots named on the host is refused; on the lists it is a user without history
    with pytest.raises(PgError) as ei:
        pa.bloom_slot_write_host(64, bs, 2, np.zeros(8, np.uint8))
    assert ei.value.code == -1 and str(ei.value).endswith("pg_bloom_slot_write_host: slot 2 of 2")
    with pytest.raises(PgError) as ei:
        pa.bloom_slot_write_host(64, bs, 0, np.zeros(9, np.uint8))
    assert ei.value.code == -1 and str(ei.value).endswith("pg_bloom_slot_write_host: 9 bytes for a bitset of 8")
    pa.bloom_add_host(64, 4, None, bs, off, data, rows, np.array([2], np.uint32))
    assert not bs.any()
    # the device entries refuse NULL before they touch a device
    assert L.pg_bloom_create(None, 64, 4, None, 1, None) == -1
    assert L.pg_bloom_keys_create(None, 0, None, None, None) == -1
    assert L.pg_bloom_keys_create_decimal(None, 0, None, None) == -1
    assert L.pg_bloom_filter_dev(*([None] * 3), 1, 4, *([None] * 5), 0, None, None, 0, *([None] * 8)) == -1
    assert L.pg_last_error() == b"pg_bloom_filter_dev: NULL argument"
    for fn, n in ((L.pg_bloom_exists_dev, 4), (L.pg_bloom_add_dev, 3)):
        assert fn(None, None, None, 1, 4, *([None] * n)) == -1
    assert L.pg_bloom_slot_write(None, None, 0, None, 0) == -1 and L.pg_bloom_slot_read(None, None, 0, None, 0) == -1
    assert L.pg_bloom_slot_clear(None, None, 0) == -1 and L.pg_bloom_info(None, None, None, None, None) == -1
    assert L.pg_bloom_exists(None, None, None, 0, None, 0, None) == -1 and L.pg_bloom_add(None, None, None, 0, None, 0) == -1
    assert L.pg_bloom_filter(None, None, None, 0, None, None, None, 0, None, None, None, None) == -1
