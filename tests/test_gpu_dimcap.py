"""GPU tests of the value cap and of DistinctIdSort on the device (csrc/dimcap.hip: pg_candidates_dimcap_dev,
pg_candidates_dimcap; csrc/cond.hip: pg_distinct_ids_dev, pg_distinct_ids) against tests/dimcap_ref.py: rows, counts, sources and
masks exactly, scores and planes as bit patterns, ids exactly.  Sizes sit on the kernel's edges: a wave of 64 lanes, the chunk of
1 024 positions, the boundary between the LDS table and the scratch table, the largest cap.  A case is one launch over one request
per key pattern; its store holds the patterns' keys row by row, so the entry at position p of request q reads row q * cap + p.
Every output buffer carries a guard word behind it."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cond_ref
import dimcap_ref as ref
import fanin_ref
import pairec_amd as pa
import trim_ref
from oracle import oracle as o
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
U32MAX = 0xFFFFFFFF
I64MIN = -(1 << 63)
HUGE = np.uint64((1 << 40) + 5)               # a row far outside every store here
LDS = pa.DIMCAP_LDS_MAX_CAP
LIMITS = (1, 2, 3, U32MAX)
MODES = (pa.DIMCAP_NULL_KEEP, pa.DIMCAP_NULL_VALUE)
NV = -7                                        # the value that stands for null where has_null is set
MAXP = 8                                       # PG_TRIM_MAX_PLANES
GUARD = 256


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


def run_many(ctx, fs, lists, confs):
    """the inputs uploaded once, one launch per conf → [outputs]"""
    rows, score, source, count, p64, mask, p32 = lists
    nq, cap = rows.shape
    g = Guarded(ctx)
    try:
        d_in = [g.put(a) for a in lists]
        all_outs = []
        for conf in confs:
            outs = empty_outs(lists)
            d_out = [g.out(a) for a in outs]
            ctx.candidates_dimcap_dev(conf, fs, nq, cap, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], 0 if p64 is None else p64.shape[0], d_in[5],
                                      d_in[6], 0 if p32 is None else p32.shape[0], *d_out)
            all_outs.append(tuple(outs))
        g.fetch()
    finally:
        g.free()
    return all_outs


# ---- key patterns -------------------------------------------------------------------------------------------------------------------

PATTERNS = ("distinct", "equal", "all_outside", "all_null_value", "one_wave", "chunk_boundary", "limit_th_last_lane", "collide", "high_bits",
            "negative", "mixed", "count_zero", "count_over", "null_value_real")


def pattern_case(rng, cap, carry):
    """one request per pattern → (store keys [nq * cap] int64, lists); carry: "none" | "some" | "all" optional arrays"""
    nq = len(PATTERNS)
    p = np.arange(cap, dtype=np.int64)
    K = np.empty((nq, cap), np.int64)
    rows = (np.arange(nq, dtype=np.uint64)[:, None] * np.uint64(cap) + np.arange(cap, dtype=np.uint64)[None, :])
    S = nq * cap
    count = np.full(nq, cap, np.uint32)
    for q, name in enumerate(PATTERNS):
        k = p + 100
        if name == "equal":
            k = np.full(cap, 9, np.int64)
        elif name == "all_outside":                                      # just outside and far outside the store
            rows[q] = np.where(p % 3 == 0, HUGE, np.uint64(S) + (p % 5).astype(np.uint64))
        elif name == "all_null_value":
            k = np.full(cap, NV, np.int64)
        elif name == "one_wave":                                         # 64 equal keys inside one wave
            k[(64 if cap >= 128 else 0):(128 if cap >= 128 else cap)] = 55
        elif name == "chunk_boundary" and cap > 1024:
            k[1023], k[1024] = 77, 77
        elif name == "limit_th_last_lane":                              # the 3rd / 2nd / 1st occurrence sits on the last lane of a chunk
            for at, key in (((1021, 1022, 1023, 1024, 1030), 66), ((2046, 2047, 2048, 2050), 67), ((3071, 3072, 3080), 68)):
                for x in at:
                    if x < cap:
                        k[x] = key
        elif name == "collide":                                          # keys whose probes start at one slot, each several times
            coll = ref.colliding_keys(cap, min(cap, 40))
            k = coll[p % coll.size]
        elif name == "high_bits":
            k = ((p % 7) << 32) | 5
        elif name == "negative":
            k = np.choose(p % 4, [np.full(cap, I64MIN), np.full(cap, I64MIN + 1), np.full(cap, -1), -(p % 11) - 2]).astype(np.int64)
        elif name in ("mixed", "count_zero", "count_over"):
            k = rng.integers(0, max(2, cap // 8), cap).astype(np.int64)
            out = rng.random(cap) < 0.2
            rows[q][out] = np.where(rng.random(cap) < 0.5, HUGE, np.uint64(S) + rng.integers(0, 40, cap).astype(np.uint64))[out]
            rows[q][rng.random(cap) < 0.07] = U64MAX                     # padding rows in the middle of the list
            count[q] = {"mixed": max(1, cap - cap // 7), "count_zero": 0, "count_over": cap + 5}[name]
        elif name == "null_value_real":
            k = rng.integers(0, max(2, cap // 4), cap).astype(np.int64)
            k[rng.random(cap) < 0.3] = NV
        K[q] = k
    score = np.round(rng.standard_normal((nq, cap)), 4)
    score.view(np.uint64)[0, cap // 2] = 0x7FF8000000000123              # a NaN with a payload travels as bits
    if carry == "none":
        lists = (rows, score, None, count, None, None, None)
    else:
        n = MAXP if carry == "all" else 2
        lists = (rows, score, rng.integers(0, 8, (nq, cap)).astype(np.uint8), count, rng.standard_normal((n, nq, cap)),
                 rng.integers(0, 256, (nq, cap)).astype(np.uint32), rng.standard_normal((n, nq, cap)).astype(np.float32))
    return K.reshape(-1), lists


def keys_at(store_keys, rows):
    """the reference's view: each entry's key and whether its row is inside the store"""
    inside = rows < np.uint64(store_keys.size)
    return store_keys[np.where(inside, rows, 0).astype(np.int64)], inside.astype(np.uint8)


CAPS = (1, 63, 64, 65, 1023, 1024, 1025, LDS - 1, LDS, LDS + 1, 16384)
CARRY = {1: "all", 65: "all", 1025: "all", LDS + 1: "all", 63: "none", 1023: "none", LDS - 1: "none"}


@pytest.mark.parametrize("cap", CAPS)
def test_key_patterns_limits_and_null_modes(ctx, cap):
    rng = np.random.default_rng(cap)
    store_keys, lists = pattern_case(rng, cap, CARRY.get(cap, "some"))
    fs = pa.Features(ctx, store_keys.size)
    try:
        fs.set_column("k64", pa.F_I64, store_keys)
        fs.set_column("k32", pa.F_I32, store_keys.astype(np.int32))           # (wraps: other keys, as valid)
        keys, item_in = keys_at(store_keys, lists[0])
        keys32 = keys_at(store_keys.astype(np.int32).astype(np.int64), lists[0])[0]
        # every pattern at every limit in both null modes with has_null set; without it (the null code is then a value like
        # any other) at two limits; the int32 column at two
        confs = [("k64", limit, mode, NV) for limit in LIMITS for mode in MODES]
        confs += [("k64", limit, mode, None) for limit in (1, 2) for mode in MODES]
        confs += [("k32", limit, pa.DIMCAP_NULL_KEEP if limit == 1 else pa.DIMCAP_NULL_VALUE, NV) for limit in (1, 3)]
        got = run_many(ctx, fs, lists, confs)
        for (col, limit, mode, nv), g in zip(confs, got):
            want = ref.dimcap(keys if col == "k64" else keys32, item_in, limit, mode, nv, *lists)
            trim_ref.same(g, want)
            if col == "k64":
                n = dict(zip(PATTERNS, g[6].astype(np.int64)))
                assert n["distinct"] == cap and n["equal"] == min(limit, cap) and n["count_zero"] == 0
                assert n["all_outside"] == (cap if mode == pa.DIMCAP_NULL_KEEP else min(limit, cap))
                assert n["all_null_value"] == (min(limit, cap) if nv is None or mode == pa.DIMCAP_NULL_VALUE else cap)
                assert n["high_bits"] == min(7 * limit, cap, sum(min(limit, len(range(r, cap, 7))) for r in range(7)))
                if cap > 1024:
                    assert n["chunk_boundary"] == (cap - 1 if limit == 1 else cap)
    finally:
        fs.destroy()


def test_go_loops_on_the_patterns(ctx):
    """the kernel against the Go transcription itself, at one cap past a chunk (the array form stands in elsewhere: the CPU
    tests hold the two together)"""
    cap = 1025
    rng = np.random.default_rng(11)
    store_keys, lists = pattern_case(rng, cap, "none")
    fs = pa.Features(ctx, store_keys.size)
    try:
        fs.set_column("k64", pa.F_I64, store_keys)
        keys, item_in = keys_at(store_keys, lists[0])
        confs = [("k64", 1, pa.DIMCAP_NULL_KEEP, NV), ("k64", 1, pa.DIMCAP_NULL_KEEP, None), ("k64", 3, pa.DIMCAP_NULL_VALUE, NV),
                 ("k64", 2, pa.DIMCAP_NULL_VALUE, None)]
        for (col, limit, mode, nv), g in zip(confs, run_many(ctx, fs, lists, confs)):
            trim_ref.same(g, ref.compact(ref.keep_go(keys, item_in, lists[0], lists[3], limit, mode, nv), *lists))
    finally:
        fs.destroy()


@pytest.mark.parametrize("nq", (1, 3, 256))
def test_request_counts(ctx, nq):
    cap = 65
    rng = np.random.default_rng(nq)
    S = 500
    store_keys = rng.integers(-20, 20, S).astype(np.int64)
    rows = rng.integers(0, S + 60, (nq, cap)).astype(np.uint64)
    rows[rng.random((nq, cap)) < 0.05] = U64MAX
    count = rng.integers(0, cap + 2, nq).astype(np.uint32)
    lists = (rows, rng.standard_normal((nq, cap)), rng.integers(0, 8, (nq, cap)).astype(np.uint8), count, rng.standard_normal((MAXP, nq, cap)),
             rng.integers(0, 256, (nq, cap)).astype(np.uint32), rng.standard_normal((MAXP, nq, cap)).astype(np.float32))
    fs = pa.Features(ctx, S)
    try:
        fs.set_column("k", pa.F_I64, store_keys)
        keys, item_in = keys_at(store_keys, rows)
        confs = [("k", 1, pa.DIMCAP_NULL_KEEP, NV), ("k", 2, pa.DIMCAP_NULL_VALUE, None)]
        for (col, limit, mode, nv), g in zip(confs, run_many(ctx, fs, lists, confs)):
            trim_ref.same(g, ref.dimcap(keys, item_in, limit, mode, nv, *lists))
        # the host-array entry is the same call
        trim_ref.same(ctx.candidates_dimcap(confs[0], fs, *lists), ref.dimcap(keys, item_in, 1, pa.DIMCAP_NULL_KEEP, NV, *lists))
    finally:
        fs.destroy()


# ---- chaining and idempotence ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain(ctx):
    rng = np.random.default_rng(41)
    S = 2000
    store = {"author": rng.integers(0, 60, S).astype(np.int32), "spu": rng.integers(0, 25, S).astype(np.int64) << 33}
    fs = pa.Features(ctx, S)
    fs.set_column("author", pa.F_I32, store["author"])
    fs.set_column("spu", pa.F_I64, store["spu"])
    yield S, store, fs
    fs.destroy()


def test_fanin_then_cap_then_trim(ctx, chain):
    """pg_fanin_merge_dev → pg_candidates_dimcap_dev → pg_candidates_trim_dev: each stage takes the one before it as it is"""
    S, store, fs = chain
    rng = np.random.default_rng(31)
    nq, ks = 3, (300, 200, 120)
    src = []
    for i, k in enumerate(ks):
        rows = np.stack([rng.choice(S + 47, k, replace=False).astype(np.uint64) for _ in range(nq)])
        sc = rng.standard_normal((nq, k))
        src.append((rows, sc if i == 1 else sc.astype(np.float32)))
    m = ctx.fanin_merge(src)                                             # rows, score, source, planes, mask, count
    wm = fanin_ref.merge(src)
    conf = ("author", 2, pa.DIMCAP_NULL_KEEP, 0)
    f = ctx.candidates_dimcap(conf, fs, m[0], m[1], m[2], m[5], m[3], m[4], None)
    keys, item_in = keys_at(store["author"].astype(np.int64), wm[0])
    wf = ref.dimcap(keys, item_in, 2, pa.DIMCAP_NULL_KEEP, 0, wm[0], wm[1], wm[2], wm[5], wm[3], wm[4], None)
    trim_ref.same(f, wf)
    assert np.all(f[6] > 0) and np.all(f[6] < m[5])
    rules = [(0, pa.TRIM_FIX, 40), (1, pa.TRIM_ACCUMULATE, 90), (2, pa.TRIM_ACCUMULATE, 120)]
    t = ctx.candidates_trim(rules, f[0], f[1], f[2], f[6], f[3], f[4])
    trim_ref.same(t, trim_ref.trim(rules, wf[0], wf[1], wf[2], wf[6], wf[3], wf[4]))
    # applied to its own output the cap changes nothing
    trim_ref.same(ctx.candidates_dimcap(conf, fs, f[0], f[1], f[2], f[6], f[3], f[4], None), f)
    conf_v = ("author", 3, pa.DIMCAP_NULL_VALUE, None)
    once = ctx.candidates_dimcap(conf_v, fs, m[0], m[1], m[2], m[5], m[3], m[4], None)
    trim_ref.same(ctx.candidates_dimcap(conf_v, fs, once[0], once[1], once[2], once[6], once[3], once[4], None), once)


def test_two_columns_are_the_two_loops_in_that_order(ctx, chain):
    S, store, fs = chain
    rng = np.random.default_rng(17)
    cap = 1500
    rows = rng.integers(0, S + 30, (1, cap)).astype(np.uint64)
    score = rng.standard_normal((1, cap))

    def props(r):
        return {} if r >= S else {"author": int(store["author"][r]), "spu": int(store["spu"][r])}
    items = [{"pos": p, "properties": props(int(rows[0, p]))} for p in range(cap)]
    for first, l1, second, l2 in (("author", 4, "spu", 9), ("spu", 9, "author", 4)):
        want = ref.go_group_weight_dimension(ref.go_group_weight_dimension(items, first, l1), second, l2)
        one = ctx.candidates_dimcap((first, l1, pa.DIMCAP_NULL_VALUE, None), fs, rows, score)
        two = ctx.candidates_dimcap((second, l2, pa.DIMCAP_NULL_VALUE, None), fs, one[0], one[1], count=one[6])
        n = int(two[6][0])
        assert two[0][0, :n].tolist() == [int(rows[0, it["pos"]]) for it in want]
        assert np.array_equal(two[1][0, :n].view(np.uint64), score[0, [it["pos"] for it in want]].view(np.uint64)) and 0 < n < int(one[6][0]) < cap


def test_one_request_entry_equals_the_dev_one(ctx, chain):
    S, store, fs = chain
    rng = np.random.default_rng(77)
    for cap in (1, 700, 2049, LDS + 1):
        rows = rng.integers(0, S + 30, cap).astype(np.uint64)
        rows[rng.random(cap) < 0.05] = U64MAX
        score, source = rng.standard_normal(cap), rng.integers(0, 8, cap).astype(np.uint8)
        for conf in (("author", 1, pa.DIMCAP_NULL_KEEP, 0), ("spu", 2, pa.DIMCAP_NULL_VALUE, None)):
            dev = run_many(ctx, fs, (rows[None, :], score[None, :], source[None, :], None, None, None, None), [conf])[0]
            o_r, o_s, o_src, cnt = ctx.candidates_dimcap_one(conf, fs, rows, score, source)
            assert cnt == dev[6][0] and np.array_equal(o_r, dev[0][0]) and np.array_equal(o_s.view(np.uint64), dev[1][0].view(np.uint64))
            assert np.array_equal(o_src, dev[2][0])
            o_r2, o_s2, none, cnt2 = ctx.candidates_dimcap_one(conf, fs, rows, score)
            assert none is None and cnt2 == cnt and np.array_equal(o_r2, o_r)
    o_r, o_s, o_src, cnt = ctx.candidates_dimcap_one(("author", 1, 0, None), fs, np.zeros(0, np.uint64), np.zeros(0))
    assert cnt == 0 and o_r.size == 0 and o_s.size == 0 and o_src is None


# ---- refusals on the device side -----------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(ctx, chain):
    S, store, fs = chain
    ff = pa.Features(ctx, 16)
    ff.set_column("f", pa.F_F32, np.zeros(16, np.float32))
    rng = np.random.default_rng(1)
    nq, cap = 2, 16
    lists = (rng.integers(0, S, (nq, cap)).astype(np.uint64), rng.standard_normal((nq, cap)), rng.integers(0, 8, (nq, cap)).astype(np.uint8),
             None, rng.standard_normal((2, nq, cap)), None, None)
    outs = empty_outs(lists)
    g = Guarded(ctx)
    who = "pg_candidates_dimcap_dev: "
    try:
        d_in = [g.put(a) for a in lists]
        d_out = [g.out(a) for a in outs]

        def call(conf=("author", 1, 0, None), store=fs, nq=nq, cap=cap, **kw):
            a = dict(d_rows=d_in[0], d_score=d_in[1], d_source=d_in[2], d_count=0, d_planes_f64=d_in[4], n_f64=2, d_source_mask=0, d_planes_f32=0,
                     n_f32=0, d_out_rows=d_out[0], d_out_score=d_out[1], d_out_source=d_out[2], d_out_planes_f64=d_out[3], d_out_source_mask=0,
                     d_out_planes_f32=0, d_out_count=d_out[6])
            a.update(kw)
            ctx.candidates_dimcap_dev(conf, store, nq, cap, **a)

        for kw, code, text in ((dict(conf=("colour", 1, 0, None)), -1, 'column "colour" is not a column of the feature store'),
                               (dict(conf=("f", 1, 0, None), store=ff), -4, 'column "f" is a float column (dtype 3): the value cap serves int32 and int64 columns'),
                               (dict(conf=("author", 0, 0, None)), -1, "limit=0 keeps nothing (1 .. UINT32_MAX; 1 is DimensionFieldUniqueFilter)"),
                               (dict(cap=0), -4, "cap=0 unsupported (1..16384)"), (dict(cap=16385), -4, "cap=16385 unsupported (1..16384)"),
                               (dict(nq=257), -1, "nq=257 must be in [1,256]"),
                               (dict(d_out_rows=d_in[0] + 64), -1, "an output overlaps its input"),
                               (dict(d_out_planes_f64=d_in[4] + 8 * nq * cap), -1, "an output overlaps its input"),
                               (dict(d_out_planes_f64=0), -1, "a carried plane set and its output come in pairs")):
            with pytest.raises(PgError) as ei:
                call(**kw)
            assert ei.value.code == code and str(ei.value).endswith(who + text), (kw, str(ei.value))
        # nothing was launched: every output byte and every guard is what it was
        ctx.synchronize()
        for p, a, nbytes in g.bufs:
            if a is not None:
                raw = np.empty(nbytes + GUARD, np.uint8)
                ctx.d2h(raw, p)
                assert np.all(raw == 0xA5)
        call()                                                           # the context still serves
        g.fetch()
        keys, item_in = keys_at(store["author"].astype(np.int64), lists[0])
        trim_ref.same(tuple(outs), ref.dimcap(keys, item_in, 1, 0, None, *lists))
    finally:
        g.free()
        ff.destroy()


# ---- pg_distinct_ids_dev ---------------------------------------------------------------------------------------------------------------------

DS, DJ = 2000, 47
RULES = [
    [{"Name": "a", "Operator": "equal", "Type": "int", "Value": 3}],
    [{"Name": "b", "Operator": "greater", "Type": "float", "Value": 0.5}, {"Name": "ui", "Domain": "user", "Operator": "equal", "Type": "int", "Value": 7}],
    [{"Name": "a", "Operator": "in", "Type": "int", "Value": [1, 2, 9]}],
    [{"Name": "c", "Operator": "not_equal", "Type": "int64", "Value": "item.a"}, {"Name": "b", "Operator": "less", "Type": "float", "Value": -0.5}],
    [{"Name": "uf", "Domain": "user", "Operator": "is_not_null"}, {"Name": "a", "Operator": "equal", "Type": "int", "Value": 5}],
    [{"Operator": "bool", "Type": "or", "Configs": [{"Name": "a", "Operator": "equal", "Type": "int", "Value": 6},
                                                     {"Name": "c", "Operator": "equal", "Type": "int64", "Value": 1 << 40}]}],
    # a candidate outside the store: `a` is missing, which is_null answers with true and every comparison above with false
    [{"Name": "a", "Operator": "is_null"}, {"Name": "ui", "Domain": "user", "Operator": "is_not_null"}],
    [{"Name": "b", "Operator": "lessThan", "Type": "float", "Value": "user.uf"}],
]
IDS = [-1, 1 << 33, 5, -(1 << 40), 0, 2147483648, 77, -2]
DECL = [("a", pa.F_I32), ("b", pa.F_F64), ("c", pa.F_I64)]
USERS = [{"ui": 7, "uf": 0.25}, {"ui": 8}, {}]
assert len(RULES) == pa.COND_MAX_RULES


class World:
    pass


@pytest.fixture(scope="module")
def world(ctx):
    w = World()
    rng = np.random.default_rng(8)
    w.store = {"a": rng.integers(0, 12, DS).astype(np.int32), "b": rng.standard_normal(DS), "c": rng.choice([0, 3, 1 << 40], DS).astype(np.int64)}
    w.fs = pa.Features(ctx, DS)
    for (n, dt) in DECL:
        w.fs.set_column(n, dt, w.store[n])
    w.cond = pa.cond_compile([{"Conditions": r} for r in RULES], DECL)
    w.universe = np.concatenate([np.arange(DS + DJ, dtype=np.uint64), [HUGE]])
    cols, inside = cond_ref.gather(w.store, DS, w.universe)
    w.cols, w.inside = cols, inside
    w.match = [np.array([[cond_ref.match(r, i, cols, inside, u) for i in range(w.universe.size)] for r in RULES]) for u in USERS]
    yield w
    w.cond.free()
    w.fs.destroy()


def index_of(rows):
    r = np.asarray(rows, dtype=np.uint64)
    return np.where(r == HUGE, DS + DJ, np.where(r == U64MAX, 0, r)).astype(np.int64)


@pytest.mark.parametrize("cap", (1, 64, 65, 1025, 16384))
def test_distinct_ids_sizes(ctx, world, cap):
    rng = np.random.default_rng(cap)
    nq = 3
    rows = rng.integers(0, DS + DJ, (nq, cap)).astype(np.uint64)
    rows[rng.random((nq, cap)) < 0.03] = HUGE
    rows[rng.random((nq, cap)) < 0.05] = U64MAX
    count = np.array([cap, max(1, cap - cap // 7), cap + 3], np.uint32)
    uv, up = world.cond.pack_user(USERS)
    out = np.empty((nq, cap), np.int64)
    g = Guarded(ctx)
    try:
        d = [g.put(a) for a in (rows, count, uv, up)]
        ctx.distinct_ids_dev(world.cond, world.fs, IDS, nq, cap, d[0], d[1], d[2], d[3], g.out(out))
        g.fetch()
    finally:
        g.free()
    live = ref.live_mask(rows, count)
    want = np.stack([ref.distinct_ids_array(world.match[q][:, index_of(rows[q])], IDS, live[q]) for q in range(nq)])
    assert np.array_equal(out, want), np.argwhere(out != want)[:4].tolist()
    if cap >= 1025:
        assert set(IDS) <= set(out.reshape(-1).tolist()) and np.any(out == np.arange(1, cap + 1)[None, :])
    # no counts: every position of a request is a candidate; and the host-array entry is the same call
    got = ctx.distinct_ids(world.cond, world.fs, IDS, rows, None, USERS)
    live = ref.live_mask(rows, None)
    assert np.array_equal(got, np.stack([ref.distinct_ids_array(world.match[q][:, index_of(rows[q])], IDS, live[q]) for q in range(nq)]))


def test_distinct_ids_one_request_and_the_go_loop(ctx, world):
    rng = np.random.default_rng(5)
    n = 700
    pick = rng.integers(0, DS + DJ, n)
    cols = {k: v[pick] for k, v in world.cols.items()}
    inside = world.inside[pick]
    for v, user in enumerate(USERS):
        items = [{"properties": {}} for _ in range(n)]
        ref.go_distinct_id_sort(items, [(r, IDS[k], "d") for k, r in enumerate(RULES)],
                                lambda rule, i, item: (cond_ref.match(rule, i, cols, inside, user), None))
        want = np.array([it["properties"]["d"] for it in items], np.int64)
        assert np.array_equal(ctx.distinct_ids_one(world.cond, IDS, cols, inside, user), want)
        assert np.array_equal(pa.distinct_ids_host(world.cond, IDS, cols, inside, user), want)
    assert ctx.distinct_ids_one(world.cond, IDS, None, None, None, 0).size == 0
    boost = pa.cond_compile([{"Conditions": [], "Expression": "score + 1"}], DECL, boost=True)
    try:
        for call, code, text in ((lambda: ctx.distinct_ids_dev(boost, world.fs, [1], 1, 16, 8, 0, 0, 0, 8), -1, "boost rule set"),
                                 (lambda: ctx.distinct_ids_dev(world.cond, world.fs, IDS, 1, 16385, 8, 0, 8, 8, 8), -4, "cap=16385"),
                                 (lambda: ctx.distinct_ids_dev(world.cond, world.fs, IDS, 257, 16, 8, 0, 8, 8, 8), -1, "nq=257"),
                                 (lambda: ctx.distinct_ids_dev(world.cond, world.fs, IDS, 1, 16, 8, 0, 0, 0, 8), -1, "user properties")):
            with pytest.raises(PgError) as ei:
                call()
            assert ei.value.code == code and "pg_distinct_ids_dev: " in str(ei.value) and text in str(ei.value), str(ei.value)
    finally:
        boost.free()


# ---- the host mirror ---------------------------------------------------------------------------------------------------------------------------

MIRROR_ROWS = 20000
TAG = [{"DistinctId": -1, "Conditions": [{"Name": "recall_name", "Operator": "equal", "Domain": "item", "Type": "string", "Value": "r1"}]},
       {"DistinctId": 5, "Conditions": [{"Name": "level", "Operator": "greater", "Type": "int", "Value": "user.min_level"}]}]
MIRROR_CONFIG = {
    "RunMode": "product", "AlgoConfs": [], "RecallConfs": [],
    "SceneConfs": {"plain": {"default": {"RecallNames": ["gpu_vector_recall"]}}, "feed": {"default": {"RecallNames": ["gpu_vector_recall"]}}},
    "SortNames": {"plain": ["ItemRankScore"], "feed": ["tag_vip", "ItemRankScore"]},
    "UserDefineConfs": {"pairec_gpu": {
        "Device": 0, "Table": {"Rows": MIRROR_ROWS, "Dim": 128, "IdPrefix": "item_", "SyntheticSeed": o.SEED_TABLE},
        "Recalls": [{"Name": "gpu_vector_recall", "Kind": "vector", "RecallCount": 300, "RecallAlgo": "gpu_faiss", "ItemType": "video"}],
        "Algorithms": [{"Name": "gpu_faiss", "Kind": "faiss"}],
        "Filters": [{"Name": "one_per_author", "FilterType": "DimensionFieldUniqueFilter", "Dimension": "author", "NullValue": 0},
                    {"Name": "no_such_column", "FilterType": "DimensionFieldUniqueFilter", "Dimension": "colour"}],
        "FilterNames": {"feed": ["one_per_author"]},
        "Sorts": [{"Name": "tag", "SortType": "DistinctIdSort", "DistinctIdConditions": TAG},
                  {"Name": "tag_other", "SortType": "DistinctIdSort",
                   "DistinctIdConditions": [{"DistinctId": 9, "DistinctIdName": "__other__", "Conditions": TAG[1]["Conditions"]}]},
                  {"Name": "tag_vip", "SortType": "DistinctIdSort",
                   "DistinctIdConditions": [{"DistinctId": 1, "Conditions": [{"Name": "vip", "Domain": "user", "Operator": "equal", "Type": "int", "Value": 1}]}]}]}},
}


def test_filter_and_sort_through_the_mirror():
    H = C.CDLL(os.environ.get("PH_HOST_LIB") or os.path.join(ROOT, "pairec_amd", "libpairec_host.so"))
    H.ph_last_error.restype = C.c_char_p
    H.ph_engine_create.restype = C.c_void_p
    H.ph_engine_create.argtypes = [C.c_char_p]
    H.ph_engine_destroy.argtypes = [C.c_void_p]
    H.ph_set_user_vector.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    H.ph_engine_set_feature_column.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
    H.ph_engine_filter.restype = C.c_char_p
    H.ph_engine_filter.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]
    H.ph_engine_sort_props.restype = C.c_char_p
    H.ph_engine_sort_props.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    H.ph_recommend.restype = C.c_char_p
    H.ph_recommend.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p]
    h = H.ph_engine_create(json.dumps(MIRROR_CONFIG).encode())
    assert h, H.ph_last_error()
    try:
        rng = np.random.default_rng(6)
        author = rng.integers(0, 120, MIRROR_ROWS).astype(np.int32)            # 0 stands for "" (NullValue)
        assert H.ph_engine_set_feature_column(h, b"author", author.ctypes.data_as(C.c_void_p), MIRROR_ROWS) == 0, H.ph_last_error()

        def as_items(ids):
            """the items as the Go filter sees them: the author as a string property, none where the table does not know the id or
            the value is the null code"""
            out = []
            for i in ids:
                r = int(i[5:]) if i.startswith("item_") and int(i[5:]) < MIRROR_ROWS else None
                out.append({"id": i, "properties": {} if r is None or author[r] == 0 else {"author": int(author[r])}})
            return out

        ids = ["item_%d" % r for r in rng.choice(MIRROR_ROWS, 900, replace=False)] + ["stranger_1", "item_99999999", "stranger_2"]
        rng.shuffle(ids)
        items = [{"id": i, "score": float(k)} for k, i in enumerate(ids)]
        r = H.ph_engine_filter(h, b"one_per_author", json.dumps(items).encode(), b"{}")
        assert r, H.ph_last_error()
        got = json.loads(r)["items"]
        want = [it["id"] for it in ref.go_dimension_field_unique(as_items(ids), "author")]
        assert [x["item_id"] for x in got] == want and 100 < len(want) < 200
        assert {"stranger_1", "stranger_2", "item_99999999"} <= set(want)
        assert [x["score"] for x in got] == [float(ids.index(i)) for i in want]            # the items themselves, scores untouched
        assert json.loads(H.ph_engine_filter(h, b"one_per_author", b"[]", b"{}"))["items"] == []
        assert H.ph_engine_filter(h, b"no_such_column", json.dumps(items).encode(), b"{}") is None
        assert b"DimensionFieldUniqueFilter no_such_column" in H.ph_last_error() and b'"colour" is not a feature column' in H.ph_last_error()

        # the sort: the kept items, tagged under one name; a second sort writes its own name beside it
        kept = [{"id": i, "score": 1.0, "properties": {"recall_name": "r1" if k % 3 == 0 else "r2", "level": k % 7}} for k, i in enumerate(want)]
        for user in ({"min_level": 4}, {}):
            r = H.ph_engine_sort_props(h, b"tag", json.dumps(kept).encode(), json.dumps(user).encode(), 10)
            assert r, H.ph_last_error()
            got = json.loads(r)["items"]
            go = [{"properties": dict(it["properties"])} for it in kept]
            cols = {"recall_name": np.array([1 if it["properties"]["recall_name"] == "r1" else 2 for it in kept]),
                    "level": np.array([it["properties"]["level"] for it in kept])}
            rules = [[dict(TAG[0]["Conditions"][0], Value=1)], TAG[1]["Conditions"]]
            ref.go_distinct_id_sort(go, [(rules[0], -1, "__distinct_id__"), (rules[1], 5, "__distinct_id__")],
                                    lambda rule, i, item: (cond_ref.match(rule, i, cols, np.ones(len(kept), bool), user), None))
            assert [x["item_id"] for x in got] == want                                    # order untouched
            assert [x["properties"]["__distinct_id__"] for x in got] == [it["properties"]["__distinct_id__"] for it in go]
            assert all(x["properties"]["level"] == it["properties"]["level"] for x, it in zip(got, kept))
            tags = [x["properties"]["__distinct_id__"] for x in got]
            assert -1 in tags and (tags.count(5) > 1) == bool(user) and any(v > 5 for v in tags)       # (one 5 is position 4's own)
        r = H.ph_engine_sort_props(h, b"tag_other", json.dumps(kept).encode(), b'{"min_level": 2}', 10)
        assert [x["properties"]["__other__"] for x in json.loads(r)["items"]] == [9 if k % 7 > 2 else k + 1 for k in range(len(kept))]
        lacking = [dict(it, properties={"recall_name": "r1"}) for it in kept]
        assert H.ph_engine_sort_props(h, b"tag", json.dumps(lacking).encode(), b"{}", 10) is None
        assert b"DistinctIdSort" in H.ph_last_error() and b'"level"' in H.ph_last_error()

        # the scene: recall → DimensionFieldUniqueFilter → DistinctIdSort → ItemRankScore returns the page the Go loop leaves
        user = o.synth_rows(o.SEED_QUERY, 3, 1, 128)[0]
        H.ph_set_user_vector(h, b"u1", " ".join("%d:%s" % (i + 1, repr(float(v))) for i, v in enumerate(user)).encode())
        base = json.loads(H.ph_recommend(h, b"u1", 300, b"plain"))["items"]
        assert len(base) == 300
        page = json.loads(H.ph_recommend(h, b"u1", 300, b"feed"))["items"]
        uniq = [it["id"] for it in ref.go_dimension_field_unique(as_items([x["item_id"] for x in base]), "author")]
        assert [x["item_id"] for x in page] == uniq and 60 < len(uniq) < 300
    finally:
        H.ph_engine_destroy(h)
