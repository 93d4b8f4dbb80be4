"""GPU tests of PriorityAdjustCountFilterV2 on the device (csrc/trim2.hip, pg_candidates_trim2_dev) against
tests/trim2_ref.py: every output array is compared by bits, padding and counts included.  The sizes sit on the kernels' edges — a
wave of 64 lanes, the chunk of 1 024 positions, the largest cap of 16 384 — and the rules on the cut's: limits at a chunk's end,
chunks without an eligible entry, limits of 0 and of UINT32_MAX."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fanin_ref
import trim2_ref as ref
import trim_ref
import pairec_amd as pa
from pairec_amd._lib import PgError

from test_trim2_cpu import GOLDEN, MIRROR_CONFIG, golden_merge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64MAX = ref.U64MAX
FIX, ACC, ANY = ref.FIX, ref.ACCUMULATE, ref.ANY


def merged_case(rng, nq, cap, n_src, overlap=0.4, pad=0.05, with_count=True, n32=2):
    """(rows, score, source, count, planes_f64, source_mask, planes_f32) as a fan-in leaves them: the mask names the first source
    and, with probability `overlap` each, the others (0.4 each: 30 - 50 % of the items are held twice or more for 2 - 3 sources);
    plane s holds source s's score where the mask names it, NaN elsewhere; 40 % of the scores from a handful of values, so that
    ties occur inside a list, across lists and across chunks"""
    rows = (rng.permutation(nq * cap).reshape(nq, cap).astype(np.uint64) * np.uint64(977)) + np.uint64(1 << 21)
    rows[rng.random((nq, cap)) < pad] = U64MAX

    def scores(shape):
        s = rng.standard_normal(shape)
        tie = rng.random(shape) < 0.4
        s[tie] = rng.integers(-2, 3, shape)[tie] * 0.5
        return s
    score = scores((nq, cap))
    source = rng.integers(0, n_src, (nq, cap)).astype(np.uint8)
    count = rng.integers(cap // 2, cap + 1, nq).astype(np.uint32) if with_count else None
    mask = np.uint32(1) << source.astype(np.uint32)
    p64 = np.full((n_src, nq, cap), np.nan)
    for s in range(n_src):
        held = (rng.random((nq, cap)) < overlap) & (source != s)
        mask = mask | (held.astype(np.uint32) << np.uint32(s))
        p64[s] = np.where(held, scores((nq, cap)), p64[s])
        p64[s] = np.where(source == s, score, p64[s])
    return rows, score, source, count, p64, mask.astype(np.uint32), rng.standard_normal((n32, nq, cap)).astype(np.float32)


def mixed_rules(n_src, counts):
    """every source, FIX and ACCUMULATE in turn, in an order that is not the source order"""
    order = list(range(n_src))[::-1]
    return [(s, (FIX, ACC)[i % 2], counts[i % len(counts)]) for i, s in enumerate(order)]


def check(ctx, rules, case, optional=False):
    rows, score, source, count, p64, mask, p32 = case
    got = ctx.candidates_trim2(rules, rows, score, source, count, p64, mask, p32)
    ref.same(got, ref.trim2(rules, rows, score, source, count, p64, mask, p32))
    if optional:
        # every optional array absent (then one rule owns every entry), and one at a time
        one = rules[:1]
        ref.same(ctx.candidates_trim2(one, rows, score), ref.trim2(one, rows, score))
        ref.same(ctx.candidates_trim2(rules, rows, score, source), ref.trim2(rules, rows, score, source))
        ref.same(ctx.candidates_trim2(one, rows, score, None, count), ref.trim2(one, rows, score, None, count))
        ref.same(ctx.candidates_trim2(rules, rows, score, source, None, p64), ref.trim2(rules, rows, score, source, None, p64))
        ref.same(ctx.candidates_trim2(rules, rows, score, source, None, p64, mask), ref.trim2(rules, rows, score, source, None, p64, mask))
        ref.same(ctx.candidates_trim2(one, rows, score, None, None, p64, mask), ref.trim2(one, rows, score, None, None, p64, mask))
        ref.same(ctx.candidates_trim2(one, rows, score, None, None, None, None, p32), ref.trim2(one, rows, score, None, None, None, None, p32))
    return got


# ---- sizes, requests and sources ---------------------------------------------------------------------------------------------------

SIZES = [(nq, cap) for cap in (1, 63, 64, 65, 1023, 1024, 1025, 2049, 16384) for nq in (1, 3, 256) if nq < 256 or cap <= 1025]


@pytest.mark.parametrize("nq,cap", SIZES)
def test_sizes_and_sources(ctx, nq, cap):
    rng = np.random.default_rng(1000 * nq + cap)
    n_src = 1 + (cap + nq) % 8                                       # 1 .. 8 sources over the cases
    if nq == 256:
        n_src = min(n_src, 3)                                        # (the reference walks every list in Python)
    case = merged_case(rng, nq, cap, n_src, n32=1)
    rules = mixed_rules(n_src, (max(1, cap // 5), max(1, cap // 2), 3, cap))
    got = check(ctx, rules, case, optional=nq == 3 and cap <= 2049)
    assert got[0].shape[1] == ref.out_cap(rules, cap)


@pytest.mark.parametrize("n_src", range(1, 9))
def test_one_to_eight_sources(ctx, n_src):
    rng = np.random.default_rng(n_src)
    case = merged_case(rng, 3, 1500, n_src, overlap=0.4)
    check(ctx, mixed_rules(n_src, (200, 450, 90, 700)), case)
    check(ctx, [(s, ACC, 150 * (i + 1)) for i, s in enumerate(range(n_src))], case)
    # only some of the sources are named: the singles of the others are dropped, their duplicates come in under a named one
    got = check(ctx, mixed_rules(n_src, (300, 500))[::2], case)
    assert set(got[2][got[2] != 0xFF].tolist()) <= set(s for s, _, _ in mixed_rules(n_src, (300, 500))[::2])


# ---- limits at the chunk's edge ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def long_case():
    # two sources, 60 % held by the other one as well: both lists are longer than two chunks
    return merged_case(np.random.default_rng(7), 3, 4000, 2, overlap=0.6, pad=0.02, with_count=False)


@pytest.mark.parametrize("count", [1, 1023, 1024, 1025, 2047, 2048, 2049])
def test_limits_at_the_chunks_edge(ctx, long_case, count):
    for rules in ([(1, FIX, count), (0, FIX, count)], [(0, ACC, count), (1, ACC, count + 1024)], [(1, ACC, count), (0, FIX, 1024)]):
        got = check(ctx, rules, long_case)
        assert np.all(got[6] >= count)                                   # (the first rule's list is longer than two chunks)


def test_limit_zero_and_the_largest_count(ctx, long_case):
    # count <= acc: the rule's limit is 0, it walks nothing and the next rule starts where it stood
    got = check(ctx, [(0, ACC, 1500), (1, ACC, 1500)], long_case)
    assert np.all(got[6] == 1500) and np.all(got[2][:, :1500] == 0)
    got = check(ctx, [(0, ACC, 1500), (1, ACC, 700)], long_case)          # a decreasing accumulate count: legal, limit 0
    assert np.all(got[6] == 1500)
    check(ctx, [(0, FIX, 0), (1, ACC, 0)], long_case)                     # out_cap 0: only the counts are written
    got = check(ctx, [(1, FIX, 0xFFFFFFFF), (0, ACC, 0xFFFFFFFF)], long_case)
    real = (long_case[0] != U64MAX).sum(axis=1)
    assert np.array_equal(got[6], real)                                   # every real entry leaves, once
    check(ctx, [(0, ACC, 0xFFFFFFFF), (1, FIX, 0xFFFFFFFF)], long_case)


# ---- entries an earlier rule took ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [1023, 1024, 1025, 1500, 2048, 2100])
def test_taken_entries_fill_a_rules_first_chunks(ctx, first):
    rng = np.random.default_rng(31)
    cap = 3000
    rows, score, source, _, p64, mask, p32 = merged_case(rng, 2, cap, 2, overlap=1.0, pad=0.0, with_count=False)
    # every item held by both sources, both recalls order them alike: rule 0 takes the head of rule 1's list, so rule 1's first
    # one or two chunks hold no eligible entry and its picks start behind them
    mask[:] = 3
    score[:] = -np.arange(cap, dtype=np.float64)
    score[1] = score[1, rng.permutation(cap)]
    p64[0], p64[1] = score, score - 0.25
    got = check(ctx, [(1, FIX, first), (0, FIX, 700)], (rows, score, source, None, p64, mask, p32))
    assert np.all(got[6] == first + 700) and np.all(got[2][:, :first] == 1) and np.all(got[2][:, first:] == 0)
    assert np.array_equal(got[0][0, first:], rows[0, first:first + 700])
    check(ctx, [(0, ACC, first), (1, ACC, first + 1024)], (rows, score, source, None, p64, mask, p32))
    # three sources in unrelated orders, every item in every list
    case = merged_case(rng, 2, 2500, 3, overlap=1.0)
    check(ctx, [(2, FIX, 1024), (0, ACC, 1030), (1, ACC, 2500)], case)


# ---- keys ---------------------------------------------------------------------------------------------------------------------------

def test_all_keys_equal_and_nan_members(ctx):
    rng = np.random.default_rng(41)
    rows, score, source, count, p64, mask, p32 = merged_case(rng, 3, 2100, 3, overlap=0.5)
    eq_score, eq_p64 = np.full_like(score, 0.5), np.where(np.isnan(p64), p64, 0.5)
    check(ctx, [(2, FIX, 300), (0, ACC, 500), (1, ACC, 1100)], (rows, eq_score, source, count, eq_p64, mask, p32))
    # a NaN plane value under a set mask bit: a member that sorts among the non-members, wherever those lie
    nan_p64 = p64.copy()
    held = ((mask >> 1) & 1).astype(bool) & (source != 1)
    nan_p64[1][held & (rng.random(held.shape) < 0.5)] = np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0]
    score2 = score.copy()
    score2[rng.random(score.shape) < 0.1] = np.nan
    got = check(ctx, [(1, FIX, 2100), (0, FIX, 2100), (2, FIX, 2100)], (rows, score2, source, count, nan_p64, mask, p32))
    assert 0x7FF8000000000123 in set(got[1].view(np.uint64)[0, :int(got[6][0])].tolist())
    check(ctx, [(1, ACC, 1030), (2, ACC, 1100)], (rows, score2, source, count, nan_p64, mask, p32))


SPECIAL = np.array([0x7FF8000000000001, 0x7FF4DEADBEEF0001, 0xFFF8000000000123, 0x7FF0000000000000, 0xFFF0000000000000,
                    0x8000000000000000, 0x0000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x0010000000000000,
                    0x3FF0000000000001, 0x3FF0000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF], np.uint64).view(np.float64)


def test_special_values_and_padding(ctx):
    rng = np.random.default_rng(51)
    rows, score, source, count, p64, mask, p32 = merged_case(rng, 4, 1400, 3, overlap=0.5, pad=0.0)
    score[:] = SPECIAL[rng.integers(0, SPECIAL.size, score.shape)]
    p64[:] = SPECIAL[rng.integers(0, SPECIAL.size, p64.shape)]
    rows[:, 5:900:3] = U64MAX                                        # padding in the middle of every list
    rows[3] = U64MAX                                                 # request 3: padding only
    source[1, 10:700:7] = 200                                        # a source no rule can name
    count = np.array([0, 1400, 1023, 1400], np.uint32)               # d_count[q] = 0 and = cap
    rules = [(2, ACC, 300), (0, FIX, 1400), (1, ACC, 900)]
    got = check(ctx, rules, (rows, score, source, count, p64, mask, p32))
    assert got[6][0] == 0 and got[6][3] == 0 and np.all(got[0][[0, 3]] == U64MAX) and np.all(got[2][[0, 3]] == 0xFF)
    assert np.all(got[1].view(np.uint64)[[0, 3]] == ref.NEG_INF_BITS) and np.all(got[3].view(np.uint64)[:, [0, 3]] == ref.NAN_BITS)
    assert not np.any(got[4][[0, 3]]) and not np.any(got[5].view(np.uint32)[:, [0, 3]])
    check(ctx, rules, (rows, score, source, np.array([5000, 1401, 0xFFFFFFFF, 7], np.uint32), p64, mask, p32))    # a count beyond cap is cap


# ---- repeats and leftover duplicates -----------------------------------------------------------------------------------------------

def test_repeats_and_leftover_duplicates(ctx):
    # source 0 holds id 7 twice (scores 5.0 then 9.0) and source 1 holds it too: UniqueFilter keeps Item.Score 5.0 and
    # RecallScores[s0] = 9.0; the pick carries the plane's
    r0 = np.array([[7, 1, 2, 7, 3]], np.uint64)
    s0 = np.array([[5.0, 4.0, 3.0, 9.0, 2.0]])
    r1 = np.array([[3, 10, 11, 1, 7]], np.uint64)
    s1 = np.array([[8.0, 7.0, 6.0, 0.5, 0.125]])
    r2 = np.array([[11, 20, 2]], np.uint64)
    s2 = np.array([[1.0, 0.25, 7.5]])
    w = fanin_ref.merge([(r0, s0), (r1, s1), (r2, s2)])
    rows, score, source, planes, mask, count = w
    assert score[0, 0] == 5.0 and planes[0, 0, 0] == 9.0
    got = check(ctx, [(0, FIX, 2)], (rows, score, source, count, planes, mask, np.zeros((1, 1, rows.shape[1]), np.float32)))
    assert got[0][0, :2].tolist() == [7, 1] and got[1][0, 0] == 9.0
    # 3 (sources 0, 1) and 1 (0, 1): rule 1 takes 3 (8.0) and 10; rule 0's quota of 1 goes to 7; 1 and 2 stay behind with every
    # quota that could take them used up, and are dropped; 11 (sources 1, 2) and 2 (0, 2) are held by source 2, which no rule
    # names — 11 is left over, 2 too
    got = check(ctx, [(1, FIX, 2), (0, FIX, 1)], (rows, score, source, count, planes, mask, np.zeros((1, 1, rows.shape[1]), np.float32)))
    assert got[0][0].tolist() == [3, 10, 7] and got[2][0].tolist() == [1, 1, 0] and got[6][0] == 3
    # a duplicate no named source holds: 2 (sources 0 and 2) under a rule for source 1 only; 20, a single of source 2, goes too
    got = check(ctx, [(1, FIX, 9)], (rows, score, source, count, planes, mask, np.zeros((1, 1, rows.shape[1]), np.float32)))
    assert got[0][0, :int(got[6][0])].tolist() == [3, 10, 11, 1, 7]


# ---- cross-checks --------------------------------------------------------------------------------------------------------------------

def test_without_a_mask_the_call_is_the_trim(ctx):
    rng = np.random.default_rng(61)
    for cap, n_src in ((1025, 3), (2500, 5)):
        rows, score, source, count, p64, mask, p32 = merged_case(rng, 3, cap, n_src)
        rules = [(s, (ACC, FIX)[i % 2], cap // 5 * (i + 1)) for i, s in enumerate(range(n_src)[::-1])]
        want = ctx.candidates_trim(rules, rows, score, source, count, p64, None, p32)
        ref.same(ctx.candidates_trim2(rules, rows, score, source, count, p64, None, p32), want)
        ref.same(want, trim_ref.trim(rules, rows, score, source, count, p64, None, p32))


def test_trim2_over_a_fanin_merge_on_the_device(ctx):
    rng = np.random.default_rng(62)
    nq, ks = 2, (500, 200, 100)
    src, seen = [], None
    for i, k in enumerate(ks):
        rows = np.empty((nq, k), np.uint64)
        for q in range(nq):
            fresh = rng.choice(1 << 30, k, replace=False).astype(np.uint64) + np.uint64(1 << 20)
            if seen is not None:
                n_old = int(0.3 * k)                                 # 30 % of a list repeats ids of the lists before it
                fresh[:n_old] = rng.choice(seen[q], n_old, replace=False)
                rng.shuffle(fresh)
            rows[q] = fresh
        src.append((rows, rng.standard_normal((nq, k))))
        seen = rows if seen is None else np.concatenate([seen, rows], axis=1)
    cap = sum(ks)
    rules = [(2, FIX, 60), (0, ACC, 150), (1, ACC, 250)]
    oc = ref.out_cap(rules, cap)
    bufs = []

    def dev(a):
        bufs.append(ctx.to_device(a) if isinstance(a, np.ndarray) else ctx.malloc(a))
        return bufs[-1]
    d_src = [(dev(r), dev(s), r.shape[1], True) for r, s in src]
    m = [dev(nq * cap * 8), dev(nq * cap * 8), dev(nq * cap), dev(3 * nq * cap * 8), dev(nq * cap * 4), dev(nq * 4)]
    outs = [np.empty((nq, oc), np.uint64), np.empty((nq, oc), np.float64), np.empty((nq, oc), np.uint8), np.empty((3, nq, oc), np.float64),
            np.empty((nq, oc), np.uint32), None, np.empty(nq, np.uint32)]
    d_out = [dev(a.nbytes) if a is not None else 0 for a in outs]
    try:
        ctx.fanin_merge_dev(d_src, nq, *m)                           # the merge's outputs stay where they are: no host copy between
        ctx.candidates_trim2_dev(rules, nq, cap, m[0], m[1], m[2], m[5], m[3], 3, m[4], 0, 0, *d_out)
        ctx.synchronize()
        for a, p in zip(outs, d_out):
            if a is not None:
                ctx.d2h(a, p)
    finally:
        for b in bufs:
            ctx.free(b)
    w = fanin_ref.merge(src)
    want = ref.trim2(rules, w[0], w[1], w[2], w[5], w[3], w[4])
    ref.same(tuple(outs), want)
    assert np.all(outs[6] == 310)
    pos = {int(r): i for i, r in enumerate(w[0][0, :int(w[5][0])])}
    assert any(w[2][0, pos[int(r)]] != s for r, s in zip(outs[0][0], outs[2][0]))       # some left under a later recall's name


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_the_reference_tests_answers(ctx, case):
    names, rules, (rows, score, source, planes, mask, count) = golden_merge(case)
    got = ctx.candidates_trim2(rules, rows, score, source, count, planes, mask)
    n = len(case["expect_ids"])
    assert got[6][0] == n and got[0][0, :n].tolist() == [names.index(i) for i in case["expect_ids"]]
    assert got[2][0, :n].tolist() == [case["recalls"].index(r) for r in case["expect_retrieve_ids"]]
    ref.same(got, ref.trim2(rules, rows, score, source, count, planes, mask))


# ---- refusals and scratch ----------------------------------------------------------------------------------------------------------

def test_argument_errors_leave_the_context_usable(ctx):
    d = ctx.malloc(1 << 16)
    o = ctx.malloc(1 << 16)
    ok = [(0, FIX, 2), (1, ACC, 4)]

    def call(rules=ok, nq=1, cap=16, **kw):
        a = dict(d_rows=d, d_score=d, d_source=d, d_count=0, d_planes_f64=0, n_f64=0, d_source_mask=0, d_planes_f32=0, n_f32=0,
                 d_out_rows=o, d_out_score=o, d_out_source=o, d_out_planes_f64=0, d_out_source_mask=0, d_out_planes_f32=0, d_out_count=o)
        a.update(kw)
        ctx.candidates_trim2_dev(rules, nq, cap, **a)

    for kw, code, text in (
            (dict(rules=[]), -1, "no rules (AdjustCountConfs is empty)"),
            (dict(rules=[(1, FIX, 1), (1, ACC, 2)]), -1, "source 1 is named twice (the reference would emit its items twice)"),
            (dict(rules=[(ANY, FIX, 4)]), -1, "rule 0 is PG_TRIM_ANY (V2 reads RecallScores by recall name: every rule names a source)"),
            (dict(rules=[(8, FIX, 4)]), -1, "rule 0 names source 8 (< 8)"),
            (dict(rules=[(0, 7, 4)]), -1, "rule 0 has type 7 (PG_TRIM_FIX or PG_TRIM_ACCUMULATE)"),
            (dict(rules=[(s % 8, FIX, 1) for s in range(9)]), -4, "n_rules=9 unsupported (1..8)"),
            (dict(cap=0), -4, "cap=0 unsupported (1..16384)"), (dict(cap=16385), -4, "cap=16385 unsupported (1..16384)"),
            (dict(nq=0), -1, "nq=0 must be in [1,256]"), (dict(nq=257), -1, "nq=257 must be in [1,256]"),
            (dict(d_rows=0), -1, "NULL argument"), (dict(d_out_count=0), -1, "NULL argument"),
            (dict(d_source=0, d_out_source=0), -1, "rules that name more than one source need d_source"),
            (dict(d_out_source=0), -1, "d_source / d_source_mask and their outputs come in pairs"),
            (dict(d_source_mask=d), -1, "d_source / d_source_mask and their outputs come in pairs"),
            (dict(d_planes_f64=d, n_f64=1), -1, "a carried plane set and its output come in pairs"),
            (dict(d_planes_f64=d, d_out_planes_f64=o, n_f64=9), -1, "a carried plane set holds 1..8 planes"),
            (dict(d_source_mask=d, d_out_source_mask=o), -1, "a source mask needs the per-recall score planes of every named source (n_f64 >= 2)"),
            (dict(d_source_mask=d, d_out_source_mask=o, d_planes_f64=d, d_out_planes_f64=o, n_f64=1), -1,
             "a source mask needs the per-recall score planes of every named source (n_f64 >= 2)"),
            (dict(d_out_rows=d), -1, "an output overlaps its input"), (dict(d_out_score=d + 8), -1, "an output overlaps its input")):
        with pytest.raises(PgError) as ei:
            call(**kw)
        assert ei.value.code == code and str(ei.value).endswith(": pg_candidates_trim2_dev: " + text), kw
    ctx.free(d)
    ctx.free(o)
    check(ctx, ok, merged_case(np.random.default_rng(15), 2, 16, 2))


def test_first_call_of_a_context_is_the_largest():
    rng = np.random.default_rng(71)
    big = merged_case(rng, 2, 16384, 8, overlap=0.3, n32=1)
    small = merged_case(rng, 1, 1, 1)
    with pa.Context(0) as fresh:                                     # the scratch slot grows on the first call, and is reused
        check(fresh, mixed_rules(8, (700, 3000, 1024, 9000)), big)
        check(fresh, [(0, FIX, 1)], small)
        check(fresh, mixed_rules(8, (1, 2, 3)), big)


# ---- the host mirror ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mirror():
    L = C.CDLL(os.environ.get("PH_HOST_LIB") or os.path.join(ROOT, "pairec_amd", "libpairec_host.so"))
    L.ph_last_error.restype = C.c_char_p
    L.ph_engine_create.restype = C.c_void_p
    L.ph_engine_create.argtypes = [C.c_char_p]
    L.ph_engine_destroy.argtypes = [C.c_void_p]
    L.ph_engine_filter.restype = C.c_char_p
    L.ph_engine_filter.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]
    h = L.ph_engine_create(json.dumps(MIRROR_CONFIG).encode())
    assert h, L.ph_last_error()

    def run(name, items):
        r = L.ph_engine_filter(h, name.encode(), json.dumps(items).encode(), b"{}")
        return (json.loads(r)["items"], None) if r else (None, L.ph_last_error())
    yield run
    L.ph_engine_destroy(h)


NAMES = ["recall_A", "recall_B", "recall_C", "recall_D"]


def mirror_items(seed, n=300):
    """items as UniqueFilter leaves them, keys distinct inside every list (there the reference is deterministic)"""
    rng = np.random.default_rng(seed)
    rows, score, source, _, p64, mask, _ = merged_case(rng, 1, n, 4, overlap=0.4, pad=0.0, with_count=False)
    keys = rng.permutation(5 * n).astype(np.float64).reshape(5, n) * 0.25 - 100.0
    score[0] = keys[4]
    for b in range(4):
        p64[b, 0] = np.where(source[0] == b, score[0], keys[b])
    items = []
    for i in range(n):
        it = {"id": "x%d" % i, "score": float(score[0, i]), "retrieve_id": NAMES[source[0, i]]}
        if bin(int(mask[0, i])).count("1") > 1:
            it["recall_scores"] = {NAMES[b]: float(p64[b, 0, i]) for b in range(4) if (int(mask[0, i]) >> b) & 1}
        items.append(it)
    return items, score, source


def test_both_quota_filters_through_the_mirror(mirror):
    filters = {f["Name"]: f for f in MIRROR_CONFIG["UserDefineConfs"]["pairec_gpu"]["Filters"]}
    items, score, source = mirror_items(81)
    # V2 against the transcription of its loop: ids, names and scores as the reference rewrites them
    objs = [ref.Item(it["id"], it["score"], it["retrieve_id"], it.get("recall_scores")) for it in items]
    want = ref.go_v2(filters["quota2"]["AdjustCountConfs"], objs)
    got, err = mirror("quota2", items)
    assert err is None and len(want) == 10 + 5
    assert [x["item_id"] for x in got] == [it.Id for it in want]
    assert [x["retrieve_id"] for x in got] == [it.RetrieveId for it in want]
    assert [x["score"] for x in got] == [it.Score for it in want]
    assert any(x["retrieve_id"] != NAMES[source[0, int(x["item_id"][1:])]] for x in got)
    # v1 against its restatement (trim_ref: priority_adjust_count_filter.go:92-203): an item is its first recall's only
    rules = [(NAMES.index(c["RecallName"]), FIX if c["Type"] == "fix" else ACC, c["Count"]) for c in filters["quota1"]["AdjustCountConfs"]]
    keep = trim_ref.picks(rules, score[0], source[0], list(range(len(items))))
    got, err = mirror("quota1", items)
    assert err is None and [x["item_id"] for x in got] == ["x%d" % i for i in keep]
    assert [x["retrieve_id"] for x in got] == [NAMES[source[0, i]] for i in keep] and [x["score"] for x in got] == [float(score[0, i]) for i in keep]
    assert mirror("quota2", []) == ([], None)


def test_too_many_items_is_that_requests_error(mirror):
    many = [{"id": "y%d" % i, "score": float(i), "retrieve_id": "recall_A"} for i in range(16385)]
    for name, word in (("quota2", b"PriorityAdjustCountFilterV2 quota2"), ("quota1", b"PriorityAdjustCountFilter quota1")):
        got, err = mirror(name, many)
        assert got is None and word in err and b"16385 items" in err
    got, err = mirror("quota2", many[:40])                            # the engine serves the next request
    assert err is None and [x["item_id"] for x in got] == ["y%d" % i for i in range(39, 34, -1)]
