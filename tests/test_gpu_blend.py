"""GPU tests of the candidate blend (csrc/blend.hip, pg_candidates_blend_dev) against tests/blend_ref.py: every
output array is compared by bits, padding and counts included.  The sizes sit on the kernels' edges — a wave of 64 lanes, the
chunk of 1 024 positions, the 2 064 list entries kept in LDS, the largest cap of 16 384."""
import numpy as np
import pytest

import blend_ref as ref
import fanin_ref
import pairec_amd as pa
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

U64MAX = ref.U64MAX
REFILL, SKIP, FAIR = ref.SNAKE_REFILL, ref.SNAKE_SKIP, ref.FAIR
MODES = (REFILL, SKIP, FAIR)


def merged_case(rng, nq, cap, n_src, overlap=0.3, pad=0.05, with_count=True, n32=2):
    """(rows, score, source, count, planes_f64, source_mask, planes_f32) as a fan-in leaves them: the mask names the first source
    and, with probability `overlap` each, the others; plane s holds source s's score where the mask names it, NaN elsewhere; a
    handful of distinct scores beside continuous ones, so that ties occur inside a list, across lists and across chunks"""
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


def snake_entries(n_src, weights):
    """every source, in an order that is not the source order"""
    order = list(range(n_src))[::-1]
    return [(s, weights[i % len(weights)]) for i, s in enumerate(order)]


def check(ctx, conf, case, optional=False):
    rows, score, source, count, p64, mask, p32 = case
    got = ctx.candidates_blend(conf, rows, score, source, count, p64, mask, p32)
    ref.same(got, ref.blend(conf, rows, score, source, count, p64, mask, p32))
    if optional:
        # every optional array absent (a snake without sources names one), and one at a time
        bare = conf if conf[0] == FAIR else (conf[0], conf[1], [(conf[2][0][0], max(conf[2][0][1], 1))])
        ref.same(ctx.candidates_blend(bare, rows, score), ref.blend(bare, rows, score))
        ref.same(ctx.candidates_blend(conf, rows, score, source), ref.blend(conf, rows, score, source))
        ref.same(ctx.candidates_blend(bare, rows, score, None, count), ref.blend(bare, rows, score, None, count))
        ref.same(ctx.candidates_blend(conf, rows, score, source, None, p64), ref.blend(conf, rows, score, source, None, p64))
        ref.same(ctx.candidates_blend(conf, rows, score, source, None, p64, mask), ref.blend(conf, rows, score, source, None, p64, mask))
        ref.same(ctx.candidates_blend(bare, rows, score, None, None, None, None, p32), ref.blend(bare, rows, score, None, None, None, None, p32))
        if conf[0] == FAIR:                                              # (FAIR carries a mask without planes)
            ref.same(ctx.candidates_blend(conf, rows, score, source, None, None, mask), ref.blend(conf, rows, score, source, None, None, mask))
    return got


# ---- sizes, modes and sources -----------------------------------------------------------------------------------------------------

SIZES = [(nq, cap) for cap in (1, 63, 64, 65, 1023, 1024, 1025, 2049, 16384) for nq in (1, 3, 256) if nq < 256 or cap <= 1025]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nq,cap", SIZES)
def test_sizes_and_sources(ctx, nq, cap, mode):
    rng = np.random.default_rng(1000 * nq + cap)
    n_src = 1 + (cap + nq) % 8                                       # 1 .. 8 sources over the cases
    if nq == 256:
        n_src = min(n_src, 4)                                        # (the reference walks every list in Python)
    case = merged_case(rng, nq, cap, n_src, n32=1)
    retain = max(1, (2 * cap) // 3)
    check(ctx, (mode, retain, snake_entries(n_src, (3, 1, 64, 2))), case, optional=nq == 3 and cap <= 2049)


@pytest.mark.parametrize("n_src", range(1, 9))
def test_one_to_eight_sources(ctx, n_src):
    rng = np.random.default_rng(n_src)
    case = merged_case(rng, 3, 1500, n_src, overlap=0.5)
    for mode in MODES:
        check(ctx, (mode, 700, snake_entries(n_src, (5, 1, 2))), case)
    # only some of the sources are named
    check(ctx, (REFILL, 700, snake_entries(n_src, (2, 3))[::2]), case)


# ---- weights and cuts ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def walk_case():
    return merged_case(np.random.default_rng(7), 3, 1500, 4, overlap=0.4)


@pytest.mark.parametrize("weights", [(0, 1, 63, 64), (65, 0, 1, 64), (64, 64, 64, 64), (63, 65, 1, 0), (1, 1, 1, 1), (5000, 1, 1, 2), (0xFFFFFFFF, 7, 0, 0)])
@pytest.mark.parametrize("mode", (REFILL, SKIP))
def test_weights(ctx, walk_case, mode, weights):
    entries = [(s, w) for s, w in zip((2, 0, 3, 1), weights)]
    for retain in (1, 130, 1500, 4000):                              # 130 cuts a round of the wider weights in the middle
        check(ctx, (mode, retain, entries), walk_case)


@pytest.mark.parametrize("retain", [1, 2, 7, 1499, 1500, 1501, 0xFFFFFFFF])
def test_fair_cuts(ctx, walk_case, retain):
    got = check(ctx, (FAIR, retain, []), walk_case)
    assert got[0].shape[1] == min(retain, 1500)


def test_fair_sources_that_run_out_one_after_the_other(ctx):
    rng = np.random.default_rng(21)
    rows, score, source, _, p64, mask, p32 = merged_case(rng, 3, 2049, 8, pad=0.0, with_count=False)
    # sizes 1, 2, 4, ... so that every exhaustion changes the slot table; request 1: one source only; request 2: all equal
    source[0] = np.minimum(np.floor(np.log2(np.arange(2049) % 255 + 1)), 7).astype(np.uint8)
    source[1] = 5
    score[2] = 0.5
    for retain in (2049, 1000, 9):
        check(ctx, (FAIR, retain, []), (rows, score, source, None, p64, mask, p32))


# ---- duplicates --------------------------------------------------------------------------------------------------------------------

def test_every_item_held_by_every_source(ctx):
    rng = np.random.default_rng(31)
    cap, w = 1100, 70
    rows, score, source, _, p64, mask, p32 = merged_case(rng, 3, cap, 2, overlap=1.0, pad=0.0, with_count=False)
    # recall 0 orders the items by position; recall 1 too, but with the first w behind the second w.  Round 1: recall 0 takes
    # 0 .. w-1, recall 1 takes w .. 2w-1.  Round 2: each spends its w slots on what the other took — no pick, the walk ends
    source[:] = 0
    mask[:] = 3
    score[:] = -np.arange(cap, dtype=np.float64)
    p64[0], p64[1] = score, score
    p64[1, :, :w] = -(2 * w - 1) - 0.25 - np.arange(w) / (4.0 * w)
    entries = [(0, w), (1, w)]
    got = check(ctx, (SKIP, cap, entries), (rows, score, source, None, p64, mask, p32))
    assert np.all(got[6] == 2 * w)                                   # a round without a pick ended the walk early
    assert np.all(got[2][:, :w] == 0) and np.all(got[2][:, w:2 * w] == 1) and np.array_equal(got[0][:, :2 * w], rows[:, :2 * w])
    full = check(ctx, (REFILL, cap, entries), (rows, score, source, None, p64, mask, p32))
    assert np.all(full[6] == cap)
    # every item in every list, in unrelated orders
    case = merged_case(rng, 3, cap, 3, overlap=1.0)
    for mode in (SKIP, REFILL):
        check(ctx, (mode, cap, [(0, 1), (1, 70), (2, 3)]), case)


def test_no_item_shared_and_unnamed_first_sources(ctx):
    rng = np.random.default_rng(32)
    case = merged_case(rng, 3, 1100, 4, overlap=0.0)
    for mode in (REFILL, SKIP):
        check(ctx, (mode, 800, [(3, 2), (0, 1), (1, 4), (2, 1)]), case)
    # sources 0 and 1 are not named: their items come in only where the mask names 2 or 3, under that name and score
    rows, score, source, count, p64, mask, p32 = merged_case(rng, 3, 1100, 4, overlap=0.5)
    got = check(ctx, (REFILL, 1100, [(3, 2), (2, 1)]), (rows, score, source, count, p64, mask, p32))
    q = 0
    c = int(got[6][q])
    pos = {int(r): i for i, r in enumerate(rows[q]) if r != U64MAX}
    first = np.array([source[q, pos[int(r)]] for r in got[0][q, :c]])
    assert np.count_nonzero(first < 2) > 50 and set(got[2][q, :c].tolist()) == {2, 3}
    moved = np.flatnonzero(first < 2)[0]
    assert got[1][q, moved] == p64[got[2][q, moved], q, pos[int(got[0][q, moved])]]


# ---- the LDS tier ------------------------------------------------------------------------------------------------------------------

def test_lists_inside_and_past_the_lds_tier(ctx):
    rng = np.random.default_rng(41)
    n = ref.LDS_LIST
    # two sources, every item in both lists: both lists hold every real entry
    for cap in (n, n + 1, n + 70, 5000):
        case = merged_case(rng, 2, cap, 2, overlap=1.0, pad=0.0, with_count=False)
        for mode, weights in ((REFILL, (3, 64)), (REFILL, (200, 1)), (SKIP, (65, 64))):
            got = check(ctx, (mode, cap, [(1, weights[0]), (0, weights[1])]), case)
            if mode == REFILL:
                assert np.all(got[6] == cap)                         # the cursors went through the lists' whole length


def test_skip_with_weight_one_at_the_largest_cap(ctx):
    rng = np.random.default_rng(42)
    case = merged_case(rng, 1, 16384, 3, overlap=0.3)
    check(ctx, (SKIP, 16384, [(0, 1), (1, 1), (2, 1)]), case)
    check(ctx, (REFILL, 9000, [(2, 1), (1, 0xFFFFFFFF)]), case)


# ---- hostile keys ------------------------------------------------------------------------------------------------------------------

SPECIAL = np.array([0x7FF8000000000001, 0x7FF4DEADBEEF0001, 0xFFF8000000000123, 0x7FF0000000000000, 0xFFF0000000000000,
                    0x8000000000000000, 0x0000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x0010000000000000,
                    0x3FF0000000000001, 0x3FF0000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF], np.uint64).view(np.float64)


def test_special_values_travel_as_bits(ctx):
    rng = np.random.default_rng(51)
    rows, score, source, count, p64, mask, p32 = merged_case(rng, 2, 1400, 3, overlap=0.5, pad=0.02)
    score[:] = SPECIAL[rng.integers(0, SPECIAL.size, score.shape)]
    p64[:] = SPECIAL[rng.integers(0, SPECIAL.size, p64.shape)]
    f32 = np.array([0x7FC00001, 0xFFC12345, 0x7FA00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x3F800001], np.uint32).view(np.float32)
    p32[:] = f32[rng.integers(0, f32.size, p32.shape)]
    for conf in ((REFILL, 1400, [(0, 2), (1, 1), (2, 3)]), (SKIP, 900, [(2, 2), (0, 1)]), (FAIR, 1400, []), (FAIR, 77, [])):
        got = check(ctx, conf, (rows, score, source, count, p64, mask, p32), optional=True)
        if conf[1] == 1400:                                          # everything real is kept: every special value is among the scores
            assert {0x8000000000000000, 0, 0x7FF4DEADBEEF0001, 1} <= set(got[1].view(np.uint64)[0, :int(got[6][0])].tolist())


def test_padding_in_the_middle_and_the_counts(ctx):
    rng = np.random.default_rng(52)
    rows, score, source, _, p64, mask, p32 = merged_case(rng, 4, 1100, 4, pad=0.0)
    rows[:, 5:900:3] = U64MAX                                        # padding in the middle of every list
    rows[3] = U64MAX                                                 # request 3: padding only
    source[1, 10:700:7] = 200                                        # sources past the limit are padding too
    count = np.array([0, 1100, 1023, 1100], np.uint32)               # d_count[q] = 0 and = cap
    for conf in ((REFILL, 700, [(0, 1), (3, 2), (1, 5)]), (SKIP, 700, [(2, 3), (0, 1)]), (FAIR, 700, [])):
        got = check(ctx, conf, (rows, score, source, count, p64, mask, p32))
        assert got[6][0] == 0 and got[6][3] == 0 and np.all(got[0][[0, 3]] == U64MAX) and np.all(got[2][[0, 3]] == 0xFF)
        assert np.all(got[1].view(np.uint64)[[0, 3]] == ref.NEG_INF_BITS) and np.all(got[3].view(np.uint64)[:, [0, 3]] == ref.NAN_BITS)
        assert not np.any(got[4][[0, 3]]) and not np.any(got[5].view(np.uint32)[:, [0, 3]])
        check(ctx, conf, (rows, score, source, None, p64, mask, p32))
        big = np.array([5000, 1101, 0xFFFFFFFF, 7], np.uint32)       # a count beyond cap is cap
        check(ctx, conf, (rows, score, source, big, p64, mask, p32))


# ---- behind the fan-in --------------------------------------------------------------------------------------------------------------

def test_blend_over_a_fanin_merge(ctx):
    rng = np.random.default_rng(61)
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
        sc = rng.standard_normal((nq, k))
        src.append((rows, sc if i == 1 else sc.astype(np.float32)))
        seen = rows if seen is None else np.concatenate([seen, rows], axis=1)
    m_rows, m_score, m_source, m_planes, m_mask, m_count = ctx.fanin_merge(src)
    w = fanin_ref.merge(src)
    for conf in ((REFILL, 300, [(0, 3), (1, 2), (2, 1)]), (SKIP, 300, [(2, 1), (1, 1), (0, 1)]), (FAIR, 300, [])):
        got = ctx.candidates_blend(conf, m_rows, m_score, m_source, m_count, m_planes, m_mask)
        ref.same(got, ref.blend(conf, w[0], w[1], w[2], w[5], w[3], w[4]))
        assert np.all(got[6] == 300)
    # REFILL, nothing dry: every round is 3 x source 0, 2 x source 1, 1 x source 2; some items came in under a later recall's name
    got = ctx.candidates_blend((REFILL, 300, [(0, 3), (1, 2), (2, 1)]), m_rows, m_score, m_source, m_count, m_planes, m_mask)
    assert np.all(got[2] == np.tile(np.array([0, 0, 0, 1, 1, 2], np.uint8), 50))
    pos = {int(r): i for i, r in enumerate(m_rows[0, :int(m_count[0])])}
    assert any(m_source[0, pos[int(r)]] != s for r, s in zip(got[0][0], got[2][0]))


def test_argument_errors_leave_the_context_usable(ctx):
    d = ctx.malloc(1 << 16)
    ok = (REFILL, 4, [(0, 1), (1, 1)])

    def call(conf=ok, nq=1, cap=16, **kw):
        a = dict(d_rows=d, d_score=d, d_source=d, d_count=0, d_planes_f64=0, n_f64=0, d_source_mask=0, d_planes_f32=0, n_f32=0,
                 d_out_rows=d, d_out_score=d, d_out_source=d, d_out_planes_f64=0, d_out_source_mask=0, d_out_planes_f32=0, d_out_count=d)
        a.update(kw)
        ctx.candidates_blend_dev(conf, nq, cap, **a)

    refused = [dict(conf=(3, 4, [(0, 1)])), dict(conf=(REFILL, 0, [(0, 1)])), dict(conf=(FAIR, 0, [])), dict(conf=(SKIP, 4, [])),
               dict(conf=(REFILL, 4, [(8, 1)])), dict(conf=(REFILL, 4, [(1, 1), (1, 2)])), dict(conf=(SKIP, 4, [(0, 0), (1, 0)])),
               dict(conf=(REFILL, 4, [(s % 8, 1) for s in range(9)])), dict(nq=0), dict(nq=257), dict(cap=0), dict(cap=16385),
               dict(d_rows=0), dict(d_score=0), dict(d_out_rows=0), dict(d_out_score=0), dict(d_out_count=0),
               dict(d_source=0, d_out_source=0), dict(d_out_source=0),
               dict(d_source_mask=d, d_out_source_mask=d), dict(d_source_mask=d, d_out_source_mask=d, d_planes_f64=d, d_out_planes_f64=d, n_f64=1),
               dict(d_planes_f64=d, n_f64=1), dict(d_planes_f64=d, d_out_planes_f64=d, n_f64=0), dict(d_planes_f64=d, d_out_planes_f64=d, n_f64=9),
               dict(d_planes_f32=d, d_out_planes_f32=d, n_f32=9), dict(d_out_planes_f32=d, n_f32=1), dict(d_source_mask=d), dict(d_out_source_mask=d)]
    for kw in refused:
        with pytest.raises(PgError) as ei:
            call(**kw)
        assert ei.value.code in (-1, -4) and "pg_candidates_blend_dev" in str(ei.value), kw
    # what the checks of the candidate lists answer, code and text (recorded from the build before cand_lists.hpp stated them once)
    for kw, code, text in ((dict(d_out_source=0), -1, "d_source / d_source_mask and their outputs come in pairs"),
                           (dict(d_source_mask=d), -1, "d_source / d_source_mask and their outputs come in pairs"),
                           (dict(d_planes_f64=d, n_f64=1), -1, "a carried plane set and its output come in pairs"),
                           (dict(d_planes_f64=d, d_out_planes_f64=d, n_f64=0), -1, "a carried plane set holds 1..8 planes"),
                           (dict(d_planes_f64=d, d_out_planes_f64=d, n_f64=9), -1, "a carried plane set holds 1..8 planes"),
                           (dict(d_rows=0), -1, "NULL argument"), (dict(nq=0), -1, "nq=0 must be in [1,256]"),
                           (dict(cap=0), -4, "cap=0 unsupported (1..16384)")):
        with pytest.raises(PgError) as ei:
            call(**kw)
        assert ei.value.code == code and str(ei.value).endswith(": pg_candidates_blend_dev: " + text), kw
    ctx.free(d)
    check(ctx, ok, merged_case(np.random.default_rng(15), 2, 16, 2))


# ---- the host mirror ----------------------------------------------------------------------------------------------------------------

import ctypes as C       # noqa: E402
import json              # noqa: E402
import os                # noqa: E402

from test_blend_cpu import GOLDEN, MIRROR_CONFIG       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
        assert r, L.ph_last_error()
        return json.loads(r)["items"]
    yield run
    L.ph_engine_destroy(h)


def test_snake_filter_through_the_mirror(mirror):
    case = {c["name"]: c for c in GOLDEN}["snake_recall_not_configured"]          # snake_filter_test.go:385-460: weights 1 / 2 / 3, retain 20
    items = [{"id": "item_%d" % i, "score": s, "retrieve_id": case["recalls"][r]} for i, s, r in case["items"]]
    got = mirror("snake", items)
    assert [x["item_id"] for x in got] == ["item_%d" % i for i in case["expect_ids"]]
    assert [x["retrieve_id"] for x in got] == [case["recalls"][s] for s in case["expect_sources"]]
    # items that UniqueFilter found in several recalls: reached through a later recall, they take its name and score
    rng = np.random.default_rng(71)
    names = ["recall_A", "recall_B", "recall_C", "recall_D"]
    rows, score, source, _, p64, mask, _ = merged_case(rng, 1, 300, 4, overlap=0.4, pad=0.0, with_count=False)
    items = []
    for i in range(300):
        it = {"id": "x%d" % i, "score": float(score[0, i]), "retrieve_id": names[source[0, i]]}
        if bin(int(mask[0, i])).count("1") > 1:
            it["recall_scores"] = {names[b]: float(p64[b, 0, i]) for b in range(4) if (int(mask[0, i]) >> b) & 1}
        items.append(it)
    ids = np.arange(300, dtype=np.uint64).reshape(1, -1)
    for name, conf in (("snake", (REFILL, 20, [(0, 1), (1, 2), (2, 3)])), ("snake_skip", (SKIP, 20, [(2, 2), (0, 0)]))):
        want = ref.blend(conf, ids, score, source, None, p64, mask)
        got = mirror(name, items)
        n = int(want[6][0])
        assert [x["item_id"] for x in got] == ["x%d" % i for i in want[0][0, :n]]
        assert [x["retrieve_id"] for x in got] == [names[s] for s in want[2][0, :n]]
        assert [x["score"] for x in got] == want[1][0, :n].tolist()
        assert any(x["retrieve_id"] != names[source[0, int(x["item_id"][1:])]] for x in got)
    assert mirror("snake", []) == []


def test_completely_fair_count_filter_through_the_mirror(mirror):
    cases = {c["name"]: c for c in GOLDEN}
    case = cases["fair_retain_10"]                                    # completely_fair_count_filter_test.go:11-55
    items = [{"id": "item_%d" % i, "score": s, "retrieve_id": case["recalls"][r]} for i, s, r in case["items"]]
    got = mirror("fair", items)                                       # (recall1 / recall2 are no recalls of the engine: dealt out all the same)
    assert [x["item_id"] for x in got] == ["item_%d" % i for i in case["expect_ids"]]
    assert [x["retrieve_id"] for x in got] == [case["recalls"][s] for s in case["expect_sources"]]
    assert [x["score"] for x in got] == [case["items"][i][1] for i in case["expect_ids"]]
