"""GPU tests of DiversityAdjustCountFilter on the device (csrc/classcut.hip: pg_classcut_masks_dev,
pg_candidates_classcut_dev, the one-request entry and the host mirror's filter) against tests/classcut_ref.py: every output array
by bits, padding and counts included.  Sizes sit on the kernels' edges: a wave of 64 lanes, the cut's chunk of 1 024 positions,
the mask kernel's workgroup of 256, the largest cap of 16 384.  Every output buffer carries a guard behind it."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import classcut_ref as ref
import pairec_amd as pa
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX, ACC = pa.TRIM_FIX, pa.TRIM_ACCUMULATE
RECALLS = ["u2i", "hot", "i2i"]
S = 6000                                        # store rows; candidates' rows reach S + S / 8: some lie outside
GUARD = 64


@pytest.fixture(scope="module")
def store(ctx):
    """one feature store for the whole module: cat, brand int32, big int64, price f32, w f64 — and their host copies"""
    rng = np.random.default_rng(77)
    host = {"cat": rng.integers(0, 10, S).astype(np.int32), "brand": rng.integers(0, 6, S).astype(np.int32),
            "big": rng.integers(-4, 5, S).astype(np.int64), "price": rng.integers(0, 9, S).astype(np.float32) / 2,
            "w": rng.integers(-3, 4, S).astype(np.float64)}
    host["big"][::7] = 2**53 + 1
    host["price"][::11] = np.nan
    host["w"][::13] = -0.0
    host["w"][5::13] = np.inf
    dt = {"cat": pa.F_I32, "brand": pa.F_I32, "big": pa.F_I64, "price": pa.F_F32, "w": pa.F_F64}
    fs = pa.Features(ctx, S)
    for k, v in host.items():
        fs.set_column(k, dt[k], v)
    yield fs, host, [(k, dt[k]) for k in host]
    fs.destroy()


def gather(host, rows):
    """the store's values at `rows`, and which rows lie inside"""
    inside = rows < S
    idx = np.where(inside, rows, 0).astype(np.int64)
    return {k: v[idx] for k, v in host.items()}, inside


# the classes of the size sweep: govaluate text and its numpy twin over (gathered columns, inside, score, source)
CLASSES = [
    ("cat == 3 || cat in (5, 7)", lambda c, i, s, r: i & ((c["cat"] == 3) | (c["cat"] == 5) | (c["cat"] == 7))),
    ("recall_name == 'u2i' && brand < 4", lambda c, i, s, r: (r == 0) & i & (c["brand"] < 4)),
    ("recall_score >= 2 && !(brand % 2 == 1)", lambda c, i, s, r: (s >= 2) & i & ~(c["brand"] % 2 == 1)),
    ("price * 2 > 5 || recall_name in ('hot', 'nobody')", lambda c, i, s, r: i & ((c["price"].astype(np.float64) * 2 > 5) | (r == 1))),
    ("recall_name != 'i2i' || w < 0", lambda c, i, s, r: (r != 2) | (i & (c["w"] < 0))),
    ("big >= 9007199254740992 || -w ** 2 > 3", lambda c, i, s, r: i & ((c["big"].astype(np.float64) >= 9007199254740992.0) | (c["w"] * c["w"] > 3))),
    ("recall_score == recall_score", lambda c, i, s, r: s == s),
    ("cat + brand <= 6 && recall_score != 1", lambda c, i, s, r: i & (c["cat"] + c["brand"] <= 6) & (s != 1)),
]


def class_masks(host, rows, score, source, n_classes):
    cols, inside = gather(host, rows)
    m = np.zeros(rows.shape, np.uint8)
    with np.errstate(all="ignore"):
        for c in range(n_classes):
            m |= CLASSES[c][1](cols, inside, score, source).astype(np.uint8) << c
    real = rows != ref.PAD_ROW
    return np.where(real, m, 0).astype(np.uint8)


def make_case(seed, nq, cap, optional=(True, True, True, True, True)):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, S + S // 8, (nq, cap)).astype(np.uint64)
    rows[rng.random((nq, cap)) < 0.05] = ref.PAD_ROW                              # padding anywhere
    score = rng.integers(0, 5, (nq, cap)).astype(np.float64)                     # many ties
    sp = rng.random((nq, cap)) < 0.03
    score[sp] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0]), int(sp.sum()))
    source = rng.integers(0, 5, (nq, cap)).astype(np.uint8)                      # 3 and 4 are >= n_recalls
    count = rng.integers(cap // 2, cap + 1, nq).astype(np.uint32) if optional[1] else None
    if count is not None and nq > 2:
        count[1] = 0
    p64 = rng.standard_normal((2, nq, cap)) if optional[2] else None
    smask = rng.integers(0, 16, (nq, cap)).astype(np.uint32) if optional[3] else None
    p32 = rng.standard_normal((1, nq, cap)).astype(np.float32) if optional[4] else None
    n = int(rng.integers(1, ref.MAX_CLASSES + 1))
    if cap >= 2049:
        n = max(n, 5)                            # (several classes walk several chunks)
    rules, last = [], None
    for _ in range(n):
        ty = int(rng.integers(0, 2))
        cnt = int(rng.integers(0, max(2, cap // 3)))
        if ty == ACC and last is not None:
            cnt = max(cnt, last)
        last = cnt if ty == ACC else None
        rules.append((ty, cnt))
    return dict(rows=rows, score=score, source=source, count=count, planes_f64=p64, source_mask=smask, planes_f32=p32, rules=rules)


def run_dev(ctx, cc, fs, case, keep_source=True):
    """pg_candidates_classcut_dev on the case's arrays with a guard behind every output → the outputs in candidates_trim's order"""
    rows, score = case["rows"], case["score"]
    nq, cap = rows.shape
    w = cc.out_cap(cap)
    source = case["source"] if keep_source else None
    ins = [rows, score, source, case["count"], case["planes_f64"], case["source_mask"], case["planes_f32"]]
    n64 = 0 if ins[4] is None else ins[4].shape[0]
    n32 = 0 if ins[6] is None else ins[6].shape[0]
    outs = [np.empty((nq, w), np.uint64), np.empty((nq, w), np.float64), None if source is None else np.empty((nq, w), np.uint8),
            None if ins[4] is None else np.empty((n64, nq, w), np.float64), None if ins[5] is None else np.empty((nq, w), np.uint32),
            None if ins[6] is None else np.empty((n32, nq, w), np.float32), np.empty(nq, np.uint32)]
    bufs = []
    try:
        d_in = [0 if a is None else ctx.to_device(np.ascontiguousarray(a)) for a in ins]
        bufs += d_in
        d_out = []
        for a in outs:
            if a is None:
                d_out.append(0)
                continue
            p = ctx.malloc(a.nbytes + GUARD)
            ctx.h2d(p + a.nbytes, np.full(GUARD, 0xA5, np.uint8))
            d_out.append(p)
        bufs += d_out
        ctx.candidates_classcut_dev(cc, fs, nq, cap, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], n64, d_in[5], d_in[6], n32, *d_out)
        ctx.synchronize()
        for a, p in zip(outs, d_out):
            if a is None:
                continue
            if a.nbytes:
                ctx.d2h(a, p)
            g = np.empty(GUARD, np.uint8)
            ctx.d2h(g, p + a.nbytes)
            assert (g == 0xA5).all(), "a write behind an output"
    finally:
        for b in bufs:
            if b:
                ctx.free(b)
    return tuple(outs)


def want_of(case, mask, keep_source=True):
    return ref.classcut(case["rules"], case["rows"], case["score"], mask, case["source"] if keep_source else None, case["count"], case["planes_f64"],
                        case["source_mask"], case["planes_f32"])


def assert_same(got, want, what=""):
    for j, (g, w) in enumerate(zip(got, want)):
        assert ref.same_bits(g, w), (what, j)


SIZES = [(nq, cap) for cap in (1, 63, 64, 65, 1023, 1024, 1025, 2049, 16384) for nq in (1, 3, 256) if nq < 256 or cap <= 1025]


@pytest.mark.parametrize("nq,cap", SIZES, ids=["nq%d-cap%d" % s for s in SIZES])
def test_sizes_by_bits(ctx, store, nq, cap):
    fs, host, decl = store
    case = make_case(1000 * nq + cap, nq, cap)
    n = len(case["rules"])
    cc = pa.classcut_compile([(CLASSES[c][0], ty, cnt) for c, (ty, cnt) in enumerate(case["rules"])], decl, RECALLS)
    try:
        got = run_dev(ctx, cc, fs, case)
        masks = ctx.classcut_masks(cc, fs, case["rows"], case["score"], case["source"], case["count"])
    finally:
        cc.free()
    mask = class_masks(host, case["rows"], case["score"], case["source"], n)
    valid = np.arange(cap)[None, :] < (case["count"][:, None] if case["count"] is not None else cap)
    assert np.array_equal(masks, np.where(valid, mask, 0))                          # the mask kernel alone: padding gets 0
    assert_same(got, want_of(case, mask))


def test_numpy_twins_equal_the_tree_evaluator(store):
    """the size sweep's vectorised masks are the tree evaluator's (no GPU work: the reference is checked once)"""
    _, host, _ = store
    col, num = (lambda x: ("col", x)), (lambda v: ("num", v))
    trees = [("or", ("cmp", "==", col("cat"), num(3)), ("in", col("cat"), [5, 7])),
             ("and", ("rn_eq", "u2i"), ("cmp", "<", col("brand"), num(4))),
             ("and", ("cmp", ">=", ("score",), num(2)), ("not", ("cmp", "==", ("bin", "%", col("brand"), num(2)), num(1)))),
             ("or", ("cmp", ">", ("bin", "*", col("price"), num(2)), num(5)), ("rn_in", ["hot", "nobody"])),
             ("or", ("rn_ne", "i2i"), ("cmp", "<", col("w"), num(0))),
             ("or", ("cmp", ">=", col("big"), num(9007199254740992)), ("cmp", ">", ("bin", "**", ("neg", col("w")), num(2)), num(3))),
             ("cmp", "==", ("score",), ("score",)),
             ("and", ("cmp", "<=", ("bin", "+", col("cat"), col("brand")), num(6)), ("cmp", "!=", ("score",), num(1)))]
    assert [ref.render(t).replace("(", "").replace(")", "") for t in trees] == \
           [x[0].replace("(", "").replace(")", "").replace('"', "'").replace("recall_name != 'i2i'", 'recall_name != "i2i"') for x in CLASSES]
    case = make_case(5, 1, 700)
    cols, inside = gather(host, case["rows"][0])
    want = ref.masks(trees, 700, cols, inside, case["score"][0], case["source"][0], RECALLS)
    assert np.array_equal(class_masks(host, case["rows"], case["score"], case["source"], 8)[0], np.where(case["rows"][0] != ref.PAD_ROW, want, 0))


# ---- the cut kernel's seams ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def member_store(ctx):
    """rows 0 .. 4095: column mK holds bit K of a membership table the seam tests set per case"""
    n = 4096
    fs = pa.Features(ctx, n)
    yield fs, n
    fs.destroy()


def run_seam(ctx, member_store, rules, members, cap, score=None, nq=1):
    """position p of every request is row p; members[c]: the positions in class c; scores descend by position unless given"""
    fs, n = member_store
    assert cap <= n
    mask = np.zeros(cap, np.uint8)
    for c, pos in enumerate(members):
        col = np.zeros(n, np.int32)
        col[np.asarray(pos, dtype=np.int64)] = 1
        fs.set_column("m%d" % c, pa.F_I32, col)
        mask[np.asarray(pos, dtype=np.int64)] |= np.uint8(1 << c)
    ctx.synchronize()
    case = dict(rows=np.tile(np.arange(cap, dtype=np.uint64), (nq, 1)),
                score=np.tile(np.arange(cap, 0, -1, dtype=np.float64) if score is None else np.asarray(score, np.float64), (nq, 1)),
                source=np.zeros((nq, cap), np.uint8), count=None, planes_f64=np.tile(np.arange(cap, dtype=np.float64), (1, nq, 1)),
                source_mask=None, planes_f32=None, rules=rules)
    cc = pa.classcut_compile([("m%d > 0" % c, ty, cnt) for c, (ty, cnt) in enumerate(rules)], [("m%d" % c, pa.F_I32) for c in range(len(rules))], RECALLS)
    try:
        got = run_dev(ctx, cc, fs, case)
    finally:
        cc.free()
    assert_same(got, want_of(case, np.tile(mask, (nq, 1))))
    return got[0][0, :got[6][0]].tolist()


@pytest.mark.parametrize("limit", [64, 65, 128, 129, 1024, 1025, 2048, 2049])
def test_limit_on_a_wave_and_a_chunk_boundary(ctx, member_store, limit):
    """a window that ends exactly on a wave's / a chunk's last lane, and one member past it; an earlier class holds a few places"""
    cap = 3000
    kept = run_seam(ctx, member_store, [(FIX, 3), (FIX, limit)], [[0, 63, 64], list(range(cap))], cap)
    assert kept == [0, 63, 64] + [p for p in range(limit) if p not in (0, 63, 64)]


def test_window_over_three_chunks_with_every_second_member_taken(ctx, member_store):
    cap = 4000
    kept = run_seam(ctx, member_store, [(FIX, cap), (ACC, 2500)], [list(range(0, cap, 2)), list(range(cap))], cap, nq=2)
    assert kept == list(range(0, cap, 2)) + list(range(1, 2500, 2))


def test_sparse_members_across_chunks(ctx, member_store):
    """members every 37th position: the window's end lies in the third chunk although the limit is small"""
    cap = 4000
    members = list(range(5, cap, 37))
    kept = run_seam(ctx, member_store, [(FIX, 70)], [members], cap)
    assert kept == members[:70] and members[69] > 2048


def test_last_place_of_the_window_is_taken(ctx, member_store):
    kept = run_seam(ctx, member_store, [(FIX, 1), (FIX, 10), (FIX, 2)], [[9], list(range(30)), list(range(8, 30))], 100)
    assert kept == [9, 0, 1, 2, 3, 4, 5, 6, 7, 8]          # class 1: nine picks, its tenth place is position 9; class 2: its window [8, 9] is taken


def test_accumulator_reaches_its_count_mid_class(ctx, member_store):
    cap = 2100
    kept = run_seam(ctx, member_store, [(ACC, 1030), (FIX, 2), (ACC, 1100), (ACC, 1100)],
                    [list(range(0, 2060, 2)), [1, 3], list(range(1, cap, 2)), list(range(cap))], cap)
    # class 0 takes 1030 evens; class 2's limit is 1100 - 1030 = 70 places, of which positions 1 and 3 are taken; class 3's limit is 2
    odd = [p for p in range(1, 140, 2)]
    assert kept == list(range(0, 2060, 2)) + [1, 3] + [p for p in odd if p not in (1, 3)]


@pytest.mark.parametrize("kind", ["equal", "nan", "zeros", "inf"])
def test_scores(ctx, member_store, kind):
    cap = 1500
    rng = np.random.default_rng(4)
    score = {"equal": np.full(cap, 2.5), "nan": np.where(rng.random(cap) < 0.5, np.nan, rng.integers(0, 3, cap).astype(np.float64)),
             "zeros": rng.choice(np.array([0.0, -0.0]), cap), "inf": rng.choice(np.array([np.inf, -np.inf, 0.0, np.nan]), cap)}[kind]
    members = [sorted(rng.choice(cap, 900, replace=False).tolist()), sorted(rng.choice(cap, 900, replace=False).tolist())]
    kept = run_seam(ctx, member_store, [(FIX, 400), (ACC, 700)], members, cap, score=score)
    if kind in ("equal", "zeros"):                          # ties keep input position; -0.0 equals +0.0
        taken = members[0][:400]
        assert kept == taken + [p for p in members[1][:700] if p not in set(taken)]


# ---- the mask kernel alone ----------------------------------------------------------------------------------------------------

def test_masks_sixteen_columns_a_64_operation_program_and_rows_outside(ctx):
    rng = np.random.default_rng(8)
    rows_in_store, n = 500, 64 * 9 + 5
    dts = [np.int32, np.int64, np.float32, np.float64]
    host = {"k%d" % j: rng.integers(-3, 4, rows_in_store).astype(dts[j % 4]) for j in range(16)}
    host["k2"][::5] = np.nan
    host["k1"][::9] = 2**53 + 1
    fcode = {np.int32: pa.F_I32, np.int64: pa.F_I64, np.float32: pa.F_F32, np.float64: pa.F_F64}
    decl = [("k%d" % j, fcode[dts[j % 4]]) for j in range(16)]
    col = lambda j: ("col", "k%d" % j)                                               # noqa: E731
    t16 = col(0)
    for j in range(1, 16):
        t16 = ("bin", "+", t16, col(j))
    t16 = ("cmp", ">", t16, ("num", 2))
    t64 = col(0)
    for j in range(1, 31):
        t64 = ("bin", "-" if j % 3 else "+", t64, col(j % 16) if j % 2 else ("num", j))
    t64 = ("not", ("cmp", "<=", t64, ("score",)))
    assert ref.shape(t64) == (ref.MAX_OPS, 2)
    deep = ("or", ("cmp", ">", col(3), ("bin", "*", col(4), ("bin", "+", col(5), ("bin", "-", col(6), ("bin", "/", col(7), ("bin", "%", col(8), ("num", 3))))))),
            ("rn_in", ["hot", "i2i"]))
    assert ref.shape(deep)[1] == 7
    trees = [t16, t64, deep]
    fs = pa.Features(ctx, rows_in_store)
    for k, v in host.items():
        fs.set_column(k, dict(decl)[k], v)
    # request q puts its rows outside the store at lanes l with (l + q) % 3 == 0: every wave position is outside somewhere
    nq = 3
    rows = rng.integers(0, rows_in_store, (nq, n)).astype(np.uint64)
    for q in range(nq):
        rows[q, (np.arange(n) + q) % 3 == 0] = rows_in_store + q
    rows[0, 7] = ref.PAD_ROW
    score = rng.integers(-2, 3, (nq, n)).astype(np.float64)
    source = rng.integers(0, 4, (nq, n)).astype(np.uint8)
    count = np.array([n, n - 70, 0], np.uint32)
    cc = pa.classcut_compile([(ref.render(t), FIX, 1) for t in trees], decl, RECALLS)
    try:
        got = ctx.classcut_masks(cc, fs, rows, score, source, count)
    finally:
        cc.free()
        fs.destroy()
    for q in range(nq):
        inside = rows[q] < rows_in_store
        cols = {k: v[np.where(inside, rows[q], 0).astype(np.int64)] for k, v in host.items()}
        want = ref.masks(trees, n, cols, inside, score[q], source[q], RECALLS)
        want[(rows[q] == ref.PAD_ROW) | (np.arange(n) >= count[q])] = 0
        assert np.array_equal(got[q], want), q
        assert q == 2 or 0 < int((want & 1).sum()) < n


# ---- chained into the trim, optional arrays, the one-request entry, refusals ----------------------------------------------------

def test_outputs_feed_the_trim_unchanged(ctx, store):
    fs, host, decl = store
    case = make_case(31, 3, 1500)
    case["rules"] = [(FIX, 200), (ACC, 500), (ACC, 900)]
    cc = pa.classcut_compile([(CLASSES[c][0], ty, cnt) for c, (ty, cnt) in enumerate(case["rules"])], decl, RECALLS)
    try:
        got = run_dev(ctx, cc, fs, case)
    finally:
        cc.free()
    keep = 333
    trimmed = ctx.candidates_trim([(pa.TRIM_ANY, FIX, keep)], got[0], got[1], got[2], got[6], got[3], got[4], got[5])
    want = ref.classcut([(FIX, keep)], got[0], got[1], np.ones(got[0].shape, np.uint8), got[2], got[6], got[3], got[4], got[5])
    assert_same(trimmed, want)
    assert trimmed[6].tolist() == [min(keep, int(c)) for c in got[6]]


OPTIONAL = [(False,) * 5] + [tuple(j == k for j in range(5)) for k in range(5)]


@pytest.mark.parametrize("optional", OPTIONAL, ids=["none", "source", "count", "planes_f64", "source_mask", "planes_f32"])
def test_optional_arrays(ctx, store, optional):
    fs, host, decl = store
    case = make_case(17, 2, 1100, optional)
    case["rules"] = [(FIX, 100), (ACC, 300)]
    texts = [CLASSES[0][0], CLASSES[7][0]] if not optional[0] else [CLASSES[0][0], CLASSES[1][0]]      # without a source nothing may read recall_name
    cc = pa.classcut_compile([(t, ty, cnt) for t, (ty, cnt) in zip(texts, case["rules"])], decl, RECALLS)
    try:
        got = run_dev(ctx, cc, fs, case, keep_source=optional[0])
    finally:
        cc.free()
    cols, inside = gather(host, case["rows"])
    with np.errstate(all="ignore"):
        second = CLASSES[1][1] if optional[0] else CLASSES[7][1]
        mask = (CLASSES[0][1](cols, inside, case["score"], case["source"]).astype(np.uint8) |
                (second(cols, inside, case["score"], case["source"]).astype(np.uint8) << 1))
    assert_same(got, want_of(case, mask, keep_source=optional[0]))


def test_one_request_entry(ctx, store):
    fs, host, decl = store
    case = make_case(9, 1, 777, (True, False, False, False, False))
    case["rules"] = [(FIX, 50), (ACC, 120), (ACC, 200)]
    cc = pa.classcut_compile([(CLASSES[c][0], ty, cnt) for c, (ty, cnt) in enumerate(case["rules"])], decl, RECALLS)
    try:
        r, s, src, cnt = ctx.candidates_classcut_one(cc, fs, case["rows"][0], case["score"][0], case["source"][0])
        assert ctx.candidates_classcut_one(cc, fs, np.zeros(0, np.uint64), np.zeros(0))[3] == 0
    finally:
        cc.free()
    want = want_of(case, class_masks(host, case["rows"], case["score"], case["source"], 3))
    assert cnt == want[6][0] and ref.same_bits(r, want[0][0]) and ref.same_bits(s, want[1][0]) and ref.same_bits(src, want[2][0])


def test_context_stays_usable_after_each_refusal(ctx, store):
    fs, host, decl = store
    case = make_case(3, 2, 300)
    case["rules"] = [(FIX, 40), (ACC, 90)]
    mask = class_masks(host, case["rows"], case["score"], case["source"], 2)
    cc = pa.classcut_compile([(CLASSES[c][0], ty, cnt) for c, (ty, cnt) in enumerate(case["rules"])], decl, RECALLS)
    other = pa.Features(ctx, 10)
    other.set_column("cat", pa.F_I64, np.zeros(10, np.int64))
    other.set_column("brand", pa.F_I32, np.zeros(10, np.int32))
    lacking = pa.Features(ctx, 10)
    lacking.set_column("cat", pa.F_I32, np.zeros(10, np.int32))
    d = ctx.malloc(1 << 16)

    def good():
        assert_same(run_dev(ctx, cc, fs, case), want_of(case, mask))

    try:
        good()
        for call, code, word in [
                (lambda: run_dev(ctx, cc, fs, case, keep_source=False), -1, "recall_name"),
                (lambda: ctx.classcut_masks_dev(cc, fs, 2, 300, d, d, 0, 0, d), -1, "recall_name"),
                (lambda: ctx.candidates_classcut_dev(cc, fs, 1, 16385, d, d, d, 0, 0, 0, 0, 0, 0, d, d, d, 0, 0, 0, d), -4, "cap=16385"),
                (lambda: ctx.candidates_classcut_dev(cc, fs, 257, 8, d, d, d, 0, 0, 0, 0, 0, 0, d, d, d, 0, 0, 0, d), -1, "nq=257"),
                (lambda: ctx.candidates_classcut_dev(cc, fs, 1, 8, d, d + 4096, d + 8192, 0, 0, 0, 0, 0, 0, d + 32, d + 12288, d + 16384, 0, 0, 0, d + 20480), -1, "overlaps"),
                (lambda: ctx.candidates_classcut_dev(cc, fs, 1, 8, d, d + 4096, d + 8192, 0, 0, 0, 0, 0, 0, d + 12288, d + 16384, 0, 0, 0, 0, d + 20480), -1, "pairs"),
                (lambda: run_dev(ctx, cc, other, case), -1, "dtype"),
                (lambda: run_dev(ctx, cc, lacking, case), -1, '"brand"'),
                (lambda: ctx.candidates_classcut_dev(cc, 0, 1, 8, d, d + 4096, d + 8192, 0, 0, 0, 0, 0, 0, d + 12288, d + 16384, d + 20480, 0, 0, 0, d + 24576), -1, "feature store"),
        ]:
            with pytest.raises(PgError) as e:
                call()
            assert e.value.code == code and word in str(e.value), str(e.value)
            good()
    finally:
        ctx.free(d)
        cc.free()
        other.destroy()
        lacking.destroy()


# ---- the host mirror ------------------------------------------------------------------------------------------------------------

MIRROR_ROWS = 2000
MIRROR_CONFIG = {
    "RunMode": "product", "AlgoConfs": [], "RecallConfs": [],
    "SceneConfs": {"feed": {"default": {"RecallNames": ["u2i", "hot"]}}},
    "UserDefineConfs": {"pairec_gpu": {
        "Device": 0, "Table": {"Rows": MIRROR_ROWS, "Dim": 128, "IdPrefix": "item_", "SyntheticSeed": 1},
        "Recalls": [{"Name": n, "Kind": "vector", "RecallCount": 50, "RecallAlgo": "gpu_faiss", "ItemType": "video"} for n in ("u2i", "hot")],
        "Algorithms": [{"Name": "gpu_faiss", "Kind": "faiss"}],
        "Filters": [{"Name": "classes", "FilterType": "DiversityAdjustCountFilter",
                     "AdjustCountConfs": [{"Expression": "recall_name == 'u2i' && category == 3", "Count": 10, "Type": "fix"},
                                          {"Expression": "[recall_score] > 0.5 || !(brand in (1, 2))", "Count": 20, "Type": "accumulator"},
                                          {"Expression": "recall_name in ('u2i', \"hot\")", "Count": 40, "Type": "accumulator"}]},
                    {"Name": "no_such_column", "FilterType": "DiversityAdjustCountFilter",
                     "AdjustCountConfs": [{"Expression": "colour == 3", "Count": 10, "Type": "fix"}]}],
        "FilterNames": {"feed": ["classes"]}}},
}


def test_filter_through_the_mirror():
    H = C.CDLL(os.environ.get("PH_HOST_LIB") or os.path.join(ROOT, "pairec_amd", "libpairec_host.so"))
    H.ph_last_error.restype = C.c_char_p
    H.ph_engine_create.restype = C.c_void_p
    H.ph_engine_create.argtypes = [C.c_char_p]
    H.ph_engine_destroy.argtypes = [C.c_void_p]
    H.ph_engine_set_feature_column.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
    H.ph_engine_filter.restype = C.c_char_p
    H.ph_engine_filter.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]
    h = H.ph_engine_create(json.dumps(MIRROR_CONFIG).encode())
    assert h, H.ph_last_error()
    try:
        rng = np.random.default_rng(6)
        cols = {"category": rng.integers(0, 6, MIRROR_ROWS).astype(np.int32), "brand": rng.integers(0, 5, MIRROR_ROWS).astype(np.int32)}
        for name, a in cols.items():
            assert H.ph_engine_set_feature_column(h, name.encode(), a.ctypes.data_as(C.c_void_p), MIRROR_ROWS) == 0, H.ph_last_error()
        ids = ["item_%d" % r for r in rng.choice(MIRROR_ROWS, 400, replace=False)] + ["stranger_1", "item_99999999"]
        rng.shuffle(ids)
        names = ["u2i", "hot", "elsewhere"]
        items = [{"id": i, "score": float(rng.integers(0, 5)) / 4, "retrieve_id": names[int(rng.integers(0, 3))]} for i in ids]
        r = H.ph_engine_filter(h, b"classes", json.dumps(items).encode(), b"{}")
        assert r, H.ph_last_error()
        got = [x["item_id"] for x in json.loads(r)["items"]]
        n = len(items)
        rows = np.array([int(i[5:]) if i.startswith("item_") and int(i[5:]) < MIRROR_ROWS else MIRROR_ROWS for i in ids], dtype=np.int64)
        inside = rows < MIRROR_ROWS
        c = {k: v[np.where(inside, rows, 0)] for k, v in cols.items()}
        col, num = (lambda x: ("col", x)), (lambda v: ("num", v))
        trees = [("and", ("rn_eq", "u2i"), ("cmp", "==", col("category"), num(3))),
                 ("or", ("cmp", ">", ("score",), num(0.5)), ("not", ("in", col("brand"), [1, 2]))), ("rn_in", ["u2i", "hot"])]
        source = np.array([names.index(x["retrieve_id"]) if x["retrieve_id"] in ("u2i", "hot") else 0xFF for x in items], np.uint8)
        score = np.array([x["score"] for x in items])
        mask = ref.masks(trees, n, c, inside, score, source, ["u2i", "hot"])
        keep = ref.cut_positions([(FIX, 10), (ACC, 20), (ACC, 40)], np.arange(n, dtype=np.uint64), score, None, mask)
        assert got == [ids[p] for p in keep] and 10 < len(keep) <= 50
        assert json.loads(H.ph_engine_filter(h, b"classes", b"[]", b"{}"))["items"] == []
        assert H.ph_engine_filter(h, b"no_such_column", json.dumps(items).encode(), b"{}") is None
        assert b"DiversityAdjustCountFilter" in H.ph_last_error() and b'"colour" is not a feature column' in H.ph_last_error()
    finally:
        H.ph_engine_destroy(h)
