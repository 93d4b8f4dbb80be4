"""The feature store's gathers (csrc/features.hip) and the FM item records (csrc/rank_mlp.hip fills them, rank_entry.hip
holds their entry points) at their edges, bit for bit against
tests/features_ref.py (its own known answers: tests/test_features_ref_cpu.py).  The rules under test are stated in
include/pairec_gpu.h — pg_features_set_column: THE STORED DEFAULT; pg_features_gather_f32_dev: DIRECT CONVERSION;
pg_rank_fm2t_rows_dev: THE CLAMP ON ITEM IDS; pg_fm2t_item_rows_update: the range check — and in DESIGN.md §5.8.

Shapes: a store of 97 rows (no multiple of anything), requests that touch rows 0, 96 (the last), 97, 98 and 0xFFFFFFFF (outside:
the column default) with repeats, and element counts on both sides of a 256-thread block.  Every column has a default of its own,
-(1000 f + 1), so that a mixed-up column shows."""
import ctypes as C

import numpy as np
import pytest

import features_ref as fr
import pairec_amd as pa
from oracle import oracle as o
from pairec_amd._lib import PgError, check

pytestmark = pytest.mark.gpu

INVALID = -1                                          # PG_ERR_INVALID
N = 97
EDGE_ROWS = [0, 96, 97, 98, 0xFFFFFFFF, 5, 5, 96, 0, 0xFFFFFFFF, 42, 97]
I32_MIN, I32_MAX, I64_MIN, I64_MAX = -2**31, 2**31 - 1, -2**63, 2**63 - 1
TIE = 2**60 + 2**36                                   # halfway between two fp32 neighbours (test_features_ref_cpu.py)


def request_rows(n, seed):
    """n rows: the edges first, then rows of the store at random (repeats included)"""
    rng = np.random.default_rng(seed)
    return np.concatenate([EDGE_ROWS, rng.integers(0, N, max(n, len(EDGE_ROWS)))]).astype(np.uint32)[:n]


def make_store(ctx, cols):
    fs = pa.Features(ctx, N)
    for name, (dtype, values, default) in cols.items():
        fs.set_column(name, dtype, values, default=default)
    return fs


def b32(x):
    return int(np.float32(x).view(np.uint32))


def same_f32(got, want):
    """bit for bit; NaN compared with isnan (its payload is not pinned)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(fr.bits32(got)[~nan], fr.bits32(want)[~nan])


# ---- integer gather: the kernel-argument form (<= 16 columns) and the staged form -----------------------------------------------------
def int_columns():
    """33 integer columns, I32 and I64 alternating, the edge values in the first rows of each"""
    rng = np.random.default_rng(97)
    cols = {}
    for f in range(33):
        if f % 2 == 0:
            v = rng.integers(-1000, 1000, N).astype(np.int32)
            v[:4] = [0, -1, I32_MIN, I32_MAX]
            cols["c%d" % f] = (fr.I32, np.roll(v, f), -(1000 * f + 1))
        else:
            v = rng.integers(-2**40, 2**40, N).astype(np.int64)
            v[:8] = [0, -1, I32_MIN, I32_MAX, 2**31, -2**31 - 1, I64_MIN, I64_MAX]
            cols["c%d" % f] = (fr.I64, np.roll(v, f), -(1000 * f + 1))
    cols["fl"] = (fr.F32, rng.random(N).astype(np.float32), -0.5)
    return cols


@pytest.fixture(scope="module")
def int_store(ctx):
    cols = int_columns()
    fs = make_store(ctx, cols)
    yield fs, cols
    fs.destroy()


@pytest.mark.parametrize("n_cols", [1, 3, 16, 17, 33])
def test_integer_gather_both_kernels(ctx, int_store, n_cols):
    """features_gather_i32_args_kernel up to 16 columns, stage_descs + features_gather_i32_kernel beyond (17, 33).  Row counts put
    n x n_cols on both sides of the 256-thread block: exactly 1, 255, 256, 257 where n_cols divides them, otherwise the nearest
    counts around 256 — there the block's edge falls inside an output row, at an element count that is no multiple of n_cols."""
    fs, cols = int_store
    names = ["c%d" % f for f in range(n_cols)]
    counts = sorted({1, 255 // n_cols, -(-256 // n_cols), -(-257 // n_cols), 256 // n_cols + 1, len(EDGE_ROWS) + 9} - {0})
    if n_cols == 1:
        assert {1, 255, 256, 257} <= set(counts)
    for n in counts:
        rows = request_rows(n, n * 131 + n_cols)
        got = fs.gather_i32(names, rows)
        assert np.array_equal(got, fr.gather_i32_ref(cols, rows, names)), (n_cols, n)
    rows = request_rows(40, 5)
    got = fs.gather_i32(names, rows)
    assert np.array_equal(got[rows >= N], np.broadcast_to([-(1000 * f + 1) for f in range(n_cols)], (int((rows >= N).sum()), n_cols)))
    if n_cols > 1:                                    # saturation happened: both ends of int64 are in column 1
        all_rows = np.arange(N, dtype=np.uint32)
        c1 = fs.gather_i32(names, all_rows)[:, 1]
        assert c1.min() == I32_MIN and c1.max() == I32_MAX and np.array_equal(c1, np.clip(cols["c1"][1], I32_MIN, I32_MAX))


def test_integer_gather_column_order_and_the_two_kernels_agree(ctx, int_store):
    fs, cols = int_store
    rows = request_rows(31, 3)
    n17 = ["c%d" % f for f in range(17)]
    g17 = fs.gather_i32(n17, rows)
    g16 = fs.gather_i32(n17[:16], rows)
    assert np.array_equal(g17[:, :16], g16)                                            # staged kernel == argument kernel
    for names in (["c3", "c3"], ["c2", "c5", "c2", "c5", "c2"], n17[::-1], n17[:16][::-1], ["c1"] * 17,
                  ["c%d" % f for f in range(32, -1, -1)]):
        got = fs.gather_i32(names, rows)
        assert np.array_equal(got, fr.gather_i32_ref(cols, rows, names)), names
    assert np.array_equal(fs.gather_i32(n17[::-1], rows), g17[:, ::-1])


def test_integer_gather_refusals_and_empty_request(ctx, int_store):
    fs, cols = int_store
    rows = request_rows(20, 1)
    n17 = ["c%d" % f for f in range(17)]
    count = int(ctx.L.pg_features_num_columns(fs.h))
    assert count == 34
    for names in (n17[:8] + ["fl"] + n17[9:], ["fl"], n17[:16] + ["fl"]):              # a float column among 17 names (and among 1)
        with pytest.raises(PgError, match=r'column "fl" is not an integer column') as ei:
            fs.gather_i32(names, rows)
        assert ei.value.code == INVALID
    for bad in (-1, count):
        for names in ([bad], n17[:5] + [bad], n17[:16] + [bad], [bad] + n17[:16]):
            with pytest.raises(PgError, match=r"column index %d out of range \(34 columns\)" % bad) as ei:
                fs.gather_i32(names, rows)
            assert ei.value.code == INVALID
    # n == 0: PG_OK, the output untouched (both forms)
    sentinel = np.full(64, 0x5A5A5A5A, np.int32)
    d_out, d_rows = ctx.to_device(sentinel), ctx.to_device(rows)
    for k in (3, 17):
        idx = np.arange(k, dtype=np.int32)
        assert ctx.L.pg_features_gather_i32_dev(ctx.h, fs.h, idx.ctypes.data_as(C.c_void_p), k, d_rows, 0, d_out) == 0
        assert ctx.L.pg_features_gather_f32_dev(ctx.h, fs.h, idx.ctypes.data_as(C.c_void_p), k, None, None, d_rows, 0, d_out) == 0
    back = np.zeros_like(sentinel)
    ctx.d2h(back, d_out)
    assert np.array_equal(back, sentinel)
    ctx.free(d_out)
    ctx.free(d_rows)
    # the store still serves
    assert np.array_equal(fs.gather_i32(n17, rows), fr.gather_i32_ref(cols, rows, n17))


# ---- float gather: one rounding into fp32, one fused multiply-add --------------------------------------------------------------------
def float_columns():
    """17 columns cycling I32, I64, F32, F64, the directed values of test_features_ref_cpu.py in the first rows of each"""
    rng = np.random.default_rng(1797)
    fused = 1 + 2.0**-12
    directed = {
        fr.I32: [I32_MAX, I32_MIN, 16777217, -16777217, 16777219, 0, -1],
        fr.I64: [TIE + 1, TIE - 1, -(TIE + 1), -(TIE - 1), TIE, -TIE, TIE + 2**37 - 1, 2**53 + 1, -(2**53 + 1), I64_MAX, I64_MIN, 0, -1],
        fr.F32: [fused, np.nan, np.inf, -np.inf, -0.0, 1e-40, -1e-40, 3.4028235e38, 1.17549435e-38, 0.1],
        fr.F64: [fused, 1e39, -1e39, 1e-40, -1e-40, np.nan, np.inf, -np.inf, -0.0, 0.1, 1e-50, 3.4028235677973366e38,
                 1 + 2.0**-24, 1 + 2.0**-24 + 2.0**-50, 7.006492321624085e-46],
    }
    cols = {}
    for f in range(17):
        dtype = (fr.I32, fr.I64, fr.F32, fr.F64)[f % 4]
        if dtype in (fr.I32, fr.I64):
            v = rng.integers(-2**30, 2**30, N).astype(fr.NP[dtype])
        else:
            v = (rng.standard_normal(N) * 10.0 ** rng.integers(-6, 6, N)).astype(fr.NP[dtype])
        with np.errstate(over="ignore"):
            v[:len(directed[dtype])] = np.array(directed[dtype], dtype=fr.NP[dtype])
        cols["v%d" % f] = (dtype, np.roll(v, 3 * f), -(1000 * f + 1) - (0.3 if dtype in (fr.F32, fr.F64) else 0.0))
    return cols


@pytest.fixture(scope="module")
def float_store(ctx):
    cols = float_columns()
    fs = make_store(ctx, cols)
    yield fs, cols
    fs.destroy()


def normalizers(n_cols):
    """(scale, bias) per mode: none, scale only, bias only, both — the last one the pair that an unfused multiply-then-add gets
    wrong for the value 1 + 2^-12 (2^-24 fused, 0 unfused) and that cancels heavily on everything near 1"""
    cyc = lambda vals: np.array([vals[f % len(vals)] for f in range(n_cols)], np.float32)
    return {"none": (None, None),
            "scale": (cyc([0.01, 2.0, 2.0**-100, 3e38, -1.5]), None),                 # results: subnormal, overflow, negated
            "bias": (None, cyc([0.25, -1.0, 1e-40, 1e30, -0.0])),
            "both": (cyc([1 + 2.0**-12]), cyc([-(1 + 2.0**-11)]))}


@pytest.mark.parametrize("names", [["v0"], ["v1"], ["v2"], ["v3"], ["v%d" % f for f in range(5)], ["v%d" % f for f in range(17)]],
                         ids=["i32", "i64", "f32", "f64", "5cols", "17cols"])
def test_float_gather_is_one_conversion_and_one_fmaf(ctx, float_store, names):
    """pg_features_gather_f32_dev = fmaf((float)value, scale, bias), IEEE: an int64 beyond 2^53 rounds once, the multiply-add is
    fused, fp32 subnormals are kept, fp64 beyond the range is ±inf, NaN stays NaN, -0.0 through (1, +0) is +0.0."""
    fs, cols = float_store
    rows = np.concatenate([EDGE_ROWS, np.arange(N)]).astype(np.uint32)
    for mode, (scale, bias) in normalizers(len(names)).items():
        got = fs.gather_f32(names, rows, scale, bias)
        want = fr.gather_f32_ref(cols, rows, names, scale, bias)
        bad = [(int(rows[i]), names[f], hex(int(fr.bits32(got)[i, f])), hex(int(fr.bits32(want)[i, f])))
               for i, f in zip(*np.nonzero(~((fr.bits32(got) == fr.bits32(want)) | (np.isnan(got) & np.isnan(want)))))]
        print("gather_f32 %s mode %s: %d of %d differ (row, column, got, want): %s" % (names[-1], mode, len(bad), got.size, bad[:8]))
        assert same_f32(got, want), (mode, bad[:8])


def test_float_gather_directed_values_on_the_device(ctx, float_store):
    """The known answers themselves, read off the device (no reference in between)."""
    fs, cols = float_store
    r = lambda f, j: np.array([(j + 3 * f) % N], np.uint32)                            # float_columns rolls column f by 3 f
    g = lambda name, f, j, **kw: fs.gather_f32([name], r(f, j), **kw)[0, 0]
    observed = [hex(b32(g("v1", 1, j))) for j in range(4)]
    print("int64 → fp32 of ±(2^60 + 2^36 ± 1), observed bits: %s (single rounding: 0x5d800001 0x5d800000 0xdd800001 0xdd800000)" % observed)
    assert observed == ["0x5d800001", "0x5d800000", "0xdd800001", "0xdd800000"]
    assert b32(g("v1", 1, 6)) == 0x5D800001                                      # 2^60 + 3·2^36 − 1: a double makes it a tie
    assert b32(g("v0", 0, 2)) == 0x4B800000 and b32(g("v0", 0, 4)) == 0x4B800002   # 2^24 + 1, 2^24 + 3: ties to even
    one = np.array([1 + 2.0**-12], np.float32)
    for name, f in (("v2", 2), ("v3", 3)):                                             # fused: 2^-24, not 0
        assert float(g(name, f, 0, scale=one, bias=np.array([-(1 + 2.0**-11)], np.float32))) == 2.0**-24
    assert g("v3", 3, 1) == np.inf and g("v3", 3, 2) == -np.inf                        # fp64 1e39
    assert b32(g("v3", 3, 3)) == 0x000116C2 and b32(g("v3", 3, 4)) == 0x800116C2   # fp64 1e-40: the subnormal, kept
    assert b32(g("v2", 2, 5)) == 0x000116C2                                      # an fp32 subnormal passes through fmaf(x, 1, 0)
    assert np.isnan(g("v3", 3, 5)) and np.isnan(g("v2", 2, 1))
    assert g("v3", 3, 6) == np.inf and g("v3", 3, 7) == -np.inf and g("v2", 2, 2) == np.inf and g("v2", 2, 3) == -np.inf
    assert b32(g("v3", 3, 8)) == 0 and b32(g("v2", 2, 4)) == 0             # -0.0 → fmaf(-0, 1, +0) = +0.0
    assert b32(g("v3", 3, 8, bias=np.array([-0.0], np.float32))) == 0x80000000
    assert g("v3", 3, 11) == np.inf                                                    # FLT_MAX + half an ulp: ties to even = inf
    assert b32(g("v3", 3, 12)) == 0x3F800000 and b32(g("v3", 3, 13)) == 0x3F800001   # 1 + 2^-24 (tie), just above


# ---- column lifecycle ----------------------------------------------------------------------------------------------------------------
def num_columns(fs):
    return int(fs.ctx.L.pg_features_num_columns(fs.h))


def eval_column(fs, name, rows):
    e = pa.Expr("${%s}" % name)
    try:
        return fs.eval_expr(e, rows)
    finally:
        e.free()


def test_null_filled_column_reads_one_default_inside_and_outside(ctx):
    """THE STORED DEFAULT: set_column(values=NULL) — a row inside and a row outside read the same bits through gather_i32,
    gather_f32 and eval_expr, and they are the default rounded to the dtype (0.1 on F32 is 0.100000001490116…, -7.9 on I32 is -7)."""
    specs = {"a": (fr.I32, -7.9), "b": (fr.I64, 2.0**40 + 0.5), "c": (fr.F32, 0.1), "d": (fr.F64, 0.1), "e": (fr.I64, -0.5),
             "f": (fr.I32, 2.0**31 - 0.5), "g": (fr.I64, -2.0**63), "h": (fr.F32, 1e39), "i": (fr.I64, 2.0**62 + 2.0**30)}
    fs = pa.Features(ctx, N)
    cols = {}
    for name, (dtype, d) in specs.items():
        fs.set_column(name, dtype, None, default=d)
        cols[name] = (dtype, fr.null_column(dtype, N, d), d)
    rows = np.array(EDGE_ROWS, np.uint32)
    inside, outside = np.flatnonzero(rows < N), np.flatnonzero(rows >= N)
    ints = [n for n in specs if specs[n][0] in (fr.I32, fr.I64)]
    names = list(specs)
    for name, (dtype, d) in specs.items():                                             # every figure first, then the assertions
        ev, gf = fr.bits64(eval_column(fs, name, rows)), fr.bits32(fs.gather_f32([name], rows))[:, 0]
        print("default %r on dtype %d: eval_expr inside %s outside %s; gather_f32 inside %s outside %s" % (
            d, dtype, hex(int(ev[inside[0]])), hex(int(ev[outside[0]])), hex(int(gf[inside[0]])), hex(int(gf[outside[0]]))))
    gi = fs.gather_i32(ints, rows)
    print("gather_i32 of %s: inside %s outside %s" % (ints, gi[inside[0]].tolist(), gi[outside[0]].tolist()))
    assert np.array_equal(gi, fr.gather_i32_ref(cols, rows, ints))
    assert gi[0].tolist() == [-7, I32_MAX, 0, I32_MAX, I32_MIN, I32_MAX] and (gi == gi[0]).all()
    for scale, bias in ((None, None), (np.full(len(names), 3.0, np.float32), np.full(len(names), -0.3, np.float32))):
        gf = fs.gather_f32(names, rows, scale, bias)
        assert same_f32(gf, fr.gather_f32_ref(cols, rows, names, scale, bias))
        assert (fr.bits32(gf) == fr.bits32(gf)[0]).all()
    for name, (dtype, d) in specs.items():
        ev = fr.bits64(eval_column(fs, name, rows))
        assert len(set(ev.tolist())) == 1, (name, [hex(int(x)) for x in ev])
        assert ev[0] == fr.bits64(np.array([float(fr.stored_default(dtype, d))]))[0], name
    assert eval_column(fs, "c", rows)[0] == float(np.float32(0.1)) != 0.1
    assert eval_column(fs, "a", rows)[3] == -7.0 and fr.bits64(eval_column(fs, "e", rows))[3] == 0     # (-0.5 → 0 → +0.0)
    fs.destroy()


def test_column_replacement_keeps_its_index_through_every_dtype(ctx):
    rng = np.random.default_rng(4)
    cols = {"keep": (fr.I64, rng.integers(-2**50, 2**50, N).astype(np.int64), -1),
            "x": (fr.I32, rng.integers(-99, 99, N).astype(np.int32), -1001),
            "tail": (fr.F64, rng.standard_normal(N), -2001.5)}
    fs = make_store(ctx, cols)
    rows = request_rows(40, 8)
    names = ["keep", "x", "tail"]

    def check_all():
        assert [fs.index(n) for n in names] == [0, 1, 2] and num_columns(fs) == 3
        assert same_f32(fs.gather_f32(names, rows), fr.gather_f32_ref(cols, rows, names))
        ints = [n for n in names if cols[n][0] in (fr.I32, fr.I64)]
        assert np.array_equal(fs.gather_i32(ints, rows), fr.gather_i32_ref(cols, rows, ints))
        assert np.array_equal(fr.bits64(eval_column(fs, "x", rows)), fr.bits64(fr.bind_f64_ref(cols, rows, "x")))

    check_all()
    # the element size changes with every step: 4, 8, 4, 8, 4
    for step, dtype in enumerate((fr.I64, fr.F32, fr.F64, fr.I32)):
        if dtype in (fr.I32, fr.I64):
            v = rng.integers(-2**30, 2**30, N).astype(fr.NP[dtype])
        else:
            v = (rng.standard_normal(N) * 1e3).astype(fr.NP[dtype])
        cols["x"] = (dtype, v, -(1000 * (step + 2) + 1))
        fs.set_column("x", dtype, v, default=cols["x"][2])
        check_all()
    # the same dtype again: new values, a new default
    cols["x"] = (fr.I32, rng.integers(-7, 7, N).astype(np.int32), 123456)
    fs.set_column("x", fr.I32, cols["x"][1], default=123456)
    check_all()
    assert fs.gather_i32(["x"], np.array([N], np.uint32))[0, 0] == 123456
    # values → NULL fill of the same dtype
    cols["x"] = (fr.I32, fr.null_column(fr.I32, N, 77.7), 77.7)
    fs.set_column("x", fr.I32, None, default=77.7)
    check_all()
    fs.destroy()


def test_forty_more_columns_leave_the_first_readable(ctx):
    rng = np.random.default_rng(40)
    cols = {"first": (fr.I64, rng.integers(-2**62, 2**62, N).astype(np.int64), -1)}
    fs = make_store(ctx, cols)
    rows = request_rows(30, 2)
    before = fs.gather_i32(["first"], rows)
    for f in range(40):
        dtype = (fr.I32, fr.I64, fr.F32, fr.F64)[f % 4]
        cols["m%d" % f] = (dtype, (rng.random(N) * 100).astype(fr.NP[dtype]), -(1000 * (f + 1) + 1))
        fs.set_column("m%d" % f, dtype, cols["m%d" % f][1], default=cols["m%d" % f][2])
    assert num_columns(fs) == 41 and fs.index("first") == 0 and fs.index("m39") == 40
    assert np.array_equal(fs.gather_i32(["first"], rows), before) and np.array_equal(before, fr.gather_i32_ref(cols, rows, ["first"]))
    names = list(cols)
    assert same_f32(fs.gather_f32(names, rows), fr.gather_f32_ref(cols, rows, names))  # 41 columns through one call
    fs.destroy()


def test_refused_integer_defaults_leave_the_store_as_it_was(ctx):
    """An I32 / I64 default that is NaN, infinite or outside the dtype's range: PG_ERR_INVALID naming the column, before anything
    is allocated or modified — a refused new column does not exist, a refused replacement keeps values, dtype and default."""
    rng = np.random.default_rng(9)
    cols = {"p": (fr.I32, rng.integers(-50, 50, N).astype(np.int32), -1), "q": (fr.I64, rng.integers(-2**40, 2**40, N).astype(np.int64), -1001),
            "r": (fr.F32, rng.random(N).astype(np.float32), -2001.0)}
    fs = make_store(ctx, cols)
    rows = request_rows(30, 6)
    bad = [(fr.I32, np.nan), (fr.I32, np.inf), (fr.I32, -np.inf), (fr.I32, 2.0**31), (fr.I32, 3e9), (fr.I32, -2.0**31 - 1),
           (fr.I64, np.nan), (fr.I64, np.inf), (fr.I64, -np.inf), (fr.I64, 2.0**63), (fr.I64, -2.0**64)]
    ones32, ones64 = np.ones(N, np.int32), np.ones(N, np.int64)

    def unchanged():
        assert num_columns(fs) == 3 and [fs.index(n) for n in ("p", "q", "r", "new")] == [0, 1, 2, -1]
        assert np.array_equal(fs.gather_i32(["p", "q"], rows), fr.gather_i32_ref(cols, rows, ["p", "q"]))
        assert same_f32(fs.gather_f32(["p", "q", "r"], rows), fr.gather_f32_ref(cols, rows, ["p", "q", "r"]))

    for dtype, d in bad:
        values = ones32 if dtype == fr.I32 else ones64
        for name in ("new", "p", "q", "r"):                                            # a new column; same-dtype and other-dtype replacements
            for v in (values, None):
                with pytest.raises(PgError, match='column "%s"' % name) as ei:
                    fs.set_column(name, dtype, v, default=d)
                assert ei.value.code == INVALID, (dtype, d, name)
        unchanged()
    # the ends of the ranges are accepted
    fs.set_column("new", fr.I32, None, default=2.0**31 - 1)
    fs.set_column("new", fr.I32, None, default=-2.0**31)
    fs.set_column("new", fr.I64, None, default=2.0**63 - 1024)
    fs.set_column("new", fr.I64, None, default=-2.0**63)
    assert fs.gather_i32(["new"], np.array([0, N], np.uint32))[:, 0].tolist() == [I32_MIN, I32_MIN]
    assert eval_column(fs, "new", np.array([0, N], np.uint32)).tolist() == [-2.0**63, -2.0**63]
    # floats take any default (rounded to the dtype)
    fs.set_column("r", fr.F32, None, default=np.nan)
    assert np.isnan(fs.gather_f32(["r"], np.array([0, N], np.uint32))).all()
    fs.destroy()


# ---- expressions over columns --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257])
def test_expression_sums_sixteen_columns_of_every_dtype(ctx, n):
    """pg_features_eval_dev binds (double)value: one expression over 16 variables, four of each dtype, int64 values beyond 2^53
    (nearest-even into the double), rows outside the store reading the stored defaults — against the oracle's evaluator."""
    rng = np.random.default_rng(16)
    cols = {}
    for f in range(16):
        dtype = (fr.I32, fr.I64, fr.F32, fr.F64)[f % 4]
        if dtype == fr.I64:
            v = rng.integers(-2**62, 2**62, N).astype(np.int64)
            v[:6] = [2**53 + 1, -(2**53 + 1), 2**53 + 3, TIE + 1, I64_MAX, I64_MIN]
            v = np.roll(v, f)
        elif dtype == fr.I32:
            v = rng.integers(I32_MIN, I32_MAX, N).astype(np.int32)
        else:
            v = (rng.standard_normal(N) * 10.0 ** rng.integers(-3, 18, N)).astype(fr.NP[dtype])
        cols["x%d" % f] = (dtype, v, -(1000 * f + 1) - (0.1 if dtype == fr.F32 else 0.0))
    fs = make_store(ctx, cols)
    rows = np.concatenate([np.arange(N), EDGE_ROWS, np.random.default_rng(n).integers(0, N, 300)]).astype(np.uint32)[:n] if n > 1 \
        else np.array([1], np.uint32)
    bound = {name: fr.bind_f64_ref(cols, rows, name) for name in cols}
    assert n == 1 or (2.0**53 + 4 in bound["x1"] and -2.0**53 in bound["x1"] and 2.0**63 in bound["x1"])     # nearest even
    src = "+".join("${x%d}" % f for f in range(16))
    e = pa.Expr(src)
    got = fs.eval_expr(e, rows)
    e.free()
    ast = o.expr_parse(src)
    want = np.array([o.expr_eval(ast, lambda nm, i=i: float(bound[nm][i])) for i in range(n)])
    assert np.array_equal(fr.bits64(got), fr.bits64(want))
    e = pa.Expr(src + "+${x0}*${nope}")                                                # 17 variables
    with pytest.raises(PgError, match=r"17 variables \(at most 16") as ei:
        fs.eval_expr(e, rows)
    assert ei.value.code == INVALID
    e.free()
    fs.destroy()


# ---- FM item field ids outside the vocabulary ----------------------------------------------------------------------------------------
VOCAB, ITEMS = 50, 300
SIZES = [0, 1, 33, 64, 130]


def fm_model_weights(nuf, nif, k, th, to):
    return o.Fm2tWeights(n_user_fields=nuf, n_item_fields=nif, k=k, d_user=96, t_h1=th, t_out=to, vocab=VOCAB)


def fm_id_columns(nif, seed):
    """nif integer columns over ITEMS rows, I32 / I64 alternating, ids inside the vocabulary at random and, in every column, the ids
    that are not: -1, INT32_MIN, 50, 55 (and the last id 49); 2^40 and -2^40 in the int64 columns.  Defaults: vocab + 100 and -3."""
    rng = np.random.default_rng(seed)
    cols = {}
    for f in range(nif):
        dtype = fr.I64 if f % 2 else fr.I32
        v = rng.integers(0, VOCAB, ITEMS).astype(np.int64)
        special = [-1, I32_MIN, 49, 50, 55] + ([2**40, -2**40] if dtype == fr.I64 else [])
        where = rng.choice(ITEMS, 6 * len(special), replace=False)
        v[where] = np.tile(special, 6)
        cols["id%d" % f] = (dtype, v.astype(fr.NP[dtype]), VOCAB + 100 if f % 2 == 0 else -3)
    return cols


def raw_ids(cols, names, cand):
    """the columns' own values at the candidates (int64, nothing saturated or clamped; the stored default outside the store)"""
    return np.stack([fr.at_rows(cols[n], cand).astype(np.int64) for n in names], axis=1)


def rank_fm2t_dev(ctx, m, users, ufids, ids, off):
    """pg_rank_fm2t_dev on device arrays: the ids go to the kernel as they are"""
    users, ufids = np.ascontiguousarray(users, np.float32), np.ascontiguousarray(ufids, np.int32)
    ids, off = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(off, np.uint32)
    n = int(off[-1])
    bufs = [ctx.to_device(a) for a in (users, ufids, ids, off)] + [ctx.malloc(max(4 * n, 16))]
    try:
        check(ctx.L.pg_rank_fm2t_dev(ctx.h, m.h, *bufs[:4], off.shape[0] - 1, n, bufs[4]))
        out = np.zeros(n, np.float32)
        ctx.d2h(out, bufs[4])
    finally:
        for p in bufs:
            ctx.free(p)
    return out


@pytest.mark.parametrize("nuf,nif,k,th,to", [(8, 8, 16, 256, 64), (16, 16, 8, 128, 64), (3, 4, 32, 256, 64)])
def test_fm_ids_outside_the_vocabulary_clamp_alike_on_every_path(ctx, nuf, nif, k, th, to):
    """THE CLAMP ON ITEM IDS: pg_rank_fm2t_rows_dev, the item records and pg_rank_fm2t_dev on the raw ids are bit-identical to each
    other and to pg_rank_fm2t on clamp_ids(...), and within the project's tolerances of the oracle on the clamped ids; the host entry
    refuses the raw ids and names the first."""
    fw = fm_model_weights(nuf, nif, k, th, to)
    cols = fm_id_columns(nif, k)
    names = list(cols)
    feats = pa.Features(ctx, ITEMS)
    for name, (dtype, v, d) in cols.items():
        feats.set_column(name, dtype, v, default=d)
    rng = np.random.default_rng(k + 1)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint32)
    R, n = len(SIZES), int(off[-1])
    cand = rng.integers(0, ITEMS, n).astype(np.uint32)
    cand[[0, 1, 40, 99, n - 1]] = [ITEMS, 0xFFFFFFFF, ITEMS - 1, ITEMS + 7, 0xFFFFFFFF]     # outside the store: the defaults
    users = o.synth_rows(o.SEED_QUERY, 1, R, 128)[:, :96].copy()
    ufids = rng.integers(0, VOCAB, (R, nuf)).astype(np.int32)
    raw = raw_ids(cols, names, cand)
    raw32 = fr.gather_i32_ref(cols, cand, names)                                       # the same raw values as int32 (2^40 saturates)
    assert np.array_equal(feats.gather_i32(names, cand), raw32)
    clamped = fr.clamp_ids(raw, VOCAB)
    assert np.array_equal(clamped, fr.clamp_ids(raw32, VOCAB))
    out_of_vocab = (raw32 < 0) | (raw32 >= VOCAB)
    assert out_of_vocab.any(axis=1).sum() > n // 8 and {-1, I32_MIN, 50, 55, I32_MAX, VOCAB + 100, -3} <= set(raw32[out_of_vocab].tolist())
    first_bad = int(raw32.reshape(-1)[np.flatnonzero(out_of_vocab.reshape(-1))[0]])
    for prec, tol in ((pa.PREC_F32, 2e-7), (pa.PREC_BF16, 1e-5)):
        m = pa.RankModel(ctx, pa.MODEL_FM_TWOTOWER, prec, pa.pack_fm2t(fw))
        ir = pa.ItemRows(m, feats, names)
        ref = m.rank_fm2t(users, ufids, clamped, off)
        paths = {"rank_fm2t_rows": m.rank_fm2t_rows(feats, names, users, ufids, cand, off),
                 "ItemRows.rank": ir.rank(users, ufids, cand, off),
                 "pg_rank_fm2t_dev": rank_fm2t_dev(ctx, m, users, ufids, raw32, off)}
        for name, got in paths.items():
            assert np.array_equal(fr.bits32(got), fr.bits32(ref)), "precision mode %d: %s differs from rank_fm2t on the clamped ids" % (prec, name)
        for r in range(R):
            if off[r + 1] > off[r]:
                want = o.fm2t_forward(fw, prec, users[r], ufids[r], clamped[off[r]:off[r + 1]])
                assert np.max(np.abs(ref[off[r]:off[r + 1]].astype(np.float64) - want)) <= tol, (prec, r)
        with pytest.raises(PgError, match=r"item field id %d outside vocab %d" % (first_bad, VOCAB)) as ei:
            m.rank_fm2t(users, ufids, raw32, off)
        assert ei.value.code == INVALID
        ir.destroy()
        m.destroy()
    feats.destroy()


# ---- item records: partial updates ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [pa.PREC_F32, pa.PREC_BF16], ids=["f32", "bf16"])
def test_item_records_partial_updates(ctx, prec):
    """pg_fm2t_item_rows_update rewrites rows [row0, row0 + nrows) and the defaults' record, nothing else; a range outside the
    store is refused on the host (a wrapping row0 + nrows included) with the records as they were."""
    nuf, nif = 8, 8
    fw = fm_model_weights(nuf, nif, 16, 256, 64)
    m = pa.RankModel(ctx, pa.MODEL_FM_TWOTOWER, prec, pa.pack_fm2t(fw))
    rng = np.random.default_rng(77)
    names = ["id%d" % f for f in range(nif)]
    dtypes = [fr.I64 if f % 2 else fr.I32 for f in range(nif)]
    defaults = [3 + f for f in range(nif)]
    old = rng.integers(0, VOCAB, (ITEMS, nif))
    new = (old + rng.integers(1, VOCAB, (ITEMS, nif))) % VOCAB                          # every id changes
    assert (old != new).all()
    feats = pa.Features(ctx, ITEMS)

    def set_cols(ids, which=range(nif)):
        for f in which:
            feats.set_column(names[f], dtypes[f], ids[:, f].astype(fr.NP[dtypes[f]]), default=defaults[f])

    set_cols(old)
    ir = pa.ItemRows(m, feats, names)
    cand = np.concatenate([np.arange(ITEMS), [ITEMS, 0xFFFFFFFF, ITEMS + 1]]).astype(np.uint32)
    off = np.array([0, 130, 131, 131, len(cand)], np.uint32)
    R = len(off) - 1
    users = o.synth_rows(o.SEED_QUERY, 2, R, 128)[:, :96].copy()
    ufids = rng.integers(0, VOCAB, (R, nuf)).astype(np.int32)
    inside = cand < ITEMS
    safe = np.minimum(cand, ITEMS - 1).astype(np.int64)

    def expect(ids_of_row):
        ids = np.where(inside[:, None], ids_of_row[safe], np.array(defaults)[None, :]).astype(np.int32)
        return fr.bits32(m.rank_fm2t(users, ufids, ids, off))

    def records():
        return fr.bits32(ir.rank(users, ufids, cand, off))

    assert np.array_equal(records(), expect(old))
    # the columns change everywhere; only [a, b) is re-materialised
    a, b = 37, 141
    set_cols(new)
    ir.update(a, b - a)
    mixed = old.copy()
    mixed[a:b] = new[a:b]
    assert np.array_equal(records(), expect(mixed)), "rows outside [a, b) were rewritten, or rows inside were not"
    assert not np.array_equal(expect(mixed), expect(new)) and not np.array_equal(expect(mixed), expect(old))
    ir.update(0, 1)                                                                     # the first row alone
    mixed[0] = new[0]
    assert np.array_equal(records(), expect(mixed))
    ir.update(ITEMS - 1, 1)                                                             # the last row alone
    mixed[ITEMS - 1] = new[ITEMS - 1]
    assert np.array_equal(records(), expect(mixed))
    # only a default changes: update(0, 0) refreshes the defaults' record and nothing else
    before = records()
    defaults[2] = 41
    set_cols(new, [2])
    assert np.array_equal(records(), before)                                            # (nothing follows before the update)
    ir.update(0, 0)
    after = records()
    assert np.array_equal(after, expect(mixed)) and np.array_equal(after[inside], before[inside]) and (after[~inside] != before[~inside]).all()
    # refusals: host-side, nothing launched, the records as they were
    for row0, nrows in ((ITEMS, 1), (1, ITEMS), (2**64 - 1, 2), (2**64 - 1, 1), (ITEMS + 1, 0), (0, 2**64 - 1), (2**63, 2**63)):
        with pytest.raises(PgError, match="outside the store") as ei:
            ir.update(row0, nrows)
        assert ei.value.code == INVALID, (row0, nrows)
    assert np.array_equal(records(), after)
    ir.update(ITEMS, 0)                                                                 # the empty range at the end is a range of the store
    assert np.array_equal(records(), after)
    # a column changes dtype (its buffer is reallocated with another element size): update(0, rows) equals a fresh build
    dtypes[0] = fr.I64
    set_cols(new, [0])
    ir.update(0, ITEMS)
    fresh = pa.ItemRows(m, feats, names)
    got = records()
    assert np.array_equal(got, fr.bits32(fresh.rank(users, ufids, cand, off))) and np.array_equal(got, expect(new))
    assert np.array_equal(got, fr.bits32(m.rank_fm2t_rows(feats, names, users, ufids, cand, off)))
    fresh.destroy()
    ir.destroy()
    m.destroy()
    feats.destroy()
