"""GPU tests of what the table pass derives from a table's rows and the screens then trust (recall_table.hip, recall_i4.hip,
recall_r2.hip), read back through pg_table_derived_info / pg_table_derived_read and held to tests/table_derived_ref.py: the
scales and every shadow bit for bit, every bound >= its fp64 value with no slack and <= its documented cap, the routing
statistics within 1e-3.  Tables are small; the sizes are those where the build kernels' shared loop shape (DIM / 8 lanes per row,
a butterfly within the row, a wave reduction, one atomic per workgroup, a grid-stride loop over ((n8 + 63) & ~63) groups) can go
wrong: fewer rows than a wave, ragged waves and workgroups, and G + 37 rows, the first size with a second, ragged trip.
Witness tables put the one row that decides a maximum where a reduction would lose it."""
import ctypes as C
import functools
import subprocess
import sys

import numpy as np
import pytest

import pairec_amd as pa
from pairec_amd import _lib
from oracle import oracle as o
import table_derived_ref as ref
from table_derived_ref import F

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1000)
SMALL = 1003
RATIOS = {}                      # the largest value / cap seen per tightness cap (printed by the last test)


@functools.lru_cache(maxsize=None)
def device_cus():
    """the device's CU count, asked of a short-lived child (as test_gpu_rank_persistent.py does: torch's HIP runtime finds no
    device in a process where the library's has already opened it)"""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout.split()[-1])


def trip_rows(dim):
    """G: the rows one trip of the build kernels' grid-stride loop covers (CUs x 16 workgroups x 256 threads, dim / 8 per row)"""
    return device_cus() * 16 * 256 // (dim // 8)


def read_arrays(t, info):
    have = {"i8": info["elem_bytes"] == 1, "bf16": info["elem_bytes"] == 2, "blknorm2": info["elem_bytes"] == 2,
            "i4": info["i4_ok"], "i4s": info["i4_ok"], "i8r": info["r2_ok"], "nx": info["nx_valid"], "nxmin": info["nx_valid"],
            "pred": info["pred_model"]}
    return {name: t.derived_read(name) for name in ref.ARRAYS if have[name]}


def derive(t, parts=ref.ALL):
    info = t.derived_info(parts)
    return info, read_arrays(t, info)


def assert_clean(x, t, parts=ref.ALL):
    info, arr = derive(t, parts)
    findings = ref.check(x, info, arr, parts, ratios=RATIOS)
    assert findings == [], "\n".join(findings)
    eb, sc, rs = t.screen_info()
    assert eb == info["elem_bytes"] and ref._bits(sc) == ref._bits(info["s8"]) and ref._bits(rs) == ref._bits(info["resid8"])
    return info, arr


def table_of(ctx, x):
    t = pa.Table(ctx, x.shape[0], x.shape[1])
    t.upload(x)
    return t


def run_clean(ctx, x):
    t = table_of(ctx, x)
    try:
        return assert_clean(x, t)
    finally:
        t.destroy()


def assert_gaps(gaps):
    for name, (top, second) in gaps.items():
        assert second <= 0.8 * top, (name, top, second)


@functools.lru_cache(maxsize=2)
def big_gaussian(dim):
    return ref.gaussian(trip_rows(dim) + 37, dim, 77)


# ---- sizes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", SIZES)
@pytest.mark.parametrize("dim", [128, 64])
def test_sizes(ctx, dim, rows):
    info, _ = run_clean(ctx, ref.gaussian(rows, dim, 100 + rows))
    assert info["elem_bytes"] == (1 if dim == 128 else 2)
    assert info["i4_ok"] == info["r2_ok"] == info["pred_model"] == int(dim == 128)


@pytest.mark.parametrize("dim", [128, 64])
def test_second_ragged_trip_of_the_grid_stride_loop(ctx, dim):
    run_clean(ctx, big_gaussian(dim))


# ---- witness positions ----------------------------------------------------------------------------------------------
def witness_case(ctx, rows, dim, positions, k, col):
    """the witnesses of max |x|, max norm and max residual at positions k, k + 1, k + 2 (cyclically): over k each visits each"""
    positions = list(dict.fromkeys(positions))         # (G + 37 rows at 4 rows per wave: the last wave holds the last row alone)
    n = len(positions)
    p = [positions[(k + i) % n] for i in range(3)]
    assert len(set(p)) == 3
    spare = next(r for r in (rows // 2, rows // 2 + 1, rows // 2 + 2, rows // 2 + 3) if r not in p)
    base = big_gaussian(dim) if rows > 4096 else None
    if dim == 128:
        x, gaps = ref.witness_table(rows, dim, 31 + k, r_abs=p[0], c_abs=col, r_norm=p[1], r_res=p[2], r_res2=spare, base=base)
    else:
        x, gaps = ref.witness_table(rows, dim, 31 + k, r_norm=p[1], base=base)
    assert_gaps(gaps)
    info, _ = run_clean(ctx, x)
    assert info["elem_bytes"] == (1 if dim == 128 else 2)


@pytest.mark.parametrize("col", [0, 7, 8, 127])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_witness_positions(ctx, k, col):
    """row 0, the last row, the first row of the last (ragged) wave; the absmax witness in a thread's first and last value
    and the row's last"""
    run = lambda dim, per_wave: witness_case(ctx, SMALL, dim, [0, SMALL - 1, (SMALL - 1) // per_wave * per_wave], k, col)   # noqa: E731
    run(128, 4)
    if col == 0:
        run(64, 8)


@pytest.mark.parametrize("dim", [128, 64])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_witness_positions_across_the_second_trip(ctx, k, dim):
    """... and rows G - 1 and G of the table whose build takes a second trip"""
    g = trip_rows(dim)
    rows, per_wave = g + 37, 64 // (dim // 8)
    witness_case(ctx, rows, dim, [0, rows - 1, (rows - 1) // per_wave * per_wave, g - 1, g], k, (0, 7, 8, 127, 0)[k])


# ---- hostile values -------------------------------------------------------------------------------------------------
def test_hostile_values(ctx):
    """zero rows, rows below the 4-bit scale floor, -0.0, values at exactly +-absmax, exact half-steps of both scales, equal rows"""
    x = ref.hostile_table()
    info, arr = run_clean(ctx, x)
    assert info["elem_bytes"] == 1 and info["s8"] == 2.0 ** -8
    X8 = arr["i8"].reshape(-1, 128)
    X4 = ref.unpack4(arr["i4"].reshape(-1, 16)[:70], 70)
    R = (arr["i4s"][:70] & np.uint32(0xffff0000)).view(F)
    assert X8[3, 5] == 127 and X8[3, 77] == -127
    for r in (10, 11, 12, 13):
        assert not X8[r].any() and not X4[r].any(), r
    assert R[11] >= np.sqrt(128.0) * 1e-38 and R[12] >= np.sqrt(128.0) * 5e-31          # zero nibbles, and R_r says so
    assert list(X8[15, :8]) == [2, 4, -2, -4, 0, 0, 2, -2] and list(X4[16, :8]) == [0, 2, 2, 0, -2, -2, 7, -7]   # ties to even
    for name, width in (("i8", 128), ("i4", 16), ("i4s", 1), ("i8r", 128), ("nx", 1)):
        a = arr[name].reshape(-1, width)
        assert np.array_equal(a[20], a[40]), name                                      # a row identical to another: equal words


# ---- routing ----------------------------------------------------------------------------------------------------------
def test_routing_and_rebuild_after_reupload(ctx):
    rows = 517
    x = ref.gaussian(rows, 128, 21)
    x[100, 9] = F(0.5)                                   # an outlier one int8 scale still serves
    t = table_of(ctx, x)
    try:
        info, _ = assert_clean(x, t)
        assert info["elem_bytes"] == 1
        y = x.copy()
        y[300, 64] = F(4.0e4)                            # ... and one it does not: bf16 main shadow, no residual shadow, the 4-bit one stays
        t.upload(y)
        info, arr = assert_clean(y, t)
        assert (info["elem_bytes"], info["i4_ok"], info["r2_ok"], info["pred_model"]) == (2, 1, 0, 0)
        assert "i8" not in arr
        with pytest.raises(_lib.PgError, match="pg_table_derived_read.*not built"):
            t.derived_read("i8r")
        z = ref.gaussian(rows, 128, 22)                  # new rows without the outlier: nothing stale survives the rebuild
        t.upload(z)
        info, arr = assert_clean(z, t)
        assert (info["elem_bytes"], info["i4_ok"], info["r2_ok"], info["pred_model"]) == (1, 1, 1, 1)
        assert "bf16" not in arr
        t.upload(y)                                      # each shadow kept across rebuilds and used again: padding still clean
        assert_clean(y, t)
        t.upload(x)
        assert_clean(x, t)
    finally:
        t.destroy()


def test_log_normal_row_scales(ctx):
    rng = np.random.default_rng(5)
    x = (ref.gaussian(1003, 128, 23) * np.exp(rng.standard_normal((1003, 1)) * 3.0)).astype(F)
    info, _ = run_clean(ctx, x)                          # every block's dnorm2 and every R_r
    assert info["elem_bytes"] == 2 and info["i4_ok"] == 1


# ---- non-finite and overflowing rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("kind", ["nan", "+inf", "-inf", "overflow"])
def test_non_finite_rows(ctx, kind, where):
    rows = 70
    x = ref.gaussian(rows, 128, 9)
    r = {"first": 0, "middle": 37, "last": rows - 1}[where]
    if kind == "overflow":
        x[r] = F(1.6e18)                                 # finite, norm^2 = 3.28e38 > 3e38
    else:
        x[r, 77] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[kind]
    t = table_of(ctx, x)
    try:
        info, arr = assert_clean(x, t)
        assert (info["elem_bytes"], info["all_finite"], info["i4_ok"], info["r2_ok"], info["pred_model"]) == (0, 0, 0, 0, 0)
        assert info["nx_valid"] == 1 and np.isfinite(info["l2_slack"]) and sorted(arr) == ["nx", "nxmin"]
        for name in ("i8", "bf16", "blknorm2", "i4", "i4s", "i8r", "pred"):
            with pytest.raises(_lib.PgError, match="pg_table_derived_read.*not built"):
                t.derived_read(name, 0, 1)
        good = ref.gaussian(rows, 128, 10)               # the refusals leave the context and the table usable
        t.upload(good)
        assert_clean(good, t)
    finally:
        t.destroy()


def test_non_finite_rows_dim64(ctx):
    x = ref.gaussian(70, 64, 9)
    x[69, 63] = np.nan
    info, arr = run_clean(ctx, x)
    assert (info["elem_bytes"], info["all_finite"], info["nx_valid"]) == (0, 0, 1) and sorted(arr) == ["nx", "nxmin"]


# ---- lifecycle ----------------------------------------------------------------------------------------------------------
def test_partial_upload_fill_and_swap(ctx):
    rows = 1003
    x, gaps = ref.witness_table(rows, 128, 41, r_abs=5, c_abs=7, r_norm=rows - 1, r_res=600, r_res2=300)
    assert_gaps(gaps)
    a, b = table_of(ctx, x), pa.Table(ctx, rows, 128)
    try:
        assert_clean(x, a)
        # a partial upload moves every witness: the derived data follow
        part, _ = ref.witness_table(200, 128, 42, r_abs=199, c_abs=127, r_norm=0, r_res=100, r_res2=50)
        part[199, 127] = F(0.625)
        x2 = x.copy()
        x2[700:900] = part
        a.upload(part, 700)
        with pytest.raises(_lib.PgError, match="pg_table_derived_read.*not built"):
            a.derived_read("i8", 0, 1)                   # (the rows were written: nothing is current until info is asked)
        assert_clean(x2, a)
        b.fill_synthetic(o.SEED_TABLE)
        y = o.synth_rows(o.SEED_TABLE, 0, rows, 128)
        assert np.array_equal(b.download(0, rows), y)
        info_b, arr_b = assert_clean(y, b)
        info_a, arr_a = derive(a)
        a.swap(b)                                        # the derived data travel with the rows
        got_a, got_arr_a = assert_clean(y, a)
        got_b, got_arr_b = assert_clean(x2, b)
        assert got_a == info_b and got_b == info_a
        for name in arr_a:
            assert np.array_equal(got_arr_b[name], arr_a[name]) and np.array_equal(got_arr_a[name], arr_b[name]), name
    finally:
        a.destroy()
        b.destroy()


def test_parts_are_built_on_request(ctx):
    x = ref.gaussian(333, 128, 51)
    t = table_of(ctx, x)
    try:
        info = t.derived_info(ref.STATS)
        assert (info["elem_bytes"], info["i4_ok"], info["r2_ok"], info["nx_valid"], info["pred_model"]) == (1, 0, 0, 0, 0)
        arr = read_arrays(t, info)
        assert sorted(arr) == ["i8"] and ref.check(x, info, arr, ref.STATS) == []
        info = t.derived_info(ref.I4 | ref.NX)
        assert (info["i4_ok"], info["r2_ok"], info["nx_valid"], info["pred_model"]) == (1, 0, 1, 0)
        assert ref.check(x, info, read_arrays(t, info), ref.I4 | ref.NX) == []
        assert_clean(x, t)
    finally:
        t.destroy()


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    x = ref.gaussian(100, 128, 61)
    t = table_of(ctx, x)
    L = ctx.L
    try:
        out = _lib.PgTableDerived()
        buf = np.zeros(64, np.uint32)
        assert L.pg_table_derived_read(ctx.h, t.h, 0, 0, 1, buf.ctypes.data) == -1          # not built: info was never asked
        assert b"pg_table_derived_read" in L.pg_last_error()
        assert L.pg_table_derived_info(ctx.h, t.h, 32, C.byref(out)) == -1                  # unknown part
        assert b"pg_table_derived_info" in L.pg_last_error()
        assert L.pg_table_derived_info(ctx.h, t.h, 31, None) == -1
        assert L.pg_table_derived_info(ctx.h, None, 31, C.byref(out)) == -1
        assert L.pg_table_derived_info(None, t.h, 31, C.byref(out)) == -1
        assert b"pg_table_derived_info" in L.pg_last_error()
        info = t.derived_info()
        for which in (-1, 9, 1000):
            assert L.pg_table_derived_read(ctx.h, t.h, which, 0, 1, buf.ctypes.data) == -1  # unknown array
            assert b"pg_table_derived_read" in L.pg_last_error()
        assert L.pg_table_derived_read(ctx.h, t.h, 0, 0, 1, None) == -1
        assert L.pg_table_derived_read(None, t.h, 0, 0, 1, buf.ctypes.data) == -1
        assert L.pg_table_derived_read(ctx.h, None, 0, 0, 1, buf.ctypes.data) == -1
        for name in ref.ARRAYS:
            if name in ("bf16", "blknorm2"):
                with pytest.raises(_lib.PgError, match="pg_table_derived_read.*not built"):
                    t.derived_read(name, 0, 1)
                continue
            n = t.derived_len(name)
            for first, cnt in ((n, 1), (n + 1, 0), (0, n + 1), (1, n), (2 ** 64 - 1, 2), (5, 2 ** 64 - 3)):
                assert L.pg_table_derived_read(ctx.h, t.h, _lib.DERIVED_ARRAYS[name], first, cnt, buf.ctypes.data) == -1, (name, first, cnt)
                assert b"pg_table_derived_read" in L.pg_last_error() and b"outside" in L.pg_last_error()
            assert t.derived_read(name, n, 0).size == 0                                     # an empty range at the end is one
            whole = t.derived_read(name)
            assert np.array_equal(t.derived_read(name, n - 3, 3), whole[-3:])               # a following call succeeds
            assert np.array_equal(t.derived_read(name, 1, 2), whole[1:3])
        assert ref.check(x, info, read_arrays(t, info)) == []
    finally:
        t.destroy()


def test_report_tightness_ratios():
    """the largest value / fp64 value this module observed for each tightness cap (printed: check() has asserted every cap)"""
    print("\ntable-derived tightness, largest value / fp64 value:", {k: round(v, 6) for k, v in sorted(RATIOS.items())})
    assert all(RATIOS[k] <= ref.CAPS[k][0] * 1.001 for k in RATIOS if k not in ("resid8", "rmax4", "resid2")), RATIOS
