"""The checker of a table's derived recall data (tests/table_derived_ref.py) would notice: no GPU.  A numpy stand-in for the device
(the exact layer plus the documented padded bounds) passes check() on the table family of test_gpu_table_derived.py, and each
plausible kernel error, applied to that answer one at a time, is reported.  The sensitivity rests on witnesses: max |x|, the max
norm and the max residuals are each decided by one row, with the runner-up at most 0.8 of it (asserted for every table)."""
import numpy as np
import pytest

import table_derived_ref as ref
from table_derived_ref import F, PAD, BLK

SIZES = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1000)
ROWS = 1003                      # the mutation table: ragged last wave, ragged last block, sample no multiple of 16


def witness128(rows=ROWS, seed=5, **kw):
    pos = dict(r_abs=rows - 1, c_abs=127, r_norm=(rows - 1) // 4 * 4, r_res=0, r_res2=rows // 2)
    pos.update(kw)
    return ref.witness_table(rows, 128, seed, **pos)


def assert_gaps(gaps):
    for name, (top, second) in gaps.items():
        assert second <= 0.8 * top, (name, top, second)


@pytest.fixture(scope="module")
def base():
    x, gaps = witness128()
    assert_gaps(gaps)
    info, arr = ref.model(x)
    assert ref.check(x, info, arr) == []
    return x, info, arr


def mutated(base):
    x, info, arr = base
    return x, dict(info), {k: v.copy() for k, v in arr.items()}


def reported(findings, word):
    assert any(word in s for s in findings), findings


@pytest.mark.parametrize("dim", [64, 128])
def test_model_passes_on_every_size(dim):
    ratios = {}
    for rows in SIZES:
        x = ref.gaussian(rows, dim, 100 + rows)
        info, arr = ref.model(x)
        assert ref.check(x, info, arr, ratios=ratios) == [], (rows, dim)
        assert info["elem_bytes"] == (1 if dim == 128 else 2)
    assert all(ratios[k] <= ref.CAPS[k][0] for k in ratios), ratios


def test_model_passes_on_witness_hostile_and_routed_tables():
    for dim, kw in ((128, {}), (64, dict(r_abs=None, r_res=None, r_res2=None))):
        x, gaps = ref.witness_table(ROWS, dim, 3, **dict(dict(r_abs=7, c_abs=8, r_norm=ROWS - 1, r_res=500, r_res2=0), **kw))
        assert_gaps(gaps)
        assert ref.check(x, *ref.model(x)) == []
    x = ref.hostile_table()
    info, arr = ref.model(x)
    assert info["elem_bytes"] == 1 and ref.check(x, info, arr) == []
    X4 = ref.unpack4(arr["i4"].reshape(-1, 16)[:70], 70)
    assert not X4[11].any() and not X4[12].any()                       # below the 4-bit scale floor: the nibbles are zero ...
    R = (arr["i4s"][:70] & np.uint32(0xffff0000)).view(F)
    assert R[12] >= np.sqrt(128.0) * 5e-31                             # ... and R_r says so
    assert list(X4[16, :8]) == [0, 2, 2, 0, -2, -2, 7, -7]             # ties go to even
    assert list(arr["i8"].reshape(-1, 128)[15, :8]) == [2, 4, -2, -4, 0, 0, 2, -2]
    # an outlier of 4.0e4 defeats one int8 scale: bf16 main shadow, no residual shadow, the 4-bit shadow stays
    x = ref.gaussian(100, 128, 4)
    x[50, 3] = F(4.0e4)
    info, arr = ref.model(x)
    assert (info["elem_bytes"], info["i4_ok"], info["r2_ok"], info["pred_model"]) == (2, 1, 0, 0)
    assert ref.check(x, info, arr) == []
    # non-finite rows: no shadow, |x|^2 all the same
    for bad in (np.nan, np.inf, -np.inf):
        x = ref.gaussian(70, 128, 9)
        x[33, 4] = bad
        info, arr = ref.model(x)
        assert (info["elem_bytes"], info["all_finite"], info["nx_valid"]) == (0, 0, 1)
        assert ref.check(x, info, arr) == []


@pytest.mark.parametrize("which,word", [("absmax", "s8 ="), ("max_norm", "max_norm"), ("resid8", "resid8"), ("rmax4", "rmax4"),
                                         ("resid2", "resid2")])
def test_witness_row_left_out_of_a_maximum(base, which, word):
    """the last ragged wave dropped, or the grid-stride loop's second trip"""
    x = base[0]
    info, arr = ref.model(x, leave_out=which)
    f = ref.check(x, info, arr)
    reported(f, word)
    assert any("BELOW" in s or "s8 =" in s for s in f), f


def test_witness_row_left_out_of_a_block_norm():
    x, gaps = ref.witness_table(ROWS, 64, 8, r_norm=ROWS - 1)
    assert_gaps(gaps)
    info, arr = ref.model(x)
    assert ref.check(x, info, arr) == []
    b = (ROWS - 1) // BLK
    arr["blknorm2"][b] = np.sum(x[b * BLK:ROWS - 1].astype(np.float64) ** 2, axis=1).max()
    reported(ref.check(x, info, arr), "dnorm2[%d]" % b)


def test_block_norm_written_to_the_next_block():
    x, gaps = ref.witness_table(ROWS, 64, 8, r_norm=40)
    assert_gaps(gaps)
    info, arr = ref.model(x)
    arr["blknorm2"] = np.roll(arr["blknorm2"], 1)
    reported(ref.check(x, info, arr), "BELOW ||x||")


def test_residual_bound_swapped_with_the_neighbour(base):
    x, info, arr = mutated(base)
    r = (ROWS - 1) // 4 * 4                                           # the norm witness: its residual is the table's largest
    hi = arr["i4s"] & np.uint32(0xffff0000)
    assert hi[r] > hi[r + 1]
    arr["i4s"][r], arr["i4s"][r + 1] = (arr["i4s"][r] & 0xffff) | hi[r + 1], (arr["i4s"][r + 1] & 0xffff) | hi[r]
    reported(ref.check(x, info, arr), "R_r")


def test_one_nibble_off_by_one(base):
    x, info, arr = mutated(base)
    arr["i4"][16 * 501 + 9] += np.uint32(1 << 12)
    f = ref.check(x, info, arr)
    reported(f, "nibbles differs at row 501 column %d" % (8 * 9 + 4 + 1))


def test_ties_rounded_away_from_zero():
    x = ref.hostile_table()
    info, arr = ref.model(x)
    t = x.astype(np.float64) * 256.0
    away = np.clip(np.sign(t) * np.floor(np.abs(t) + 0.5), -127, 127).astype(np.int8)
    assert np.count_nonzero(away != arr["i8"].reshape(-1, 128)[:70]) >= 16
    arr["i8"].reshape(-1, 128)[:70] = away
    reported(ref.check(x, info, arr), "X8 differs at row 15 column 0")


def test_row_scale_rounded_to_nearest(base):
    x, info, arr = mutated(base)
    amax = np.max(np.abs(x), axis=1).astype(F)
    near = ref.bf16_nearest((amax / F(7.0)).astype(F)).view(np.uint32) >> 16
    assert np.count_nonzero(near != (arr["i4s"][:ROWS] & 0xffff)) > ROWS // 4
    arr["i4s"][:ROWS] = (arr["i4s"][:ROWS] & np.uint32(0xffff0000)) | near
    reported(ref.check(x, info, arr), "s_r (bf16 bits) differs")


def test_norms_as_a_plain_sum(base):
    x, info, arr = mutated(base)
    plain = np.zeros(ROWS, F)
    for c in range(128):
        plain = (plain + (x[:, c] * x[:, c]).astype(F)).astype(F)
    differ = np.flatnonzero(plain != arr["nx"][:ROWS])
    assert differ.size > ROWS // 4                                    # (the two differ on most rows)
    arr["nx"][differ[:3]] = plain[differ[:3]]
    arr["nxmin"] = ref.nxmin_of(arr["nx"], ROWS)
    reported(ref.check(x, info, arr), "nx differs at row %d" % differ[0])


def test_block_minimum_includes_a_row_past_the_end(base):
    x, info, arr = mutated(base)
    assert ROWS % BLK
    arr["nxmin"][-1] = min(arr["nxmin"][-1], arr["nx"][ROWS])         # the padding row's zero
    reported(ref.check(x, info, arr), "nxmin differs at row %d" % (ROWS // BLK))


@pytest.mark.parametrize("name,width", [("i8", 128), ("i4", 16), ("i4s", 1), ("i8r", 128), ("nx", 1)])
def test_a_padding_row_is_not_clean(base, name, width):
    x, info, arr = mutated(base)
    arr[name][(ROWS + PAD - 1) * width] = 1
    reported(ref.check(x, info, arr), "differs")
    x, gaps = ref.witness_table(ROWS, 64, 8, r_norm=40)
    assert_gaps(gaps)
    info, arr = ref.model(x)
    arr["bf16"][(ROWS + 1) * 64 + 3] = 0x3f80
    reported(ref.check(x, info, arr), "bf16 padding differs")


def test_covariance_without_its_last_partial_stage(base):
    x, info, arr = mutated(base)
    assert ROWS % 16
    xs = x.astype(np.float64)[:ROWS // 16 * 16]
    mean = np.sum(xs, axis=0) / ROWS
    cov = xs.T @ xs / ROWS - np.outer(mean, mean)
    arr["pred"][128:128 + 128 * 128] = cov.astype(F).reshape(-1).view(np.uint32)
    reported(ref.check(x, info, arr), "pred covariance")
    x, info, arr = mutated(base)
    arr["pred"][128 + 128 * 128:].view(np.float64)[3] = 0.0
    reported(ref.check(x, info, arr), "observation block")


def test_entries_refuse_null_arguments_without_a_device():
    """the argument checks come before anything touches the GPU (as tests/test_index_cpu.py does for the index's diagnostics)"""
    import ctypes as C
    from pairec_amd import _lib
    L = _lib.load()
    out, buf = _lib.PgTableDerived(), np.zeros(4, np.uint32)
    assert L.pg_table_derived_info(None, None, _lib.DERIVED_ALL, C.byref(out)) == -1
    assert b"pg_table_derived_info" in L.pg_last_error()
    assert L.pg_table_derived_read(None, None, 0, 0, 1, buf.ctypes.data) == -1
    assert b"pg_table_derived_read" in L.pg_last_error()
    assert C.sizeof(_lib.PgTableDerived) == 80                 # pg_table_derived_t: 15 four-byte fields, padding, two uint64
