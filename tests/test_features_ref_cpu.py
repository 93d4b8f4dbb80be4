"""Known answers for tests/features_ref.py itself — the restatement the GPU edge tests (tests/test_gpu_features_edges.py) compare
the feature store with.  No GPU, no library: numpy and hand-computed bit patterns only."""
import math
import struct

import numpy as np
import pytest

import features_ref as fr
from features_ref import F32, F64, I32, I64


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def from_bits(b):
    return np.uint32(b).view(np.float32)


# 2^60 + 2^36 lies halfway between the fp32 neighbours 2^60 (0x5D800000) and 2^60 + 2^37 (0x5D800001).  One more rounds up when
# converted directly; a double (53 bits) first drops the 1, lands on the tie and rounds to even: down.
TIE = 2**60 + 2**36


def test_int64_to_fp32_rounds_once_where_a_double_rounds_twice():
    for sign in (1, -1):
        s = 0x80000000 if sign < 0 else 0
        assert f32_bits(fr.to_f32(I64, sign * (TIE + 1))) == 0x5D800001 | s            # above the tie: up
        assert f32_bits(fr.to_f32(I64, sign * (TIE - 1))) == 0x5D800000 | s            # below the tie: down
        assert f32_bits(fr.to_f32(I64, sign * TIE)) == 0x5D800000 | s                  # the tie itself: to even
        assert f32_bits(fr.to_f32(I64, sign * (TIE + 2**37))) == 0x5D800002 | s        # the next tie: to even, up
        # the double rounding this reference must NOT reproduce
        assert f32_bits(np.float32(np.float64(np.int64(sign * (TIE + 1))))) == 0x5D800000 | s
        assert f32_bits(np.float32(np.float64(np.int64(sign * (TIE + 2**37 - 1))))) == 0x5D800002 | s
        assert f32_bits(fr.to_f32(I64, sign * (TIE + 2**37 - 1))) == 0x5D800001 | s
    assert f32_bits(fr.to_f32(I64, 2**63 - 1)) == 0x5F000000                           # INT64_MAX → 2^63
    assert f32_bits(fr.to_f32(I64, -2**63)) == 0xDF000000
    assert f32_bits(fr.to_f32(I32, 2**31 - 1)) == 0x4F000000                           # INT32_MAX → 2^31
    assert f32_bits(fr.to_f32(I32, 16777217)) == 0x4B800000                            # 2^24 + 1: tie, to even
    assert f32_bits(fr.to_f32(I64, 0)) == 0


def test_round_f32_agrees_with_numpy_on_doubles_and_on_the_range_ends():
    rng = np.random.default_rng(7)
    xs = np.concatenate([rng.standard_normal(300) * 10.0 ** rng.integers(-44, 39, 300),
                         [3.4028234663852886e38, 3.4028235677973366e38, 3.402823669209385e38, 1e-45, 7.006492321624085e-46,
                          7.006492321624087e-46, 1.1754943508222875e-38, 1.1754942106924411e-38, 0.1, 1.0]])
    with np.errstate(over="ignore"):
        for x in xs:
            assert f32_bits(fr.to_f32(F64, x)) == f32_bits(np.float32(x)), x
            assert f32_bits(fr.to_f32(F64, -x)) == f32_bits(np.float32(-x)), x


def test_fused_multiply_add_is_fused():
    a = np.float32(1 + 2.0**-12)
    c = np.float32(-(1 + 2.0**-11))
    assert float(fr.fma_f32(a, a, c)) == 2.0**-24                                      # the exact product keeps its 2^-24
    assert np.float32(a * a) + c == 0.0                                                # multiply, round, add: lost
    assert f32_bits(fr.fma_f32(a, a, c)) == 0x33800000
    # exact cancellation is +0, also from a negative product
    assert f32_bits(fr.fma_f32(np.float32(-2.0), np.float32(3.0), np.float32(6.0))) == 0


def test_zero_signs():
    assert f32_bits(fr.fma_f32(np.float32(-0.0), np.float32(1.0), np.float32(0.0))) == 0            # -0·1 + +0 = +0
    assert f32_bits(fr.fma_f32(np.float32(-0.0), np.float32(1.0), np.float32(-0.0))) == 0x80000000  # -0 + -0 = -0
    assert f32_bits(fr.to_f32(F64, -0.0)) == 0x80000000
    cols = {"z": (F64, np.array([-0.0, 0.0]), 0.0), "zf": (F32, np.array([-0.0, 0.0], np.float32), 0.0)}
    assert fr.bits32(fr.gather_f32_ref(cols, [0, 1], ["z", "zf"])).tolist() == [[0, 0], [0, 0]]


def test_fp64_overflow_subnormal_and_nan():
    cols = {"d": (F64, np.array([1e39, -1e39, 1e-40, -1e-40, np.nan, np.inf, -np.inf, 1e-50]), 0.0)}
    got = fr.gather_f32_ref(cols, np.arange(8), ["d"])[:, 0]
    assert got[0] == np.inf and got[1] == -np.inf
    assert f32_bits(got[2]) == 0x000116C2 and f32_bits(got[3]) == 0x800116C2           # the fp32 subnormal nearest 1e-40, kept
    assert got[2] != 0 and abs(float(got[2]) - 1e-40) <= 2.0**-150
    assert np.isnan(got[4]) and got[5] == np.inf and got[6] == -np.inf
    assert f32_bits(got[7]) == 0                                                       # below half the smallest subnormal
    # inf · 0 and inf − inf are NaN, finite overflow in the fmaf is ±inf
    assert np.isnan(fr.fma_f32(np.float32(np.inf), np.float32(0.0), np.float32(1.0)))
    assert np.isnan(fr.fma_f32(np.float32(np.inf), np.float32(1.0), np.float32(-np.inf)))
    big = np.float32(3e38)
    assert fr.fma_f32(big, np.float32(2.0), np.float32(0.0)) == np.inf
    assert fr.fma_f32(big, np.float32(-2.0), big) == -big                              # finite: no intermediate overflow
    # a subnormal result of the fmaf itself
    assert f32_bits(fr.fma_f32(from_bits(0x00800000), np.float32(0.5), np.float32(0.0))) == 0x00400000


def test_integer_gather_saturates():
    v64 = np.array([0, -1, 2**31 - 1, 2**31, -2**31, -2**31 - 1, 2**63 - 1, -2**63], np.int64)
    cols = {"a": (I64, v64, -5), "b": (I32, np.array([0, -1, 2**31 - 1, -2**31, 7, 8, 9, 10], np.int32), 2**31 - 1),
            "f": (F32, np.zeros(8, np.float32), 0.0)}
    got = fr.gather_i32_ref(cols, np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 0xFFFFFFFF], np.uint32), ["a", "b"])
    assert got.dtype == np.int32
    assert got[:, 0].tolist() == [0, -1, 2**31 - 1, 2**31 - 1, -2**31, -2**31, 2**31 - 1, -2**31, -5, -5]
    assert got[:, 1].tolist() == [0, -1, 2**31 - 1, -2**31, 7, 8, 9, 10, 2**31 - 1, 2**31 - 1]
    with pytest.raises(ValueError):
        fr.gather_i32_ref(cols, [0], ["f"])
    # an int64 default beyond int32 is stored whole and saturates only in the int32 view
    cols = {"a": (I64, v64, 2.0**40)}
    assert fr.gather_i32_ref(cols, [8], ["a"])[0, 0] == 2**31 - 1
    assert fr.bind_f64_ref(cols, [8], "a")[0] == 2.0**40


def test_stored_default_per_dtype():
    assert fr.stored_default(F32, 0.1) == float(np.float32(0.1)) == 0.10000000149011612
    assert fr.stored_default(F64, 0.1) == 0.1
    assert fr.stored_default(I32, -7.9) == -7 and fr.stored_default(I64, -7.9) == -7
    assert fr.stored_default(I32, 7.9) == 7 and fr.stored_default(I32, -0.5) == 0
    assert fr.stored_default(I32, 2.0**31 - 1) == 2**31 - 1 and fr.stored_default(I32, -2.0**31) == -2**31
    assert fr.stored_default(I32, 2.0**31 - 0.5) == 2**31 - 1                          # truncates into the range
    assert fr.stored_default(I64, -2.0**63) == -2**63
    assert fr.stored_default(I64, 2.0**63 - 1024) == 2**63 - 1024                      # the largest double below 2^63
    assert math.isnan(fr.stored_default(F32, math.nan)) and fr.stored_default(F64, math.inf) == math.inf
    assert fr.stored_default(F32, 1e39) == math.inf                                    # rounded to the dtype
    for dtype, bad in ((I32, math.nan), (I32, math.inf), (I32, -math.inf), (I32, 2.0**31), (I32, 3e9), (I32, -2.0**31 - 1),
                       (I64, math.nan), (I64, math.inf), (I64, -math.inf), (I64, 2.0**63), (I64, -2.0**64)):
        with pytest.raises(ValueError):
            fr.stored_default(dtype, bad)
    # a NULL-filled column and a row outside the store read the same bits
    for dtype, d in ((F32, 0.1), (F64, 0.1), (I32, -7.9), (I64, 2.0**62)):
        cols = {"c": (dtype, fr.null_column(dtype, 5, d), d)}
        b = fr.bits64(fr.bind_f64_ref(cols, [0, 4, 5, 0xFFFFFFFF], "c"))
        assert len(set(b.tolist())) == 1, dtype
        g = fr.bits32(fr.gather_f32_ref(cols, [0, 4, 5, 0xFFFFFFFF], ["c"]))
        assert len(set(g[:, 0].tolist())) == 1, dtype
    assert struct.pack("<d", fr.stored_default(F32, 0.1)) != struct.pack("<d", 0.1)


def test_clamp_ids():
    ids = [-1, -2**31, 0, 49, 50, 55, 2**40, -2**40, 2**63 - 1, -2**63]
    assert fr.clamp_ids(ids, 50).tolist() == [0, 0, 0, 49, 49, 49, 49, 0, 49, 0]
    assert fr.clamp_ids(np.array([[3, 2**31]], np.int64), 2**31 - 1).tolist() == [[3, 2**31 - 2]]
    assert fr.clamp_ids(ids, 50).dtype == np.int32


def test_gather_f32_applies_scale_and_bias_per_column():
    cols = {"i": (I64, np.array([TIE + 1, 3], np.int64), -1001), "x": (F32, np.array([1 + 2.0**-12, 2.0], np.float32), -2001.0)}
    sc = np.array([1.0, 1 + 2.0**-12], np.float32)
    bi = np.array([0.0, -(1 + 2.0**-11)], np.float32)
    got = fr.gather_f32_ref(cols, [0, 1, 2], ["i", "x"], sc, bi)
    assert f32_bits(got[0, 0]) == 0x5D800001 and got[1, 0] == 3.0 and got[2, 0] == -1001.0
    assert float(got[0, 1]) == 2.0**-24
    only_scale = fr.gather_f32_ref(cols, [1], ["x", "i"], scale=np.array([0.5, 2.0], np.float32))
    assert only_scale.tolist() == [[1.0, 6.0]]
    only_bias = fr.gather_f32_ref(cols, [1], ["x"], bias=np.array([0.25], np.float32))
    assert only_bias.tolist() == [[2.25]]
