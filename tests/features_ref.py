"""The feature store's gathers (csrc/features.hip, pg_features_*) restated in numpy and Python alone — no GPU, no library.
The three rules it states are the ones of include/pairec_gpu.h (pg_features_set_column: THE STORED DEFAULT;
pg_features_gather_f32_dev: DIRECT CONVERSION; pg_rank_fm2t_rows_dev: THE CLAMP ON ITEM IDS) and DESIGN.md §5.8.

A store is a dict {name: (dtype, values, default)}: `values` an array of the store's row count in the dtype's numpy type
(`null_column` makes the one a NULL fill stores), `default` the caller's double.  tests/test_features_ref_cpu.py holds the known
answers of this file; tests/test_gpu_features_edges.py compares the device with it bit for bit."""
import math
from fractions import Fraction

import numpy as np

I32, I64, F32, F64 = 1, 2, 3, 4                      # pg_feature_dtype
NP = {I32: np.int32, I64: np.int64, F32: np.float32, F64: np.float64}
INT_RANGE = {I32: (-2**31, 2**31 - 1), I64: (-2**63, 2**63 - 1)}


def stored_default(dtype, default):
    """The ONE default of a column: `default` (a double) rounded to the dtype.  F32: (double)(float)default; F64: default; I32 / I64:
    the integer truncated toward zero (a Python int) — ValueError for NaN, an infinity or a value outside the dtype's range."""
    d = float(default)
    if dtype == F64:
        return d
    if dtype == F32:
        with np.errstate(over="ignore"):
            return float(np.float32(d))
    if not math.isfinite(d):
        raise ValueError("default %r is not an integer value" % d)
    t = math.trunc(d)                                # exact: a Python int
    lo, hi = INT_RANGE[dtype]
    if not lo <= t <= hi:
        raise ValueError("default %r outside the range of the dtype" % d)
    return t


def null_column(dtype, n, default):
    """what set_column(values=NULL) stores: every row the stored default"""
    return np.full(n, stored_default(dtype, default), dtype=NP[dtype])


def at_rows(col, rows):
    """column values at `rows` in the column's own type; a row >= n reads the stored default"""
    dtype, values, default = col
    values = np.asarray(values, dtype=NP[dtype])
    n = values.shape[0]
    rows = np.asarray(rows, dtype=np.uint32).astype(np.int64)
    inside = rows < n
    out = np.full(rows.shape[0], stored_default(dtype, default), dtype=NP[dtype])
    out[inside] = values[rows[inside]]
    return out


def gather_i32_ref(cols, rows, names):
    """pg_features_gather_i32_dev → [n][len(names)] int32: int64 saturates to int32, a row >= n reads the stored default"""
    out = np.empty((len(rows), len(names)), dtype=np.int32)
    for f, name in enumerate(names):
        if cols[name][0] not in (I32, I64):
            raise ValueError("column %r is not an integer column" % name)
        out[:, f] = np.clip(at_rows(cols[name], rows).astype(np.int64), -2**31, 2**31 - 1)
    return out


def round_f32(q):
    """An exact rational → the nearest fp32, ties to even, subnormals kept, ±inf past the range.  The two neighbours are told
    apart by exact comparison; the result n·2^e (n < 2^25) then passes through a double unchanged.  q = 0 gives +0.0."""
    q = Fraction(q)
    if q == 0:
        return np.float32(0.0)
    m = abs(q)
    e = m.numerator.bit_length() - m.denominator.bit_length()       # floor(log2 m) or one more
    if Fraction(2) ** e > m:
        e -= 1
    e = max(e, -126)                                                   # below the normals the spacing stays 2^-149
    k = m / Fraction(2) ** (e - 23)                                    # in units of the spacing: [2^23, 2^24) for a normal
    n = k.numerator // k.denominator
    rem = k - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    if e > 127 or (e == 127 and n >= 2**24):
        v = math.inf
    else:
        v = math.ldexp(n, e - 23)                                      # exact in a double (n <= 2^24, e - 23 >= -149)
    return np.float32(-v if q < 0 else v)


def to_f32(dtype, x):
    """(float)value with ONE rounding: an integer converts directly (never through a double), an fp64 is (float)double"""
    if dtype in (I32, I64):
        return round_f32(Fraction(int(x)))
    x = float(x)
    if not math.isfinite(x):
        return np.float32(x)
    if x == 0.0:
        return np.float32(x)                                           # keeps the zero's sign
    return round_f32(Fraction(x))


def fma_f32(a, b, c):
    """One true fp32 fmaf: a·b + c exact, rounded once.  Finite operands by exact arithmetic; NaN and infinities from numpy's IEEE
    arithmetic in fp64 (the product of two fp32 is exact there and cannot overflow)."""
    a, b, c = np.float32(a), np.float32(b), np.float32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore"):
            return np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    q = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if q == 0:
        if (a == 0 or b == 0) and c == 0:                              # a sum of two zeros: IEEE's sign rule, from numpy
            return np.float32(np.float64(a) * np.float64(b) + np.float64(c))
        return np.float32(0.0)                                         # exact cancellation: +0 (round to nearest)
    return round_f32(q)


def gather_f32_ref(cols, rows, names, scale=None, bias=None):
    """pg_features_gather_f32_dev → [n][len(names)] fp32: fmaf((float)value, scale[f], bias[f]), scale = 1 / bias = +0 when None"""
    out = np.empty((len(rows), len(names)), dtype=np.float32)
    for f, name in enumerate(names):
        dtype = cols[name][0]
        s = np.float32(1.0) if scale is None else np.float32(scale[f])
        b = np.float32(0.0) if bias is None else np.float32(bias[f])
        for i, x in enumerate(at_rows(cols[name], rows)):
            out[i, f] = fma_f32(to_f32(dtype, x), s, b)
    return out


def bind_f64_ref(cols, rows, name):
    """what pg_features_eval_dev binds to a variable: (double)value, the stored default for a row outside the store"""
    return at_rows(cols[name], rows).astype(np.float64)


def clamp_ids(ids, vocab):
    """The rule for FM item field ids: saturate to int32, then clamp to [0, vocab - 1]"""
    ids = np.clip(np.asarray(ids).astype(np.int64), -2**31, 2**31 - 1)
    return np.clip(ids, 0, int(vocab) - 1).astype(np.int32)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
