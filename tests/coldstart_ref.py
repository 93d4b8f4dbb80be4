"""An independent numpy restatement of ColdStartRecall's answer (include/pairec_gpu.h, "ColdStartRecall"):
np.flatnonzero over the bitmap for the pool, the keyed permutation P in Python ints (and the same arithmetic over numpy uint64
lanes, checked against the ints, where a test needs many slots), np.lexsort for the ordered form.  It shares no code with
csrc/coldstart_host.hpp: the float keys go through an exact widening to float64, the library's through the 32-bit pattern."""
import math

import numpy as np

U64 = (1 << 64) - 1
U64MAX = np.uint64(U64)
GOLDEN = 0x9E3779B97F4A7C15
ROUNDS = 8


def mix(x: int) -> int:
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & U64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & U64
    return x ^ (x >> 31)


def half_bits(A: int) -> int:
    b = 2
    while (1 << b) < A:
        b += 2
    return b // 2


def step(seed: int, x: int, h: int) -> int:
    mask = (1 << h) - 1
    L, R = x >> h, x & mask
    for r in range(ROUNDS):
        L, R = R, L ^ (mix((seed + GOLDEN * (1 + (r << 32) + R)) & U64) & mask)
    return (L << h) | R


def perm(seed: int, A: int, i: int) -> int:
    """P(i) in Python ints"""
    h = half_bits(A)
    x = step(seed, i, h)
    while x >= A:
        x = step(seed, x, h)
    return x


def _mix_np(x):
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def perm_np(seed: int, A: int, n: int) -> np.ndarray:
    """P(0 .. n - 1), n <= A, over uint64 lanes (wrapping arithmetic)"""
    h = half_bits(A)
    hh, mask, sd = np.uint64(h), np.uint64((1 << h) - 1), np.uint64(seed)
    x = np.arange(n, dtype=np.uint64)
    todo = np.ones(n, dtype=bool)
    with np.errstate(over="ignore"):
        while todo.any():
            v = x[todo]
            L, R = v >> hh, v & mask
            for r in range(ROUNDS):
                f = _mix_np(sd + np.uint64(GOLDEN) * (np.uint64(1 + (r << 32)) + R)) & mask
                L, R = R, L ^ f
            x[todo] = (L << hh) | R
            todo = x >= np.uint64(A)
    return x


def keys(col: np.ndarray, desc: bool) -> np.ndarray:
    """order-preserving uint64 keys of a column; desc complements them"""
    col = np.asarray(col)
    if col.dtype in (np.int32, np.int64):
        k = col.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    else:
        with np.errstate(invalid="ignore"):                   # (signalling NaNs)
            d = col.astype(np.float64) + 0.0                  # exact widening; -0.0 + 0.0 = +0.0
        b = d.view(np.uint64)
        k = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))
        k = np.where(np.isnan(d), U64MAX, k)
    return ~k if desc else k


def pool(bits, rows: int) -> np.ndarray:
    if bits is None:
        return np.arange(rows, dtype=np.int64)
    b = np.unpackbits(np.ascontiguousarray(bits, dtype="<u4").view(np.uint8), bitorder="little")[:rows]
    return np.flatnonzero(b)


def recall(order_by, bits, rows: int, nq: int, k: int, col=None, seed=None, row_offset: int = 0):
    """order_by: None (random), "asc" or "desc" → (rows [nq][k] u64, scores [nq][k] f32, counts [nq] u32)"""
    sel = pool(bits, rows)
    A = len(sel)
    kk = min(k, A)
    out_r = np.full((nq, k), U64MAX, dtype=np.uint64)
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_s[:, :kk] = 0.0
    if kk and order_by is not None:
        ky = keys(np.asarray(col)[sel], order_by == "desc")
        head = sel[np.lexsort((sel, ky))][:kk]
        out_r[:, :kk] = (head + row_offset).astype(np.uint64)
    elif kk:
        for q in range(nq):
            s = 0 if seed is None else int(seed[q])
            out_r[q, :kk] = (sel[perm_np(s, A, kk).astype(np.int64)] + row_offset).astype(np.uint64)
    return out_r, out_s, np.full(nq, kk, dtype=np.uint32)


def chi2_quantile_999(dof: int) -> float:
    """the 0.999 quantile of chi-square: scipy's if importable, else Wilson-Hilferty"""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(0.999, dof))
    except Exception:
        z = 3.090232306167813
        return dof * (1.0 - 2.0 / (9.0 * dof) + z * math.sqrt(2.0 / (9.0 * dof))) ** 3


def same(got, want, what=""):
    for name, g, w in zip(("rows", "scores", "count"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        gb, wb = g.view(np.uint8 if g.dtype.itemsize == 1 else "u%d" % g.dtype.itemsize), w.view("u%d" % w.dtype.itemsize)
        if not np.array_equal(gb, wb):
            at = np.argwhere(gb != wb)[0]
            raise AssertionError("%s: %s differs first at %s: got %s, want %s (%d of %d differ)" %
                                 (what, name, tuple(at), g[tuple(at)], w[tuple(at)], int((gb != wb).sum()), gb.size))
