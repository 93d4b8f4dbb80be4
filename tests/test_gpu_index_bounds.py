"""GPU tests of the exact IVF index's device state (pg_index_read, pg_index_bounds) against fp64: the build's
offsets, permutation, centroid norms and radii, and the per-(query, list) bound U the search prunes with.  U must dominate every
chain score of the list's rows (soundness) and equal the numpy restatement of tests/index_bound_ref.py to one fp32 ulp, +inf
exactly where the restatement is +inf (tightness: an all-+inf kernel is sound and would prune nothing).  Tables: adversarial lists
at scales 1, 1e-18, 1e17 and near the fp32 underflow, a mixture, all-equal rows; n_lists 1, a middle value and rows / 64."""
import numpy as np
import pytest

import pairec_amd as pa
from oracle import oracle as o
from index_bound_ref import _adversarial, _bound_ip, _bound_neg_l2, _cnorm, _list_side

pytestmark = pytest.mark.gpu

SCALES = (1.0, 1e-18, 1e17, 3e-39 * 2 ** 20)
GAP = 1e-3                    # relative distance of the cutoff queries from the +inf cutoff


def _table(ctx, tab):
    t = pa.Table(ctx, tab.shape[0], tab.shape[1])
    t.upload(tab)
    return t


def _gam(dim, l2):
    dd = dim + (3 if l2 else 0)
    return dd * 2.0 ** -24 / (1 - dd * 2.0 ** -24)


def _qnorm(q):
    return np.sqrt(np.sum(q.astype(np.float64) ** 2, axis=1)) * (1 + 2.0 ** -40)


def check_build_state(tab, st):
    """offsets, permutation, ||c_L|| and r_L against fp64 over the rows the permutation puts in each list"""
    rows = tab.shape[0]
    off, perm, cent, cnorm, rad = st["offsets"], st["perm"], st["centroids"], st["cnorm"], st["radius"]
    nl = cent.shape[0]
    assert off[0] == 0 and off[-1] == rows and np.all(np.diff(off.astype(np.int64)) >= 0)
    assert np.array_equal(np.sort(perm), np.arange(rows, dtype=np.uint32))
    starts = np.zeros(rows, bool)
    starts[off[:-1][off[:-1] < rows]] = True
    assert np.all((np.diff(perm.astype(np.int64)) > 0) | starts[1:]), "a list's rows are not in ascending source order"
    c64 = cent.astype(np.float64)
    for L in range(nl):
        cn_exact = np.sqrt(np.sum(c64[L] ** 2))
        assert cnorm[L] >= cn_exact, (L, cnorm[L], cn_exact)
        assert cnorm[L] <= np.nextafter(np.float32(_cnorm(cent[L])), np.float32(np.inf)), (L, cnorm[L], _cnorm(cent[L]))
        x = tab[perm[off[L]:off[L + 1]]]
        if x.shape[0] == 0:
            assert rad[L] == 0, (L, rad[L])
            continue
        d = x.astype(np.float64) - c64[L]
        r_exact = np.sqrt(np.max(np.sum(d * d, axis=1)))
        assert rad[L] >= r_exact, (L, float(rad[L]), r_exact)
        r_ref, _ = _list_side(x, cent[L])
        assert rad[L] <= np.nextafter(np.float32(r_ref), np.float32(np.inf)), (L, float(rad[L]), r_ref)


def reference_bounds(q, st, l2):
    cent, cnorm, rad = st["centroids"], st["cnorm"], st["radius"]
    nl = cent.shape[0]
    out = np.empty((q.shape[0], nl), np.float64)
    tol = np.empty_like(out)
    qn = _qnorm(q)
    with np.errstate(over="ignore", invalid="ignore"):
        for L in range(nl):
            r, cn = float(rad[L]), float(cnorm[L])
            if l2:
                out[:, L] = _bound_neg_l2(q, cent[L], r, cn)
                tol[:, L] = 2.0 ** -44 * (cn + r + qn) ** 2
            else:
                out[:, L] = _bound_ip(q, cent[L], r, cn)
                tol[:, L] = 2.0 ** -44 * (cn + r) * qn
    return out, tol


def chain_maxima(tab, q, st, l2):
    """[nq][n_lists] the largest chain score of each list's rows (-d for l2); -inf for an empty list"""
    off, perm = st["offsets"], st["perm"]
    nl = off.shape[0] - 1
    if l2:
        rows, dist = o.recall_topk_l2(tab, q, tab.shape[0])
        S = np.empty((q.shape[0], tab.shape[0]), np.float32)
        np.put_along_axis(S, rows.astype(np.int64), -dist, axis=1)
    else:
        S = o.dot_scores(tab, q)
    Sp = S[:, perm.astype(np.int64)]
    out = np.full((q.shape[0], nl), -np.inf, np.float64)
    live = np.nonzero(off[1:] > off[:-1])[0]
    if live.size:
        out[:, live] = np.maximum.reduceat(Sp, off[live].astype(np.int64), axis=1)
    return out


def check_bounds(ix, tab, q, st, l2):
    U = ix.bounds(q, l2=l2)
    assert U.shape == (q.shape[0], st["centroids"].shape[0]) and U.dtype == np.float32
    assert not np.any(np.isnan(U))
    ref, tol = reference_bounds(q, st, l2)
    # +inf exactly where the restatement is
    assert np.array_equal(np.isinf(U), np.isinf(ref)), np.argwhere(np.isinf(U) != np.isinf(ref))[:8]
    assert not np.any(np.isneginf(U))
    # tightness: one fp32 ulp of the restatement (or the fp64 evaluation order's few-ulp-of-2^-53 difference)
    fin = np.isfinite(ref)
    diff = np.abs(U.astype(np.float64) - np.where(fin, ref, 0.0))
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    bad = fin & ~(diff <= np.maximum(ulp, tol))
    assert not np.any(bad), [(int(a), int(b), float(U[a, b]), float(ref[a, b])) for a, b in np.argwhere(bad)[:8]]
    # soundness: U >= every chain score of the list's rows
    m = chain_maxima(tab, q, st, l2)
    fu = np.isfinite(U)
    assert not np.any(np.isnan(m[fu]) | np.isposinf(m[fu])), "a chain score overflowed under a finite bound"
    low = fu & (U.astype(np.float64) < m)
    assert not np.any(low), [(int(a), int(b), float(U[a, b]), float(m[a, b])) for a, b in np.argwhere(low)[:8]]
    return U, ref


def cutoff_queries(st, dim, l2):
    """two queries along the centroid of the list L with the largest ||c|| + r that put L just below and just above the +inf
    cutoff of the inner-product bound ((||c|| + r) ||q|| (1 + gamma) 2 < 2^127) or of the squared Euclidean one
    ((||c|| + r + ||q||)^2 2 < 2^126); none when such a query is not representable in fp32"""
    side = st["cnorm"].astype(np.float64) + st["radius"].astype(np.float64)
    L = int(np.argmax(side))
    c = st["centroids"][L].astype(np.float64)
    u = c / np.linalg.norm(c) if np.any(c) else np.full(dim, dim ** -0.5)
    out = []
    for f in (1 - GAP, 1 + GAP):
        if l2:
            target = f * 2.0 ** 62.5 - side[L]
        else:
            target = f * 2.0 ** 126 / ((1 + _gam(dim, False)) * side[L])
        qv = u * target
        if not (target > 0 and np.all(np.abs(qv) < 1e38)):
            return np.zeros((0, dim), np.float32), L
        out.append(qv.astype(np.float32))
    return np.stack(out), L


def queries_for(tab, st, rng, extra):
    dim = tab.shape[1]
    cent = st["centroids"]
    live = np.nonzero(st["offsets"][1:] > st["offsets"][:-1])[0]
    pick = live[rng.permutation(live.size)[:4]]
    scale = float(np.max(np.abs(tab))) or 1.0
    onehot = np.zeros((2, dim), np.float32)
    onehot[0, 0] = 1.0
    onehot[1, dim - 1] = -np.float32(scale)
    signs = np.sign(rng.standard_normal((4, dim))).astype(np.float32) * np.float32(scale)
    return np.concatenate([np.zeros((1, dim), np.float32), onehot, cent[pick], -cent[pick],
                           tab[rng.integers(0, tab.shape[0], 8)], signs, extra]).astype(np.float32)


def run_table(ctx, tab, n_lists_set, rng, extra_q):
    t = _table(ctx, tab)
    dim = tab.shape[1]
    try:
        for nl in n_lists_set:
            ix = pa.Index(ctx, t, n_lists=nl)
            try:
                st = ix.read()
                assert st["centroids"].shape == (nl, dim), (nl, st["centroids"].shape)
                check_build_state(tab, st)
                q = queries_for(tab, st, rng, extra_q)
                for l2 in (False, True):
                    cq, L = cutoff_queries(st, dim, l2)
                    qq = np.concatenate([q, cq]).astype(np.float32)
                    U, ref = check_bounds(ix, tab, qq, st, l2)
                    if cq.shape[0]:
                        # the two cutoff queries straddle the cutoff for list L: finite below, +inf above
                        assert np.isfinite(ref[-2, L]) and np.isinf(ref[-1, L]), (l2, ref[-2:, L])
                        assert np.isfinite(U[-2, L]) and np.isinf(U[-1, L]), (l2, U[-2:, L])
            finally:
                ix.destroy()
    finally:
        t.destroy()


@pytest.mark.parametrize("dim", [64, 128, 256])
@pytest.mark.parametrize("scale", SCALES)
def test_bounds_on_adversarial_lists(ctx, dim, scale):
    rng = np.random.default_rng(dim * 131 + int(np.log2(scale) + 200))
    parts, qs = [], []
    for i in range(48):
        x, c, q = _adversarial(dim, scale, rng)
        parts.append(x)
        if i < 3:
            qs.append(q)
    tab = np.concatenate(parts).astype(np.float32)
    assert np.all(np.isfinite(tab))
    run_table(ctx, tab, (1, 7, tab.shape[0] // 64), rng, np.concatenate(qs))


def test_bounds_on_a_mixture(ctx):
    rng = np.random.default_rng(41)
    n, d = 50_000, 128
    tab = o.synth_mixture_rows(41, 0, n, d, 40, 0.1)
    q = o.synth_mixture_rows(41, 9, 24, d, 40, 0.1, stream=1)
    run_table(ctx, tab, (1, 64, n // 64), rng, q)


def test_bounds_on_equal_rows(ctx):
    """radius 0 for the list that holds every row, empty lists everywhere else"""
    rng = np.random.default_rng(43)
    d = 128
    tab = np.tile(rng.standard_normal(d).astype(np.float32), (4096, 1))
    t = _table(ctx, tab)
    ix = pa.Index(ctx, t, n_lists=64)
    try:
        st = ix.read()
        sizes = np.diff(st["offsets"].astype(np.int64))
        assert sizes.max() == 4096 and np.count_nonzero(sizes) == 1 and st["radius"].max() == 0
    finally:
        ix.destroy()
        t.destroy()
    run_table(ctx, tab, (1, 8, 64), rng, rng.standard_normal((4, d)).astype(np.float32))


def test_bounds_refusals(ctx):
    tab = o.synth_rows(o.SEED_TABLE, 0, 4096, 64)
    t = _table(ctx, tab)
    ix = pa.Index(ctx, t, n_lists=8)
    try:
        q = np.zeros((257, 64), np.float32)
        out = np.zeros((257, 8), np.float32)
        assert ctx.L.pg_index_bounds(ctx.h, ix.h, q.ctypes.data, 257, 0, out.ctypes.data) == -1
        assert ctx.L.pg_index_bounds(ctx.h, ix.h, q.ctypes.data, 0, 0, out.ctypes.data) == -1
        assert ctx.L.pg_index_bounds(ctx.h, ix.h, None, 1, 0, out.ctypes.data) == -1
        assert ctx.L.pg_index_read(ctx.h, ix.h, None, None, None, None, None) == 0      # every output may be NULL
        assert ix.bounds(q[:256]).shape == (256, 8)
    finally:
        ix.destroy()
        t.destroy()
