"""CPU tests of the exact IVF index (pg_index_*): the ABI is there and refuses NULLs with a message, and the
per-(query, list) bound the search prunes with is restated in numpy and checked to dominate every row's chain score
(o.dot_scores: the specification's k-ascending fp32 fmaf chain) over adversarial data.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import pairec_amd as pa
from pairec_amd import _lib
from oracle import oracle as o

PG_ERR_INVALID = -1


def test_index_abi_exported_and_refuses_nulls():
    L = _lib.load()
    for name in ("pg_index_build", "pg_index_destroy", "pg_index_recall_topk", "pg_index_recall_topk_dev",
                 "pg_index_recall_topk_l2", "pg_index_recall_topk_l2_dev", "pg_index_stats"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert hasattr(pa, "Index")
    h = C.c_void_p()
    assert L.pg_index_build(None, None, None, C.byref(h)) == PG_ERR_INVALID
    assert b"NULL" in L.pg_last_error()
    assert L.pg_index_build(None, None, None, None) == PG_ERR_INVALID
    rows = np.zeros(4, dtype=np.uint64)
    sc = np.zeros(4, dtype=np.float32)
    q = np.zeros(128, dtype=np.float32)
    for fn in (L.pg_index_recall_topk, L.pg_index_recall_topk_dev, L.pg_index_recall_topk_l2, L.pg_index_recall_topk_l2_dev):
        assert fn(None, None, q.ctypes.data, 1, 4, rows.ctypes.data, sc.ctypes.data, None) == PG_ERR_INVALID
        assert len(L.pg_last_error()) > 0
    assert L.pg_index_stats(None, None) == PG_ERR_INVALID
    st = _lib.PgIndexStats()
    assert L.pg_index_stats(None, C.byref(st)) == PG_ERR_INVALID
    assert L.pg_index_destroy(None, None) == PG_ERR_INVALID


# ---- the bound, restated (index.hip: bound_kernel; all fp64, every table-side input rounded up to fp32 first) -------------
def _up32(v):
    """the smallest float32 >= v (elementwise, v float64)"""
    f = np.asarray(v, dtype=np.float64).astype(np.float32)
    low = f.astype(np.float64) < v
    return np.where(low, np.nextafter(f, np.float32(np.inf)), f)


def _list_side(x, c):
    """r_L and ||c_L|| as the build measures them: fp64, a 2^-40 relative margin, rounded up to fp32"""
    d = x.astype(np.float64) - c.astype(np.float64)
    r = _up32(np.sqrt(np.max(np.sum(d * d, axis=1))) * (1 + 2.0 ** -40))
    cn = _up32(np.sqrt(np.sum(c.astype(np.float64) ** 2)) * (1 + 2.0 ** -40))
    return float(r), float(cn)


def _bound_ip(q, c, r, cn):
    dim = q.shape[1]
    u = 2.0 ** -24
    gam = dim * u / (1 - dim * u)
    qn = np.sqrt(np.sum(q.astype(np.float64) ** 2, axis=1)) * (1 + 2.0 ** -40)
    cq = q.astype(np.float64) @ c.astype(np.float64)
    a = (cn + r) * qn
    slack = gam * a * (1 + 2.0 ** -20) + 2.0 ** -40 * a + dim * 2.0 ** -148
    out = _up32(cq + r * qn + slack)
    return np.where(a * (1 + gam) * 2 < 2.0 ** 127, out, np.inf)


def _bound_neg_l2(q, c, r, cn):
    """upper bound of -d (the search ranks squared Euclidean recalls by -d)"""
    dim = q.shape[1]
    u = 2.0 ** -24
    gam = (dim + 3) * u / (1 - (dim + 3) * u)
    qn = np.sqrt(np.sum(q.astype(np.float64) ** 2, axis=1)) * (1 + 2.0 ** -40)
    s = np.sqrt(np.sum((q.astype(np.float64) - c.astype(np.float64)) ** 2, axis=1)) * (1 - 2.0 ** -40)
    lb = np.maximum(s - r, 0.0)
    lb2 = lb * lb * (1 - 2.0 ** -40)
    b = cn + r + qn
    err = gam * b * b * (1 + 2.0 ** -20) + 2.0 ** -40 * b * b + dim * 2.0 ** -146
    out = _up32(err - lb2)
    return np.where(b * b * 2 < 2.0 ** 126, out, np.inf)


def _adversarial(dim, scale, rng):
    """a list: centroid c and rows around it — some exactly on the sphere of the measured radius, sign patterns that line up
    every term of the chain (maximal rounding), near-duplicates of the centroid; queries: aligned, opposite, one-hot, zero,
    sign-matched"""
    c = (rng.standard_normal(dim) * scale).astype(np.float32)
    signs = np.sign(rng.standard_normal((8, dim))).astype(np.float32)
    dirs = rng.standard_normal((24, dim))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rad = 0.3 * np.linalg.norm(c.astype(np.float64)) + 1e-30
    on_sphere = (c.astype(np.float64) + rad * dirs).astype(np.float32)        # rows at (about) the measured radius
    aligned = (c.astype(np.float64) + rad * signs / np.sqrt(dim)).astype(np.float32)
    near = (c + np.float32(scale) * np.float32(1e-6) * signs[:2]).astype(np.float32)
    x = np.concatenate([on_sphere, aligned, near, c[None, :]]).astype(np.float32)
    onehot = np.zeros((2, dim), dtype=np.float32)
    onehot[0, 0] = 1.0
    onehot[1, dim - 1] = -np.float32(scale)
    q = np.concatenate([
        c[None, :], -c[None, :], signs[:3] * np.float32(scale), aligned[:2], onehot, np.zeros((1, dim), np.float32),
        (rng.standard_normal((3, dim)) * scale).astype(np.float32),
    ]).astype(np.float32)
    return x, c, q


@pytest.mark.parametrize("dim", [64, 128, 256])
@pytest.mark.parametrize("scale", [1.0, 1e-18, 1e17, 3e-39 * 2 ** 20])
def test_bound_dominates_every_chain_score(dim, scale):
    rng = np.random.default_rng(dim * 7 + int(np.log2(scale) + 200))
    x, c, q = _adversarial(dim, scale, rng)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(q))
    r, cn = _list_side(x, c)
    # inner product: U >= fl(x.q) for every row of the list
    s = o.dot_scores(x, q).astype(np.float64)            # [nq][rows]
    U = _bound_ip(q, c, r, cn)
    assert np.all(np.isfinite(s))
    assert np.all(U[:, None] >= s), float(np.max(s - U[:, None]))
    # squared Euclidean: -U_l2 <= fl(d) for every row (d = fmaf(-2, ip, |x|^2 + |q|^2))
    _, dist = o.recall_topk_l2(x, q, x.shape[0])
    assert dist.shape == (q.shape[0], x.shape[0])
    Ul2 = _bound_neg_l2(q, c, r, cn)
    assert np.all(-dist.astype(np.float64) <= Ul2[:, None]), float(np.max(-dist - Ul2[:, None]))


def test_bound_is_tight_enough_to_prune():
    """the bound is not vacuous: on a tight cluster a query far from it gets a bound far below the cluster's own scores"""
    rng = np.random.default_rng(5)
    dim = 128
    c = rng.standard_normal(dim)
    c /= np.linalg.norm(c)
    x = (c + 0.01 * rng.standard_normal((500, dim)) / np.sqrt(dim)).astype(np.float32)
    r, cn = _list_side(x, c.astype(np.float32))
    q_far = (-c).astype(np.float32)[None, :]
    q_near = c.astype(np.float32)[None, :]
    assert _bound_ip(q_far, c.astype(np.float32), r, cn)[0] < -0.9
    near_scores = o.dot_scores(x, q_near)
    assert _bound_ip(q_near, c.astype(np.float32), r, cn)[0] - near_scores.max() < 0.05
