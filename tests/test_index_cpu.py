"""CPU tests of the exact IVF index (pg_index_*): the ABI is there and refuses NULLs with a message, and the
per-(query, list) bound the search prunes with is restated in numpy and checked to dominate every row's chain score
(o.dot_scores: the specification's k-ascending fp32 fmaf chain) over adversarial data.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import pairec_amd as pa
from pairec_amd import _lib
from oracle import oracle as o
from index_bound_ref import _adversarial, _bound_ip, _bound_neg_l2, _list_side

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
    # the diagnostics: NULL ctx or index refused (every output pointer may be NULL, but not the handles)
    for name in ("pg_index_read", "pg_index_bounds"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    off = np.zeros(2, dtype=np.uint32)
    assert L.pg_index_read(None, None, off.ctypes.data, None, None, None, None) == PG_ERR_INVALID
    assert b"NULL" in L.pg_last_error()
    assert L.pg_index_read(None, None, None, None, None, None, None) == PG_ERR_INVALID
    assert L.pg_index_bounds(None, None, q.ctypes.data, 1, 0, sc.ctypes.data) == PG_ERR_INVALID
    assert b"NULL" in L.pg_last_error()
    assert L.pg_index_bounds(None, None, q.ctypes.data, 1, 1, sc.ctypes.data) == PG_ERR_INVALID


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
