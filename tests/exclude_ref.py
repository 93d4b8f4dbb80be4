"""The recalls with per-request exclusion lists, restated in numpy on the CPU oracle alone: for every request
the oracle's recall at depth k + n_q (n_q = the length of its list), the listed ids dropped, the rest cut to k and padded.  The
tests' expectations come from here; tests/test_exclude_cpu.py checks the restatement itself against an oracle recall over the
table with the excluded rows physically removed."""
import numpy as np

from oracle import oracle as o

U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def plain_top(tab, q, depth, l2=False, row_offset=0, mask=None):
    """the oracle's answer of ONE query at `depth` (as many entries as there are candidates, unpadded): global ids, scores;
    mask: only the rows it admits are candidates (the oracle over those rows, ids mapped back)"""
    q = np.ascontiguousarray(q, np.float32).reshape(1, -1)
    fn = o.recall_topk_l2 if l2 else o.recall_topk
    if mask is None:
        rows, sc = fn(tab, q, depth)
        return rows[0] + np.uint64(row_offset), sc[0]
    ids = np.flatnonzero(mask)
    if ids.size == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.float32)
    rows, sc = fn(tab[ids], q, depth)
    return ids[rows[0].astype(np.int64)].astype(np.uint64) + np.uint64(row_offset), sc[0]


def drop_cut_pad(rows, sc, ids, k, l2=False):
    """drop the listed ids from an ordered answer, cut to k, pad (UINT64_MAX with -inf, +inf for squared Euclidean)"""
    keep = ~np.isin(rows, np.asarray(ids, np.uint64)) & (rows != U64MAX)
    r, s = rows[keep][:k], sc[keep][:k]
    out_r = np.full(k, U64MAX, np.uint64)
    out_s = np.full(k, np.inf if l2 else -np.inf, np.float32)
    out_r[:r.size] = r
    out_s[:r.size] = s
    return out_r, out_s, r.size


def recall_exclude(tab, q, k, lists, l2=False, row_offset=0, mask=None):
    """→ (rows [nq][k], scores [nq][k], counts [nq]) of pg_recall_topk_exclude"""
    q = np.ascontiguousarray(q, np.float32).reshape(-1, tab.shape[1])
    nq = q.shape[0]
    assert len(lists) == nq
    rows = np.empty((nq, k), np.uint64)
    sc = np.empty((nq, k), np.float32)
    cnt = np.empty(nq, np.uint32)
    for i in range(nq):
        pr, ps = plain_top(tab, q[i], k + len(lists[i]), l2, row_offset, mask)
        rows[i], sc[i], cnt[i] = drop_cut_pad(pr, ps, lists[i], k, l2)
    return rows, sc, cnt
