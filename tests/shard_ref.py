"""The shard-side exchange calls on the CPU: one plain numpy function per device call of the sharded path —
pg_topk_merge[_lists]_dev, pg_owned_compact_dev, pg_scatter_f32_dev, pg_dpp_candidates_dev, pg_gather_owned_rows_dev,
pg_rows_to_local_dev — and per piece of arithmetic the group step shares with pairec_amd/dist.py (the exchange width, the
"does a shard's unsent tail matter" criterion).  Rows are uint64 with UINT64_MAX as padding; scores never meet arithmetic, they
travel as bits (a NaN leaves the merge as the canonical quiet NaN, the only change of bits anywhere)."""
import math

import numpy as np

from oracle import oracle as o

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
QNAN_BITS = np.uint32(0x7FC00000)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(got, want):
    """equal bit for bit; NaN by NaN-ness (the payload of a NaN is only specified where a ref says so)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn]))


def ordered_bits(scores) -> np.ndarray:
    """float32 → uint32 whose unsigned order is the recall's score order: IEEE totalOrder (-inf < ... < -0.0 < +0.0 < ... <
    +inf) with every NaN below everything (f32_ordered_bits of recall_shared.hpp / oracle.c, tail_ord of group.hip)."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    b = s.view(np.uint32)
    ob = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(s), np.uint32(0), ob).astype(np.uint32)


def merge_ref(rows, scores, k: int):
    """rows / scores [nq][nlists][per_list] → the global top-k per request, (rows [nq][k] u64, scores [nq][k] f32): padding
    entries dropped wherever they stand, the rest ordered score descending (ordered_bits) and row ascending by o.topk_merge,
    the tail behind the last real entry padded with (UINT64_MAX, -inf).  NaN scores come out as the canonical quiet NaN."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    nq = rows.shape[0]
    out_r = np.full((nq, k), PAD, dtype=np.uint64)
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    for q in range(nq):
        rr, ss = rows[q].reshape(-1), scores[q].reshape(-1)
        keep = rr != PAD
        if not keep.any():
            continue
        r, s = o.topk_merge(rr[keep][None], ss[keep][None], k)
        s = s.copy()
        s.view(np.uint32)[np.isnan(s)] = QNAN_BITS
        out_r[q, :r.shape[0]], out_s[q, :s.shape[0]] = r, s
    return out_r, out_s


def owned(rows, row_offset: int, nrows: int) -> np.ndarray:
    """a global row id belongs to the shard holding [row_offset, row_offset + nrows); padding belongs to nobody"""
    r = np.asarray(rows, dtype=np.uint64)
    return (r != PAD) & (r >= np.uint64(row_offset)) & (r < np.uint64(row_offset + nrows))


def owned_compact_ref(rows, row_offset: int, nrows: int):
    """rows [nq][k] → (local u32 [total], slot u32 [total], offsets u32 [nq + 1]): the owned entries request by request, in list
    order (stable), as shard-local row and position q * k + j in the merged lists; offsets = CSR over the requests"""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    nq, k = rows.shape
    m = owned(rows, row_offset, nrows)
    slot = np.flatnonzero(m.reshape(-1)).astype(np.uint32)                  # row-major = request by request, j ascending
    local = (rows.reshape(-1)[slot] - np.uint64(row_offset)).astype(np.uint32)
    off = np.zeros(nq + 1, dtype=np.uint32)
    off[1:] = np.cumsum(m.sum(axis=1))
    return local, slot, off


def scatter_ref(vals, slot, total: int, cap: int, out):
    """out[slot[i]] = vals[i] for i < min(total, cap), values as bits; the rest of `out` as it was (a copy is returned)"""
    res = np.array(out, dtype=np.float32, copy=True)
    n = min(int(total), int(cap))
    res.view(np.uint32)[np.asarray(slot[:n], dtype=np.int64)] = bits(np.asarray(vals, dtype=np.float32)[:n])
    return res


def sorted_head_ref(order, rows, fused, n_cand: int):
    """the first n_cand entries of every request's sorted list: (rows u64 [nq * n_cand], fused f64 [nq * n_cand]) by bits"""
    order = np.asarray(order).astype(np.int64)
    head = order[:, :n_cand]
    c_rows = np.take_along_axis(np.asarray(rows, dtype=np.uint64), head, axis=1).reshape(-1)
    c_rel = np.take_along_axis(bits(np.asarray(fused, dtype=np.float64)), head, axis=1).reshape(-1)
    return c_rows.copy(), c_rel.copy().view(np.float64)


def gather_owned_ref(tab_shard, row_offset: int, c_rows, out):
    """out[i] = the shard's embedding row of c_rows[i] where the shard owns it; every other destination row untouched"""
    tab_shard = np.asarray(tab_shard, dtype=np.float32)
    res = np.array(out, dtype=np.float32, copy=True)
    r = np.asarray(c_rows, dtype=np.uint64)
    m = owned(r, row_offset, tab_shard.shape[0])
    res[m] = tab_shard[(r[m] - np.uint64(row_offset)).astype(np.int64)]
    return res


def rows_to_local_ref(rows, row_offset: int, nrows: int):
    """(local u32 [n], owned u8 [n]): the shard-local row, or 0 and owned = 0 for a row of another shard or padding"""
    r = np.asarray(rows, dtype=np.uint64).reshape(-1)
    m = owned(r, row_offset, nrows)
    local = np.where(m, r - np.uint64(row_offset), np.uint64(0)).astype(np.uint32)
    return local, m.astype(np.uint8)


def exchange_width_ref(k: int, G: int) -> int:
    """entries per request and shard of the first exchange: ceil(k/G + 6 sqrt(k/G) + 8) in double precision, clipped to k
    (step_enqueue of group.hip; one shard sends everything: the formula exceeds k by itself)"""
    per = float(k) / float(G)
    return min(k, int(math.ceil(per + 6.0 * math.sqrt(per) + 8.0)))


def tail_needed_ref(g_rows, g_scores, m_rows, m_scores, k: int) -> np.ndarray:
    """[G] bool — could an entry shard g did NOT send belong to some request's global top-k?  g_rows / g_scores [G][nq][m] are the
    heads that were exchanged, m_rows / m_scores [nq][k] their merge.  As tail_needed_kernel decides it: a padded last-sent entry
    means the list ended, nothing was left unsent; a merged list short of k makes every full list suspect; otherwise the last-sent
    entry must not rank strictly before the k-th merged one — score by ordered_bits (so +0.0 before -0.0, NaN last), then row
    ascending."""
    g_rows = np.asarray(g_rows, dtype=np.uint64)
    m_rows = np.asarray(m_rows, dtype=np.uint64)
    r_m, a = g_rows[:, :, -1], ordered_bits(np.asarray(g_scores, dtype=np.float32)[:, :, -1])       # [G][nq]
    r_k, b = m_rows[:, k - 1], ordered_bits(np.asarray(m_scores, dtype=np.float32)[:, k - 1])       # [nq]
    short = (m_rows != PAD).sum(axis=1) < k                                                        # [nq]
    inside = (a > b[None]) | ((a == b[None]) & (r_m < r_k[None]))
    return ((r_m != PAD) & (short[None] | inside)).any(axis=1)
