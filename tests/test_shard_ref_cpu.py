"""CPU tests of tests/shard_ref.py, the one statement of the shard-side exchange stages: against the oracle (a merge of per-shard
recalls is the single-table recall), against the CpuEngine stand-in of test_dist_gloo.py (stage by stage, shared inputs), and the
pruned exchange's criterion itself — whenever tail_needed_ref (and dist.tail_needed) flags no shard, merging the heads must give
what merging the whole lists gives, on scores drawn from signed zeros, infinities, NaN and ties."""
import numpy as np
import pytest
import torch

import shard_ref as sr
from oracle import oracle as o
from pairec_amd import dist as pd
from test_dist_gloo import CpuEngine

PAD = sr.PAD


def _i64(rows_u64):
    return torch.from_numpy(np.ascontiguousarray(rows_u64).view(np.int64).copy())


def test_merge_ref_of_per_shard_recalls_is_the_single_table_recall():
    """merge_ref over the per-shard o.recall_topk lists = o.recall_topk of the whole table — uneven shards, one of them shorter than
    k (its list is padded), and k above the table (the merged tail is padded)."""
    n, d, nq = 700, 64, 3
    tab = o.synth_rows(o.SEED_TABLE, 0, n, d)
    q = o.synth_rows(o.SEED_QUERY, 0, nq, d)
    bounds = [0, 40, 300, 301, 700]
    for k in (1, 64, 300, 900):
        lr = np.full((nq, len(bounds) - 1, k), PAD, dtype=np.uint64)
        ls = np.full((nq, len(bounds) - 1, k), -np.inf, dtype=np.float32)
        for g in range(len(bounds) - 1):
            r, s = o.recall_topk(tab[bounds[g]:bounds[g + 1]], q, k, row_offset=bounds[g])
            lr[:, g, :r.shape[1]], ls[:, g, :s.shape[1]] = r, s
        got_r, got_s = sr.merge_ref(lr, ls, k)
        want_r, want_s = o.recall_topk(tab, q, k)
        kk = want_r.shape[1]
        assert kk == min(k, n)
        assert np.array_equal(got_r[:, :kk], want_r) and np.array_equal(sr.bits(got_s[:, :kk]), sr.bits(want_s))
        assert np.all(got_r[:, kk:] == PAD) and np.all(np.isneginf(got_s[:, kk:]))


def test_merge_ref_orders_by_bits_and_canonicalises_nan():
    rows = np.array([[[7, 3, 9, 2, 5, 0xFFFFFFFFFFFFFFFF, 4, 1]]], dtype=np.uint64)
    sc = np.array([[[0.0, -0.0, np.nan, np.inf, 0.0, 99.0, -np.inf, 1e-45]]], dtype=np.float32)
    sc.view(np.uint32)[0, 0, 2] = 0xFFC12345                                # a negative NaN with a payload
    r, s = sr.merge_ref(rows, sc, 9)
    assert r[0].tolist() == [2, 1, 5, 7, 3, 4, 9, int(PAD), int(PAD)]
    assert sr.bits(s)[0].tolist() == [0x7F800000, 1, 0, 0, 0x80000000, 0xFF800000, 0x7FC00000, 0xFF800000, 0xFF800000]


def _stage_inputs(seed=3, nq=4, k=37, off=1000, nrows=500):
    rng = np.random.default_rng(seed)
    rows = rng.choice(np.arange(off - 300, off + nrows + 300), size=(nq, k), replace=False).astype(np.uint64)
    rows[0, :5] = [off - 1, off, off + nrows - 1, off + nrows, 0]
    return rng, rows


def test_refs_equal_the_cpu_stand_in_stage_by_stage():
    """Every ref against the CpuEngine method that stands for the same device call in test_dist_gloo.py, on shared inputs (the
    stand-in takes no padding in merge inputs' outputs and int64 rows; both are converted here, nothing else)."""
    off, nrows, dim = 1000, 500, 64
    rng, rows = _stage_inputs(off=off, nrows=nrows)
    nq, k = rows.shape
    tab = rng.standard_normal((nrows, dim)).astype(np.float32)
    eng = CpuEngine(tab, off, None)
    # merge: G lists of `per` entries, list-major as all-gathered; padding inside the lists, enough real entries for k
    G, per = 3, 20
    g_rows = rng.permutation(5000)[:G * nq * per].astype(np.uint64).reshape(G, nq, per)
    g_sc = rng.choice(np.array([0.0, -0.0, 1.0, 2.5, -1.0, np.inf, -np.inf], dtype=np.float32), size=(G, nq, per))
    g_rows[1, :, 7] = PAD
    g_rows[2, 1, :] = PAD
    er, es = eng.merge(_i64(g_rows), torch.from_numpy(g_sc), k)
    rr, rs = sr.merge_ref(g_rows.transpose(1, 0, 2), g_sc.transpose(1, 0, 2), k)
    assert np.array_equal(er.numpy().view(np.uint64), rr) and np.array_equal(sr.bits(es.numpy()), sr.bits(rs))
    # owned_compact
    el, esl, eo = eng.owned_compact(_i64(rows), nq, k)
    local, slot, offs = sr.owned_compact_ref(rows, off, nrows)
    total = int(offs[-1])
    assert 0 < total < nq * k and np.array_equal(eo.numpy().astype(np.uint32), offs)
    assert np.array_equal(el.numpy()[:total].astype(np.uint32), local) and np.array_equal(esl.numpy()[:total].astype(np.uint32), slot)
    # scatter
    vals = rng.standard_normal(nq * k).astype(np.float32)
    vals[0] = -0.0
    es_ = eng.scatter(torch.from_numpy(vals), esl, eo, nq, k)
    assert np.array_equal(sr.bits(es_.numpy()), sr.bits(sr.scatter_ref(vals, slot, total, nq * k, np.zeros(nq * k, np.float32))))
    # dpp_candidates
    fused = rng.standard_normal((nq, k))
    order = np.stack([rng.permutation(k) for _ in range(nq)]).astype(np.int32)
    ecr, ecl = eng.dpp_candidates(torch.from_numpy(order), _i64(rows), torch.from_numpy(fused), nq, k, 11)
    c_rows, c_rel = sr.sorted_head_ref(order, rows, fused, 11)
    assert np.array_equal(ecr.numpy().view(np.uint64), c_rows) and np.array_equal(sr.bits(ecl.numpy()), sr.bits(c_rel))
    # gather_owned
    ee = eng.gather_owned(_i64(c_rows), nq * 11)
    assert np.array_equal(sr.bits(ee.numpy()), sr.bits(sr.gather_owned_ref(tab, off, c_rows, np.zeros((nq * 11, dim), np.float32))))
    # rows_to_local agrees with owned_compact on who owns what
    loc, own = sr.rows_to_local_ref(rows, off, nrows)
    assert np.array_equal(np.flatnonzero(own).astype(np.uint32), slot) and np.array_equal(loc[own == 1], local)
    assert np.all(loc[own == 0] == 0)


def test_exchange_width_equals_the_group_steps_formula():
    """dist.exchange_width = exchange_width_ref = ceil(k/G + 6 sqrt(k/G) + 8) of step_enqueue clipped to k, k 1…16384 x G 1…8"""
    for G in range(1, 9):
        for k in range(1, 16385):
            assert pd.exchange_width(k, G) == sr.exchange_width_ref(k, G), (k, G)
    assert sr.exchange_width_ref(5000, 8) == 783 and sr.exchange_width_ref(1, 4) == 1 and sr.exchange_width_ref(400, 4) == 168


# ---- the criterion ----------------------------------------------------------------------------------------------------------
VALUES = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 1.0, -1.0, 2.0, 1e-45], dtype=np.float32)
N_CASES = 600


def _sorted_list(rng, rows, k):
    """a shard's list as its recall leaves it: its best k entries by (ordered bits descending, row ascending), padded to k"""
    sc = rng.choice(VALUES, size=rows.shape[0])
    key = [o.topk_key(float(s), int(r)) for s, r in zip(sc, rows)]
    idx = sorted(range(rows.shape[0]), key=lambda i: -key[i])[:k]
    out_r = np.full(k, PAD, dtype=np.uint64)
    out_s = np.full(k, -np.inf, dtype=np.float32)
    out_r[:len(idx)], out_s[:len(idx)] = rows[idx], sc[idx]
    return out_r, out_s


def _cases():
    """(G, k, m, rows [G][1][k], scores [G][1][k]): G 2…4 shards, k <= 12, m < k; a shard holds 0 … 2k rows, so some lists end before
    their m-th entry, some before their k-th, some are full; row ids are spread over the shards at random (distinct)."""
    rng = np.random.default_rng(20260)
    for _ in range(N_CASES):
        G = int(rng.integers(2, 5))
        k = int(rng.integers(2, 13))
        m = int(rng.integers(max(1, k // 2), k))
        ids = rng.permutation(200)
        rows = np.empty((G, 1, k), dtype=np.uint64)
        sc = np.empty((G, 1, k), dtype=np.float32)
        p = 0
        for g in range(G):
            n = int(rng.choice([0, int(rng.integers(0, m + 1)), int(rng.integers(m, k + 1)), 2 * k]))
            rows[g, 0], sc[g, 0] = _sorted_list(rng, ids[p:p + n].astype(np.uint64), k)
            p += n
        yield G, k, m, rows, sc


def _qm(a):
    return np.ascontiguousarray(np.asarray(a).transpose(1, 0, 2))           # list-major [G][nq][*] → [nq][G][*]


def _check_criterion(flags_of):
    quiet = 0
    for G, k, m, rows, sc in _cases():
        h_r, h_s = sr.merge_ref(_qm(rows[:, :, :m]), _qm(sc[:, :, :m]), k)
        need = flags_of(rows[:, :, :m], sc[:, :, :m], h_r, h_s, k)
        assert need.shape == (G,)
        if not need.any():
            quiet += 1
            f_r, f_s = sr.merge_ref(_qm(rows), _qm(sc), k)
            assert np.array_equal(h_r, f_r) and sr.same_bits(h_s, f_s), (G, k, m, rows.tolist(), sr.bits(sc).tolist())
    return quiet


def test_no_flag_means_the_heads_merge_to_the_whole_answer():
    """tail_needed_ref flags no shard → merge_ref(heads) == merge_ref(whole lists).  Not vacuous: between a quarter and three
    quarters of the generated cases come out "not needed"."""
    quiet = _check_criterion(sr.tail_needed_ref)
    print("criterion: %d of %d cases not needed (%.1f %%)" % (quiet, N_CASES, 100.0 * quiet / N_CASES))
    assert N_CASES // 4 <= quiet <= 3 * N_CASES // 4, quiet


def _dist_flags(g_rows, g_sc, m_rows, m_sc, k):
    return pd.tail_needed(torch, _i64(g_rows), torch.from_numpy(np.ascontiguousarray(g_sc)), _i64(m_rows),
                          torch.from_numpy(np.ascontiguousarray(m_sc)), k).numpy()


def test_dist_tail_needed_is_never_less_conservative_than_the_ref():
    """dist.tail_needed on the same cases: it may flag more than tail_needed_ref and never less, and when it flags nothing the heads
    merge to the whole answer."""
    def both(g_rows, g_sc, m_rows, m_sc, k):
        ref, got = sr.tail_needed_ref(g_rows, g_sc, m_rows, m_sc, k), _dist_flags(g_rows, g_sc, m_rows, m_sc, k)
        assert np.all(got[ref]), (ref, got, g_rows.tolist(), sr.bits(g_sc).tolist())
        return got
    quiet = _check_criterion(both)
    assert quiet >= N_CASES // 4


def test_signed_zero_tail_is_needed():
    """k = 2, one entry sent per shard: A holds (5, +0.0), (6, +0.0), B holds (0, -0.0), (1, -1.0).  The heads merge to rows [5, 0],
    the whole lists to [5, 6] (+0.0 ranks before -0.0 by ordered bits): shard A's last sent entry lies strictly inside the merged
    top-2 and must be flagged.  A float compare sees a tie on the score that row 0 wins, and flags nothing."""
    rows = np.array([[[5, 6]], [[0, 1]]], dtype=np.uint64)
    sc = np.array([[[0.0, 0.0]], [[-0.0, -1.0]]], dtype=np.float32)
    h_r, h_s = sr.merge_ref(_qm(rows[:, :, :1]), _qm(sc[:, :, :1]), 2)
    f_r, _ = sr.merge_ref(_qm(rows), _qm(sc), 2)
    assert h_r.tolist() == [[5, 0]] and f_r.tolist() == [[5, 6]]
    assert sr.tail_needed_ref(rows[:, :, :1], sc[:, :, :1], h_r, h_s, 2).tolist() == [True, False]
    assert _dist_flags(rows[:, :, :1], sc[:, :, :1], h_r, h_s, 2).tolist() == [True, False]


@pytest.mark.parametrize("last,kth,want", [
    ((3, np.nan), (9, np.nan), True),            # NaN against NaN: the lower row is inside
    ((9, np.nan), (3, np.nan), False),
    ((3, np.nan), (9, -np.inf), False),          # NaN ranks below -inf
    ((9, -np.inf), (3, np.nan), True),
    ((3, 1.0), (3, 1.0), False),                 # the last sent entry IS the k-th: nothing unsent can precede it
])
def test_tail_needed_orders_nan_last_and_is_strict(last, kth, want):
    g_rows = np.array([[[100, last[0]]]], dtype=np.uint64)
    g_sc = np.array([[[5.0, last[1]]]], dtype=np.float32)
    m_rows = np.array([[100, kth[0]]], dtype=np.uint64)
    m_sc = np.array([[5.0, kth[1]]], dtype=np.float32)
    assert sr.tail_needed_ref(g_rows, g_sc, m_rows, m_sc, 2).tolist() == [want]
    assert _dist_flags(g_rows, g_sc, m_rows, m_sc, 2).tolist() == [want]


def test_tail_needed_padding_rules():
    """a padded last-sent entry: the list ended, never needed; a merged list short of k: every list that did not end is suspect"""
    g_rows = np.array([[[4, 0xFFFFFFFFFFFFFFFF]], [[7, 8]]], dtype=np.uint64)
    g_sc = np.array([[[9.0, -np.inf]], [[1.0, 0.5]]], dtype=np.float32)
    m_r, m_s = sr.merge_ref(_qm(g_rows), _qm(g_sc), 4)
    assert m_r.tolist() == [[4, 7, 8, int(PAD)]]
    assert sr.tail_needed_ref(g_rows, g_sc, m_r, m_s, 4).tolist() == [False, True]
    assert _dist_flags(g_rows, g_sc, m_r, m_s, 4).tolist() == [False, True]
