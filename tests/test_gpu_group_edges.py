"""GPU tests of the shard group's step (pg_group_recommend, csrc/group.hip) at the edges its glue kernels — pack_heads,
tail_needed, scatter_to_tails, take_requests, gather_to_tails — and step_enqueue's branches have: tables so small that k reaches
and passes a shard's rows, k = 1 (the exchange width clips to k), fewer requests than shards (a tail shard with no request), 256
requests over 3 shards, uneven row ranges.  Logical shards on device 0, F32 model, against the single-table oracle_pipeline of
test_gpu_group.py with that file's tolerances: page ids and order exact, recall scores bit-exact, model scores within 2e-7, fused
scores within 1e-6."""
import numpy as np
import pytest

import pairec_amd as pa
import shard_ref as sr
from oracle import oracle as o
from test_gpu_group import EXPR, bits, oracle_pipeline

pytestmark = pytest.mark.gpu

D = 128


class Group:
    """a shard group over G logical shards of device 0 with the synthetic table of n rows, the F32 DNN3 model, and the same rows on
    the host"""

    def __init__(self, G, n):
        self.G, self.n = G, n
        self.tab = o.synth_rows(o.SEED_TABLE, 0, n, D)
        self.w = o.Dnn3Weights()
        self.g = pa.ShardGroup([0] * G)
        self.g.table_create(n, D)
        self.g.table_fill_synthetic(o.SEED_TABLE)
        w = self.w
        self.g.model_load(pa.MODEL_DNN3, pa.PREC_F32, pa.pack_dnn3(w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, 128))
        self.ex = pa.Expr(EXPR)
        self._want = {}

    def want(self, user0, nq, k, top_n, dpp_c):
        """the oracle's pages of a step (computed once per shape, shared by the tests that run it)"""
        key = (user0, nq, k, top_n, dpp_c)
        if key not in self._want:
            q = o.synth_rows(o.SEED_QUERY, user0, nq, D)
            self._want[key] = (q, oracle_pipeline(self.tab, self.w, pa.PREC_F32, q, k, top_n, dpp_c, 1.0, 10))
        return self._want[key]

    def check(self, got, want, top_n, what):
        rows, rec, rnk, fus, cnt = got
        for r, (w_rows, w_rec, w_rk, w_fu) in enumerate(want):
            n = w_rows.shape[0]                                     # (DPP may stop before top_n picks; the oracle says when)
            assert cnt[r] == n, "%s request %d: %d page entries, the oracle has %d" % (what, r, cnt[r], n)
            assert np.array_equal(rows[r][:n], w_rows), "%s request %d: page ids / order differ" % (what, r)
            assert np.array_equal(bits(rec[r][:n]), bits(w_rec)), "%s request %d: recall scores" % (what, r)
            assert np.max(np.abs(rnk[r][:n].astype(np.float64) - w_rk)) <= 2e-7, "%s request %d: model scores" % (what, r)
            assert np.max(np.abs(fus[r][:n] - w_fu)) <= 1e-6, "%s request %d: fused scores" % (what, r)

    def step(self, user0, nq, k, top_n, dpp_c):
        q, want = self.want(user0, nq, k, top_n, dpp_c)
        got = self.g.recommend(self.ex, "gpu_dnn", q, k, top_n, dpp_candidates=dpp_c, dpp_alpha=1.0, dpp_window=10)
        self.check(got, want, top_n, "nq=%d k=%d top_n=%d dpp=%d" % (nq, k, top_n, dpp_c))

    def destroy(self):
        self.g.destroy()


@pytest.fixture(scope="module")
def g1000():
    g = Group(4, 1000)
    yield g
    g.destroy()


@pytest.fixture(scope="module")
def g1003():
    g = Group(4, 1003)
    yield g
    g.destroy()


def _shapes():
    for k in (1, 4, 100, 400, 1000):
        for top_n in ((1, k) if k <= 100 else (40,)):
            for dpp in ("none", "top_n", "above_k"):
                yield k, top_n, dpp


@pytest.mark.parametrize("k,top_n,dpp", sorted(set(_shapes())))
def test_small_table_k_from_one_to_every_row(g1000, k, top_n, dpp):
    """1 000 rows over 4 shards of 250.  k = 1: step_enqueue's `w < k` fails, m clips to k, no pack_heads / tail_needed (checked:
    entries_per_request_and_shard).  k = 4: the same with a list of more than one entry.  k = 100: heads of m = 63 < k.  k = 400 >
    a shard's 250 rows: every shard's list is padded behind its rows, merge_keys_kernel drops the padding, owned_fill_kernel and
    scatter_to_tails see 400-entry lists.  k = 1000 = the table: m = 353 > 250, every list ends before its m-th entry
    (tail_needed_kernel's `r_m == ~0` return) and every merged slot is filled from padded lists.  dpp_candidates 0 (no
    gather_to_tails), = top_n, and k + 50 (C clips to k: sorted_head / gather_to_tails at C = k)."""
    dpp_c = {"none": 0, "top_n": top_n, "above_k": k + 50}[dpp]
    g1000.step(60 + k, 5, k, top_n, dpp_c)
    st = g1000.g.exchange_stats()
    if st["entries_per_request_and_shard"] != k:                    # (k after a repeated step; the width otherwise)
        assert st["entries_per_request_and_shard"] == sr.exchange_width_ref(k, 4)
    if k in (1, 4):
        assert sr.exchange_width_ref(k, 4) == k == st["entries_per_request_and_shard"]


@pytest.mark.parametrize("k,top_n,dpp_c", [(100, 40, 0), (400, 40, 60), (1003, 40, 0), (1003, 40, 1100)])
def test_uneven_row_ranges(g1003, k, top_n, dpp_c):
    """1 003 rows over 4 shards: 251 / 251 / 251 / 250 (shard_range's remainder rule, the row_offset of every shard off the multiples
    of 250) — owned_count / owned_fill's `r - off < nrows` at ranges of two lengths, gather_to_tails' too; k = 1003 takes every row."""
    g1003.step(17, 5, k, top_n, dpp_c)


@pytest.mark.parametrize("dpp_c", [0, 30])
@pytest.mark.parametrize("nq", [1, 2, 3, 5])
def test_fewer_requests_than_shards(g1000, nq, dpp_c):
    """G = 4, nq 1 / 2 / 3: tail shards nq … 3 have nqs = 0 — step_enqueue skips their memset, take_requests, fusion and page copy
    but still records ev_ready / ev_sel / ev_done for the peers; gather_to_tails' `s < nq ? … : 0` leaves their buffers alone.  nq = 5:
    shard 0 finishes two requests, the others one (take_requests' q = s + i G, scatter_to_tails' q % G, q / G)."""
    g1000.step(200 + nq, nq, 100, 10, dpp_c)


@pytest.mark.parametrize("dpp_c", [0, 20])
def test_256_requests_over_three_shards(dpp_c):
    """G = 3, nq = 256 on 3 000 rows at k = 64: nqs = 86 / 85 / 85 — the request → tail shard maps of scatter_to_tails, take_requests
    and gather_to_tails with a remainder, owned_scan_kernel with all 256 threads live."""
    g = Group(3, 3000)
    try:
        g.step(0, 256, 64, 10, dpp_c)
    finally:
        g.destroy()


def test_no_second_round_when_every_list_ends_before_its_mth_entry(g1000, g1003):
    """exchange_stats: at k = 1000 the first exchange sends m = 353 entries per request and shard, more than any shard's 250 (251)
    rows — the last sent entry of every list is padding, tail_needed_kernel returns at `r_m == ~0` for every (shard, request), so the
    step cannot ask for the whole lists: round2_steps stays where it was and the width that was sent is reported.  The same at
    k = 1 and 4, where m = k and nothing is pruned at all."""
    for g, ks in ((g1000, (1000, 1, 4)), (g1003, (1000,))):
        for k in ks:
            before = g.g.exchange_stats()
            g.step(60 + k if g is g1000 else 17, 5, k, 1 if k == 1 else min(k, 40), 0)
            st = g.g.exchange_stats()
            assert st["round2_steps"] == before["round2_steps"] and st["steps"] == before["steps"] + 1, (k, before, st)
            assert st["entries_per_request_and_shard"] == sr.exchange_width_ref(k, 4) == min(k, 353)
            assert st["exchange1_bytes_per_shard"] == 5 * min(k, 353) * 12


def test_two_steps_in_flight_alternating_small_shapes(g1000):
    """pg_group_recommend_begin / _end with two steps outstanding on the two lanes, alternating among the small shapes above (k = 1,
    nq < G, k above a shard's rows, DPP clipped to k): each lane's buffers and events are reused by a step of another shape while
    the other lane's step is still outstanding; collected out of order."""
    shapes = [(301, 1, 1, 1, 0), (302, 5, 400, 40, 60), (303, 3, 4, 4, 4), (304, 2, 100, 10, 150), (305, 5, 1000, 40, 0)]
    g1000.step(300, 5, 1000, 40, 1000)                              # (buffers grow to the largest shape while the group is idle)
    for i in range(len(shapes)):
        a, b = shapes[i], shapes[(i + 1) % len(shapes)]
        tickets = []
        for user0, nq, k, top_n, dpp_c in (a, b):
            q, _ = g1000.want(user0, nq, k, top_n, dpp_c)
            tickets.append(g1000.g.recommend_begin(g1000.ex, "gpu_dnn", q, k, top_n, dpp_candidates=dpp_c))
        for tk, (user0, nq, k, top_n, dpp_c) in ((tickets[1], b), (tickets[0], a)):
            got = g1000.g.recommend_end(tk)
            g1000.check(got, g1000.want(user0, nq, k, top_n, dpp_c)[1], top_n, "in flight: nq=%d k=%d dpp=%d" % (nq, k, dpp_c))


def test_second_round_over_padded_lists():
    """The repeated exchange on lists that carry padding: 1 000 rows over 4 shards, k = 400 > a shard's 250 rows, m = 168.  Every
    row is the same vector, so all scores tie and the lowest row ids win: the answer is shard 0 whole and 150 rows of shard 1.
    Shard 0's 168th entry (row 167) lies inside the merged top-400, so tail_needed_kernel flags the step — once, counted — and the
    whole 400-entry lists travel, 150 of them padding on every shard; merge_keys_kernel drops it and the page is the single-table
    oracle's."""
    g = Group(4, 1000)
    try:
        g.tab[:] = g.tab[0]
        g.g.table_upload(g.tab, 0)
        before = g.g.exchange_stats()
        g.step(40, 5, 400, 40, 0)
        st = g.g.exchange_stats()
        assert st["round2_steps"] == before["round2_steps"] + 1 and st["steps"] == before["steps"] + 1, (before, st)
        assert st["entries_per_request_and_shard"] == 400 and sr.exchange_width_ref(400, 4) == 168
    finally:
        g.destroy()
