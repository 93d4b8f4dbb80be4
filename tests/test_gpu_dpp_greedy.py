"""GPU tests of the three DPP greedy kernels (csrc/dpp.hip) at their edges.  dpp_run_locked picks the kernel by shape
(window 0 means 10 first):

    wave8    dpp_greedy_wave_kernel<8, 16>    n <= 512 and window <= 16      (one wave per request, eight items per lane)
    wave16   dpp_greedy_wave_kernel<16, 10>   otherwise n <= 1024 and window <= 10
    block    dpp_greedy_kernel                everything else up to 8192     (one workgroup of 1024 threads)

and pg_stats' dpp_wave8_calls / dpp_wave16_calls / dpp_block_calls say which one ran: every case asserts that exactly
the expected counter moved by one, so a change of the rule cannot move the cases onto one kernel unnoticed.

The kernels perform the arithmetic, its order and the tie rules of oracle/oracle.c:dpp_once (dpp_sort.go:493-551), so
every comparison is exact: np.array_equal on the pick sequence, equality on the count.  Where exp() is in play the
cases use alpha = 0 (r = 1 exactly on host and device) whenever they pick by rounding noise; the well-conditioned
pages use alpha = 1 as tests/test_gpu_parity.py::test_dpp_matches_oracle does.

  a, c  exact rank-deficient pages and ties (tests/dpp_ref.py): device == hand model == oracle
  b     duplicate table rows: every window ends in the `dj < epsilon` break and the fill by index
  d     shape edges on well-conditioned data: n around the lanes and the dispatch boundaries, windows 0 … 17, topn > n
  e     pg_dpp_batch_dev, R = 1, 8, 9, 17, requests that break mixed with requests that do not"""
import numpy as np
import pytest

import pairec_amd as pa
from pairec_amd import _lib
from oracle import oracle as o

import dpp_ref as ref
from dpp_ref import BLOCK, WAVE8, WAVE16

pytestmark = pytest.mark.gpu

KINDS = (WAVE8, WAVE16, BLOCK)


def counters(ctx):
    s = ctx.stats()
    return {k: getattr(s, k) for k in KINDS}


def moved(before, after):
    return {k: after[k] - before[k] for k in before}


def only(kind, by=1):
    return {k: (by if k == kind else 0) for k in KINDS}


def counted(ctx, kind, call):
    """call() with the assertion that it was served by one launch sequence of `kind`"""
    before = counters(ctx)
    got = call()
    assert moved(before, counters(ctx)) == only(kind)
    return got


def oracle_picks(F, rel, alpha, topn, window):
    with np.errstate(all="ignore"):
        return o.dpp_with_window(o.dpp_kernel_matrix_f(F, rel, alpha), topn, window or 10)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if len(got) != len(want) or not np.array_equal(got, want):
        m = min(len(got), len(want))
        diff = np.nonzero(got[:m] != want[:m])[0]
        first = int(diff[0]) if len(diff) else m
        pytest.fail("%s: counts %d / %d, picks differ first at %d: device %s, reference %s"
                    % (what, len(got), len(want), first, got[first:first + 6].tolist(), want[first:first + 6].tolist()))


# ---- a, c: exact pages -------------------------------------------------------------------------------------------
def run_hook_page(ctx, hook, kinds, exps, topn, window, kind):
    n = hook.shape[0]
    hand = ref.greedy_by_hand(kinds, exps, topn, window)
    want = oracle_picks(o.dpp_features(None, hook, False, False), np.zeros(n), 0.0, topn, window)
    assert hand == want.tolist()
    got, _ = counted(ctx, kind, lambda: pa.dpp_ex(ctx, None, None, np.zeros(n), 0.0, topn, window, False, False, 0, hook))
    same(got, hand, "hand model")
    return hand


@pytest.mark.parametrize("case", ref.HOOK_CASES, ids=lambda c: "%dx%d-top%d-w%d" % (c[0], c[1], c[2], c[3]))
def test_exact_rank_deficient_pages(ctx, case):
    """Hook-only pages on which nothing rounds: fewer live columns than the window, so windows leave the loop through
    `dj < epsilon` and end in the fill (first, middle and remainder windows); topn > n over several windows, later
    windows over NaN alone (item 0 appended again and again, and counted); n = 1, 5, 63, 65."""
    hook, kinds, exps, topn, window = ref.hook_case(case)
    n = hook.shape[0]
    trace = []
    hand = ref.greedy_by_hand(kinds, exps, topn, window, trace)
    what = case[6]
    if what in ("fill", "every window"):
        assert ref.filled_windows(hand, n, trace), "precondition: no window of this case breaks and fills"
    if what == "every window":
        assert ref.filled_windows(hand, n, trace) == list(range(len(trace)))
    if what == "exhausted":
        assert len(hand) < topn or len(set(hand)) < len(hand), "precondition: nothing runs out"
    assert run_hook_page(ctx, hook, kinds, exps, topn, window, case[5]) == hand


@pytest.mark.parametrize("case", ref.TIE_CASES, ids=lambda c: "%d-%s-w%d" % (c[0], "_".join(map(str, c[2])) or "all", c[4]))
def test_first_maximum_ties_across_lanes_and_slots(ctx, case):
    """Equal maxima in one lane of several element slots (6, 70, 454 / 518), in different lanes, in the last valid lane
    alone, and everywhere at once: the first index wins."""
    hook, kinds, exps, topn, window = ref.tie_case(case)
    hand = run_hook_page(ctx, hook, kinds, exps, topn, window, case[6])
    top = case[2]
    assert hand[:len(top)] == sorted(top)


# ---- b: duplicate rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hook_dim", [0, 5], ids=["table", "hook_table"])
@pytest.mark.parametrize("case", ref.DUP_CASES, ids=lambda c: "%dof%d-d%d-w%d" % (c[0], c[1], c[2], c[4]))
def test_duplicate_rows_fill_every_window(ctx, case, hook_dim):
    """Candidates drawn with repetition from m < window table rows, normalised, alpha = 0: copies of a picked row are
    left with the same rounding noise on both sides and tie exactly.  dpp_prepare_table_kernel<128> / <64>, and with hook
    rows in front of the table's the generic dpp_prepare_kernel."""
    n, m, d, topn, window, kind = case
    tab, cand, rel, hook = ref.dup_case(case, hook_dim=hook_dim)
    want = oracle_picks(o.dpp_features(tab[cand], hook, True, True), rel, 0.0, topn, window)
    ref.check_duplicates_fill_every_window(want.tolist(), cand, topn, window)
    t = pa.Table(ctx, tab.shape[0], d)
    t.upload(tab)
    try:
        if hook is None:
            got = counted(ctx, kind, lambda: pa.dpp(ctx, t, cand, rel, 0.0, topn, window, True))
        else:
            got, _ = counted(ctx, kind, lambda: pa.dpp_ex(ctx, t, cand, rel, 0.0, topn, window, True, True, 0, hook))
    finally:
        t.destroy()
    same(got, want, "oracle")


# ---- d: shape edges ----------------------------------------------------------------------------------------------
class Clustered:
    """The table of test_dpp_matches_oracle (12 centres + 0.2 x noise, 4000 x 128) and, per n, one candidate set with its
    feature rows: computed once, shared by every case of that n"""
    def __init__(self):
        rng = np.random.default_rng(8)
        centers = rng.standard_normal((12, 128)).astype(np.float32)
        self.tab = (centers[rng.integers(0, 12, 4000)] + 0.2 * rng.standard_normal((4000, 128))).astype(np.float32)
        self.sets = {}

    def of(self, n):
        if n not in self.sets:
            rng = np.random.default_rng(100 + n)
            cand = rng.choice(4000, n, replace=False).astype(np.uint32)
            rel = np.sort(rng.random(n))[::-1].copy()
            self.sets[n] = (cand, rel, o.dpp_features(self.tab[cand], None, True, True), {})
        return self.sets[n]

    def want(self, n, alpha, topn, window):
        cand, rel, F, Ls = self.of(n)
        if alpha not in Ls:
            Ls[alpha] = o.dpp_kernel_matrix_f(F, rel, alpha)
        with np.errstate(all="ignore"):
            return o.dpp_with_window(Ls[alpha], topn, window or 10)


@pytest.fixture(scope="module")
def clustered(ctx):
    c = Clustered()
    c.table = pa.Table(ctx, 4000, 128)
    c.table.upload(c.tab)
    yield c
    c.table.destroy()


@pytest.mark.parametrize("n,window,topn", ref.EDGE_CASES, ids=lambda v: str(v))
def test_shape_edges_match_oracle(ctx, clustered, n, window, topn):
    """n = 1, 2, lanes without an item (63 / 64 / 65), both sides of 512 / 513 and 1024 / 1025; windows 0 (-> 10), 1,
    11 … 16 on the wave kernel's unrolled picks (16 x 512 doubles = 64 KB of LDS), 17 and 11 beyond 512 on the
    workgroup kernel; window > n, topn < window, topn = n and n + 7 (the last windows find nothing left)."""
    cand, rel, _, _ = clustered.of(n)
    want = clustered.want(n, 1.0, topn, window)
    w = window or 10
    assert len(want) == (min(topn, n) if topn <= w else (topn // w) * min(w, n) + min(topn % w, n))
    if (n, window) in ref.BOUNDARIES:
        assert ref.kernel_of(n, window) == ref.BOUNDARIES[(n, window)]
    got = counted(ctx, ref.kernel_of(n, window), lambda: pa.dpp(ctx, clustered.table, cand, rel, 1.0, topn, window, True))
    same(got, want, "oracle")
    if window == 0:
        assert np.array_equal(want, clustered.want(n, 1.0, topn, 10))


@pytest.mark.parametrize("n,window,kind", [(65, 10, WAVE8), (520, 10, WAVE16), (65, 17, BLOCK)])
def test_an_item_that_is_never_picked(ctx, clustered, n, window, kind):
    """A NaN relevance score with alpha = 0 (r = exp(0 x NaN) = NaN: the item's row and column of L are NaN) and, apart,
    an all-zero table row under normalize_emb (its feature row is NaN): floats.MaxIdx never returns the item while
    another is left, and topn = n + 7 runs the others out."""
    cand, rel, _, _ = clustered.of(n)
    topn = n + 7
    nan_rel = rel.copy()
    nan_rel[5] = np.nan
    tab = clustered.tab.copy()
    zero_row = 3999 if 3999 not in cand else 3998
    assert zero_row not in cand
    tab[zero_row] = 0.0
    zcand = cand.copy()
    zcand[7] = zero_row
    t = pa.Table(ctx, 4000, 128)
    t.upload(tab)
    try:
        for c, r, never in ((cand, nan_rel, 5), (zcand, rel, 7)):
            with np.errstate(all="ignore"):
                F = o.dpp_features(tab[c], None, True, True)
            want = oracle_picks(F, r, 0.0, topn, window)
            assert np.isnan(F[7]).any() == (never == 7)
            assert never not in want[:n - 1].tolist() and len(want) == topn
            got = counted(ctx, kind, lambda: pa.dpp(ctx, t, c, r, 0.0, topn, window, True))
            same(got, want, "oracle")
    finally:
        t.destroy()


# ---- e: batches --------------------------------------------------------------------------------------------------
BATCH_R = (1, 8, 9, 17)
#   n, window, topn, kernel: the remainder window of a breaking request has five (ten) picks for its three rows
BATCH_SHAPES = [(300, 10, 35, WAVE8), (800, 10, 35, WAVE16), (600, 20, 50, BLOCK)]


def batch_inputs(tab, n, mixed):
    """17 requests over the clustered table: their own candidates and relevance; in a mixed batch the odd ones draw
    their candidates with repetition from three rows"""
    rng = np.random.default_rng(7 * n + int(mixed))
    cand = np.stack([rng.choice(tab.shape[0], n, replace=False) for _ in range(max(BATCH_R))]).astype(np.uint32)
    if mixed:
        for q in range(1, max(BATCH_R), 2):
            rows = cand[q, :3].copy()
            cand[q] = rows[rng.integers(0, 3, n)]
            cand[q, :3] = rows
    rel = np.sort(rng.random((max(BATCH_R), n)), axis=1)[:, ::-1].copy()
    return cand, rel


@pytest.mark.parametrize("mixed", [True, False], ids=["mixed_alpha0", "plain_alpha1"])
@pytest.mark.parametrize("n,window,topn,kind", BATCH_SHAPES, ids=lambda v: str(v))
def test_batches_match_oracle_request_by_request(ctx, clustered, n, window, topn, kind, mixed):
    """pg_dpp_batch_dev (blockIdx.x = request, every slice offset by it) with R = 1, 8, 9, 17 — full rounds of eight
    requests and a partial one in the kernel matrix's placement: out_count[q] and out[q, :count] equal the oracle's for
    request q's data and pg_dpp's alone on it; one count per batch.  Mixed: odd requests break and fill in every window
    (alpha = 0), even ones never do."""
    alpha = 0.0 if mixed else 1.0
    cand, rel = batch_inputs(clustered.tab, n, mixed)
    R_max = max(BATCH_R)
    want = []
    for q in range(R_max):
        w = oracle_picks(o.dpp_features(clustered.tab[cand[q]], None, True, True), rel[q], alpha, topn, window)
        if mixed and q % 2:
            ref.check_duplicates_fill_every_window(w.tolist(), cand[q], topn, window)
        else:
            assert len(set(w.tolist())) == topn and not np.array_equal(w, np.arange(topn))
        want.append(w)
    for q in range(R_max):
        solo = counted(ctx, kind, lambda: pa.dpp(ctx, clustered.table, cand[q], rel[q], alpha, topn, window, True))
        same(solo, want[q], "request %d alone" % q)
    emb = clustered.tab[cand]                                     # [17][n][128]
    d_out, d_cnt = ctx.malloc(R_max * topn * 4), ctx.malloc(R_max * 4)
    try:
        for R in BATCH_R:
            d_e, d_r = ctx.to_device(emb[:R]), ctx.to_device(rel[:R])
            ctx.h2d(d_out, np.full(R_max * topn, 0xFFFFFFFF, np.uint32))
            ctx.h2d(d_cnt, np.full(R_max, 0xFFFFFFFF, np.uint32))
            try:
                counted(ctx, kind, lambda: _lib.check(ctx.L.pg_dpp_batch_dev(ctx.h, d_e, d_r, R, n, 128, alpha, topn, window, 1, d_out, d_cnt)))
                out, cnt = np.zeros((R, topn), np.uint32), np.zeros(R, np.uint32)
                ctx.d2h(out, d_out)
                ctx.d2h(cnt, d_cnt)
            finally:
                ctx.free(d_e)
                ctx.free(d_r)
            for q in range(R):
                assert cnt[q] == len(want[q]), (R, q)
                same(out[q, :cnt[q]], want[q], "batch of %d, request %d" % (R, q))
    finally:
        ctx.free(d_out)
        ctx.free(d_cnt)
