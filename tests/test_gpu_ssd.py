"""GPU tests of the three SSD re-rank kernels (csrc/ssd.hip) against oracle/oracle.c:orc_ssd_window, each at its own
edges.  ssd_run_locked picks the kernel by shape (d1 = embedding dim + ensure_pos_similarity):

    grid     ssd_kernel_grid<D1>   d1 in {64, 65, 128, 129} and window <= 16   (one wave per workgroup, G = ceil(n / 64) <= 128)
    reg      ssd_kernel_reg<D1>    those widths, window > 16, n <= 2048        (one workgroup, state in LDS)
    generic  ssd_kernel            everything else up to 8192 x 320            (blocks of 16 values plus a tail)

and pg_stats' ssd_grid_calls / ssd_reg_calls / ssd_generic_calls say which one ran; every case asserts that exactly
the expected counter moved, so a change of the dispatch rule cannot move the cases onto one kernel unnoticed.

SSD is fp64 with a fixed operation order and no transcendental function: every comparison is exact (pick sequence
with array_equal, quality scores bit for bit).  A table holds dims 64 / 128 / 192 / 256 only; the other widths go in
as the candidates' own embeddings (pg_ssd_emb), which is the same code behind the checks."""
import numpy as np
import pytest

import pairec_amd as pa
from oracle import oracle as o
from test_gpu_scene_coalescer import bits, run_threads

pytestmark = pytest.mark.gpu

UNSUPPORTED = -4
GRID, REG, GENERIC = "ssd_grid_calls", "ssd_reg_calls", "ssd_generic_calls"
GAMMA = 0.25


def counters(ctx):
    s = ctx.stats()
    return {k: getattr(s, k) for k in (GRID, REG, GENERIC)}


def moved(before, after):
    return {k: after[k] - before[k] for k in before}


def only(kind, by=1):
    return {k: (by if k == kind else 0) for k in (GRID, REG, GENERIC)}


def make_inputs(dim, n, prop, seed=9):
    """Clustered embeddings (12 centres + 0.2 x noise) for a table of n + 200 rows, n candidate rows of it, relevance in
    descending order; `prop` plants the case's input property.  → (tab fp32, cand u32, rel f64, index of the zero row or None)"""
    rng = np.random.default_rng(seed)
    n_tab = n + 200
    centers = rng.standard_normal((12, dim)).astype(np.float32)
    tab = (centers[rng.integers(0, 12, n_tab)] + 0.2 * rng.standard_normal((n_tab, dim))).astype(np.float32)
    cand = rng.choice(n_tab, n, replace=False).astype(np.uint32)
    rel = np.sort(rng.random(n))[::-1].copy()
    zero = None
    if prop == "duplicates":                 # a quarter of the candidates are exact copies of candidate 0
        cand[rng.integers(0, n, n // 4)] = cand[0]
    elif prop == "ties":                     # relevance with eleven distinct values
        rel = np.sort(np.round(rng.random(n), 1))[::-1].copy()
    elif prop == "zero row":                 # the third candidate by relevance has an all-zero row: NaN once normalised
        zero = 2
        tab[cand[zero]] = 0.0
        rel[:3] += 0.05                      # (its NaN norm counts as 0.5, half of most others': stand clear of the next
                                             #  ranks by a fifth of gamma, or 50 picks of 1025 never reach it)
    elif prop == "const":                    # every first-maximum decision of the first pick is a tie
        rel = np.full(n, 0.5)
    elif prop == "nan":
        rel[5::97] = np.nan
    else:
        assert prop is None
    return tab, cand, rel, zero


def run_device(ctx, tab, cand, rel, gamma, topn, window, norm, pos, mode, star):
    """pg_ssd on rows of an uploaded table where a table can hold the dim, pg_ssd_emb on the same rows otherwise"""
    if tab.shape[1] % 64 == 0 and tab.shape[1] <= 256:
        t = pa.Table(ctx, tab.shape[0], tab.shape[1])
        t.upload(tab)
        try:
            return pa.ssd(ctx, t, cand, rel, gamma, topn, window, norm, pos, mode, star)
        finally:
            t.destroy()
    return pa.ssd_emb(ctx, tab[cand], rel, gamma, topn, window, norm, pos, mode, star)


def check_against_oracle(ctx, tab, cand, rel, topn, window, norm, pos, star, kind, gamma=GAMMA, mode=0, tiny=False):
    emb = o.ssd_embeddings(tab[cand], norm, pos)
    qual, ok = o.ssd_quality(rel, mode)
    assert ok
    with np.errstate(all="ignore"):
        want = o.ssd_window(emb, qual, gamma, topn, window, star)
    T = min(topn, len(rel))
    # conditions on the inputs, not on the device: the oracle's own sequence is a sequence of distinct items (its
    # volume has not overflowed) and diversity changed the order (a kernel returning 0, 1, 2, … would not pass)
    assert len(want) == T and len(set(want.tolist())) == T, "precondition: the oracle's sequence repeats an item"
    if not tiny:
        assert not np.array_equal(want, np.arange(T)), "precondition: the oracle's sequence is the identity"
    before = counters(ctx)
    got, gq = run_device(ctx, tab, cand, rel, gamma, topn, window, norm, pos, mode, star)
    after = counters(ctx)
    if not np.array_equal(got, want):
        m = min(len(got), len(want))
        diff = np.nonzero(got[:m] != want[:m])[0]
        first = int(diff[0]) if len(diff) else m
        pytest.fail("%s: picks differ from the oracle first at pick %d of %d (window %d, pop %s): device %s, oracle %s"
                    % (kind, first, T, window, first > (window if window > 1 else 5),
                       got[first:first + 4].tolist(), want[first:first + 4].tolist()))
    assert np.array_equal(bits(gq), bits(qual))
    assert moved(before, after) == only(kind)
    return want


#        dim  pos    norm   n     topn window star  property
GENERIC_CASES = [
    (3, False, True, 63, 63, 2, False, None),                # d1 < 16: all tail, every candidate picked
    (16, False, True, 1025, 40, 17, False, None),            # exactly one full block and no tail; n one past the 1024 threads
    (17, True, True, 1500, 60, 30, False, "duplicates"),     # d1 = 18
    (31, True, False, 300, 80, 5, True, None),               # d1 = 32, raw embeddings, SSD*
    (96, False, True, 1025, 50, 5, False, "zero row"),
    (200, True, True, 500, 64, 30, False, "ties"),
    (319, True, True, 700, 40, 17, False, None),             # d1 = 320 = kSsdMaxDim
    (320, False, True, 8192, 24, 5, False, None),            # both limits of pg_ssd at once
    (128, True, True, 2049, 48, 17, False, None),            # one past kSsdRegMaxN: a known width on the generic kernel
]
REG_CASES = [
    (128, True, True, 2048, 48, 17, False, "duplicates"),    # the LDS arrays are full
    (64, False, True, 257, 70, 30, False, "zero row"),
    (64, True, True, 256, 60, 20, False, "ties"),
    (128, False, False, 255, 60, 17, True, None),
]
GRID_CASES = [
    (64, False, True, 64, 64, 16, False, None),              # one full workgroup, every candidate picked, pick_ring wraps
    (64, True, True, 65, 65, 16, False, "duplicates"),       # a second workgroup with a single valid lane
    (128, True, True, 4097, 50, 16, False, "ties"),          # G = 65: the first use of the second reduction slot
    (128, False, True, 8192, 50, 16, False, "const"),        # G = 128, the size the mailbox arrays have
    (64, True, False, 4096, 40, 3, True, "nan"),             # NaN skipping, unnormalised, SSD*
    (128, True, True, 500, 120, 16, False, "zero row"),
]


# the fixed seed of make_inputs, except where the oracle's sequence on it is the identity (three dims leave nothing to
# diversify after three picks; with seed 9 not even those three change places)
SEED_OF = {(3, 63): 11}


def case_id(c):
    return "%dx%d-w%d-%s" % (c[3], c[0] + int(c[1]), c[5], (c[7] or "plain").replace(" ", "_"))


def run_case(ctx, case, kind):
    dim, pos, norm, n, topn, window, star, prop = case
    tab, cand, rel, zero = make_inputs(dim, n, prop, SEED_OF.get((dim, n), 9))
    want = check_against_oracle(ctx, tab, cand, rel, topn, window, norm, pos, star, kind)
    if zero is not None:                 # the NaN embedding is picked before the last pick: every ssd_bad branch ran
        assert zero in want[:-1].tolist(), "precondition: the zero row is picked before the last pick"
    return want


@pytest.mark.parametrize("case", GENERIC_CASES, ids=case_id)
def test_generic_kernel_matches_oracle(ctx, case):
    """ssd_kernel: the 16-wide blocks and their tails (d1 = 3, 16, 18, 32, 96, 201, 320), the i += blockDim stride loops
    (n = 1025 … 8192 on 1024 threads), e_sel / e_old at kSsdMaxDim, duplicates, ties, a NaN embedding."""
    run_case(ctx, case, GENERIC)


@pytest.mark.parametrize("case", REG_CASES, ids=case_id)
def test_register_kernel_matches_oracle(ctx, case):
    """ssd_kernel_reg<64 / 65 / 128 / 129>: full LDS arrays (n = 2048), n around the 256 threads, windows > 16."""
    run_case(ctx, case, REG)


@pytest.mark.parametrize("case", GRID_CASES, ids=case_id)
def test_grid_kernel_matches_oracle(ctx, case):
    """ssd_kernel_grid<64 / 65 / 128 / 129>: one and two workgroups, G = 65 and G = 128 (both reduction slots), the
    32-entry pick_ring with W = 16, NaN relevance, a NaN embedding."""
    want = run_case(ctx, case, GRID)
    if case[7] == "const":               # the winners come from both reduction slots
        assert (want // 64 >= 64).any() and (want // 64 < 64).any()


@pytest.mark.parametrize("dim,window,n,kind", [(96, 0, 200, GENERIC), (96, 1, 200, GENERIC),
                                               (64, 0, 200, GRID), (64, 1, 2100, GRID)])
def test_window_fallback_happens_before_the_dispatch(ctx, dim, window, n, kind):
    """window <= 1 means 5 (ssd_sort.go:357-360): the picks are those of window 5.  On a width only the generic kernel
    serves that is the generic kernel with W = 5.  On a known width a window of 5 belongs to the grid kernel whatever n is
    (the register kernel needs window > 16, so no fallback window reaches it); n = 2100 is beyond the register kernel too."""
    tab, cand, rel, _ = make_inputs(dim, n, None)
    want = check_against_oracle(ctx, tab, cand, rel, 30, window, True, True, False, kind)
    emb = o.ssd_embeddings(tab[cand], True, True)
    assert np.array_equal(want, o.ssd_window(emb, rel, GAMMA, 30, 5, False))


@pytest.mark.parametrize("dim,window,kind", [(96, 5, GENERIC), (64, 17, REG), (64, 16, GRID)])
def test_tiny_and_overlong_requests(ctx, dim, window, kind):
    """n = 1, n = 2 and topn > n on each kernel: T = min(topn, n) picks, each item once."""
    for n, topn in [(1, 10), (2, 2), (2, 7), (70, 75)]:
        tab, cand, rel, _ = make_inputs(dim, n, None)
        want = check_against_oracle(ctx, tab, cand, rel, topn, window, True, True, False, kind, tiny=n <= 2)
        assert sorted(want.tolist()) == list(range(n))


def test_unsupported_shapes_are_refused_and_the_context_stays_usable(ctx):
    """n = 8193, d1 = 321 and candidate rows outside the table: PG_ERR_UNSUPPORTED, no kernel launched, and the next
    call is served correctly."""
    tab, cand, rel, _ = make_inputs(64, 300, None)
    t = pa.Table(ctx, tab.shape[0], 64)
    t.upload(tab)
    rng = np.random.default_rng(4)
    big = rng.integers(0, tab.shape[0], 8193).astype(np.uint32)
    big_rel = np.sort(rng.random(8193))[::-1].copy()
    wide = rng.standard_normal((40, 321)).astype(np.float32)
    outside = cand.copy()
    outside[17] = tab.shape[0]
    refused = [
        lambda: pa.ssd(ctx, t, big, big_rel, GAMMA, 10, 5),
        lambda: pa.ssd_emb(ctx, tab[big], big_rel, GAMMA, 10, 5),
        lambda: pa.ssd_emb(ctx, wide[:, :320], rel[:40], GAMMA, 10, 5, ensure_pos_similarity=True),      # d1 = 321
        lambda: pa.ssd_emb(ctx, wide, rel[:40], GAMMA, 10, 5, ensure_pos_similarity=False),
        lambda: pa.ssd(ctx, t, outside, rel, GAMMA, 10, 5),
        lambda: pa.ssd(ctx, t, np.full(300, 0xFFFFFFFF, np.uint32), rel, GAMMA, 10, 5),
    ]
    emb = o.ssd_embeddings(tab[cand], True, True)
    want = o.ssd_window(emb, rel, GAMMA, 40, 5, False)
    for call in refused:
        before = counters(ctx)
        with pytest.raises(pa._lib.PgError) as ei:
            call()
        assert ei.value.code == UNSUPPORTED
        assert counters(ctx) == before
        got, _ = pa.ssd(ctx, t, cand, rel, GAMMA, 40, 5)
        assert np.array_equal(got, want)
    t.destroy()


def test_coalesced_ssd_calls_match_oracle(ctx):
    """pg_coalescer_ssd from 64 threads at once, two shapes mixed (130 candidates with the appended 1, 300 without) over
    a 64-wide table: EVERY caller's picks and quality scores equal the oracle's (not pg_ssd's — an error the two paths
    share would pass that), and the batched launches are fewer than the callers."""
    callers = 64
    rng = np.random.default_rng(31)
    n_tab, d = 3000, 64
    centers = rng.standard_normal((12, d)).astype(np.float32)
    tab = (centers[rng.integers(0, 12, n_tab)] + 0.2 * rng.standard_normal((n_tab, d))).astype(np.float32)
    t = pa.Table(ctx, n_tab, d)
    t.upload(tab)
    shapes = [(130, True, 25, 8, 1), (300, False, 40, 5, 0)]        # n, pos, topn, window, norm_quality_score
    cand, rel, want, wq = [], [], [], []
    for i in range(callers):
        n, pos, topn, window, mode = shapes[i % 2]
        cand.append(rng.choice(n_tab, n, replace=False).astype(np.uint32))
        rel.append(np.sort(rng.random(n))[::-1].copy())
        q, ok = o.ssd_quality(rel[i], mode)
        assert ok
        w = o.ssd_window(o.ssd_embeddings(tab[cand[i]], True, pos), q, GAMMA, topn, window, False)
        assert len(set(w.tolist())) == topn and not np.array_equal(w, np.arange(topn))
        want.append(w)
        wq.append(q)
    # depth 1: every batch runs on this context, so its counters see all of them
    co = pa.Coalescer(ctx, t, 100, algos=[], depth=1, max_wait_us=3000, max_rerank_items=512)
    got = [None] * callers

    def call(i):
        n, pos, topn, window, mode = shapes[i % 2]
        got[i] = co.ssd(cand[i], rel[i], GAMMA, topn, window, ensure_pos_similarity=pos, norm_quality_score=mode)
    before = counters(ctx)
    run_threads(callers, call)
    after = counters(ctx)
    st = co.stats()
    co.destroy()
    t.destroy()
    for i in range(callers):
        assert np.array_equal(got[i][0], want[i]), "caller %d (shape %s): picks differ from the oracle" % (i, shapes[i % 2])
        assert np.array_equal(bits(got[i][1]), bits(wq[i]))
    grew = moved(before, after)
    assert grew[REG] == 0 and grew[GENERIC] == 0
    assert st.requests[4] == callers and grew[GRID] == st.batches[4]
    assert 0 < grew[GRID] < callers
