"""The bf16-shadow screen (csrc/recall.hip: screen_kernel with I8 = false — every dim-64 table and every dim-128 table that leaves
the int8 shadow) at the places where a screen goes wrong: block norms that differ by six decades between neighbours with the
answers right at the threshold, ragged ends, tables that change, a winner in every accumulator slot, every query-count
instantiation, hostile values, the guards of screen_thr_kernel from both sides, filters, subnormal rows.  Every recall goes
through pa.Table.recall_topk and is compared with the CPU oracle by bits: ids, order, scores.  The fixtures and their numpy
model are screen_bf16_ref.py; test_screen_bf16_cpu.py shows on the CPU that they are sharp."""
import numpy as np
import pytest

import pairec_amd as pa
import screen_bf16_ref as ref
from oracle import oracle as o

pytestmark = pytest.mark.gpu

DIMS = (64, 128)
K = ref.Sharp.K
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def recall_on_the_shadow(ctx, t, call, rows=None):
    """call() under the proof that the bf16 screen gave its answer: the table is on the bf16 shadow, no screened plan overflowed, no
    plan was run again, and the scan launches streamed fewer than 3 bytes per element — the 2-byte shadow plus a plan's small exact
    seed, not the fp32 rows.  A case that completes on the exact scan fails here."""
    assert t.screen_info()[0] == 2, "the table is not on the bf16 shadow: the test no longer reaches the kernel it is about"
    st = ctx.stats()
    before = (st.recall_screen_overflows, st.recall_rescans)
    out = call()
    st = ctx.stats()
    assert (st.recall_screen_overflows, st.recall_rescans) == before, "a screened plan gave up: the answer is another plan's"
    scanned = ctx.last_scan_kernel()[1]
    assert 0 < scanned < (t.rows if rows is None else rows) * t.dim * 3, "the pass streamed the fp32 rows"
    return out, scanned


def check(ctx, t, tab, q, k, sel=None, want=None):
    """recall_topk against the oracle on the queries `sel` (all by default); want: (rows, scores) of the oracle if already known"""
    (rows, sc, cnt), scanned = recall_on_the_shadow(ctx, t, lambda: t.recall_topk(q, k))
    idx = np.arange(len(q)) if sel is None else np.asarray(sel)
    orow, osc = want if want is not None else o.recall_topk(tab, q[idx], k)
    assert cnt.tolist() == [min(k, len(tab))] * len(q)
    assert np.array_equal(rows[idx], orow)
    assert np.array_equal(bits(sc[idx]), bits(osc))
    assert rows.max() < len(tab)
    return rows, scanned


# ---- the fixture of (a), one table per dim for the whole module (never written to), the oracle's answers computed once ----------
_sharp = {}


def sharp(ctx, dim):
    if dim not in _sharp:
        fx = ref.Sharp(dim)
        t = pa.Table(ctx, fx.rows, dim)
        t.upload(fx.tab)
        _sharp[dim] = (fx, t, o.recall_topk(fx.tab, fx.q, K))
    return _sharp[dim]


def sharp_check(ctx, dim, nq, sel=None):
    fx, t, (orow, osc) = sharp(ctx, dim)
    idx = np.arange(nq) if sel is None else np.asarray(sel)
    return check(ctx, t, fx.tab, fx.q[:nq], K, idx, (orow[idx], osc[idx]))


def plan_bytes(rows, dim, k, sampled_eighth):
    """What the scan launches of a recall stream on a table of `rows` rows (csrc/recall_plan_math.hpp): the pilot plan reads a
    sample of every 8th block — its first 2048 rows on the exact scan, 4 bytes an element, the rest on the shadow — and then
    the whole shadow once, whether or not that pass is split for the refinement."""
    blocks = (rows + 31) // 32
    sample_rows = ((rows // 32) // 8) * 32
    assert sampled_eighth and sample_rows > 2048
    return dim * (2048 * 4 + (sample_rows - 2048) * 2 + blocks * 32 * 2)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("nq", [8, 200])
def test_block_norms_that_differ_default_plans(ctx, dim, nq):
    """(a) The sharp queries 0 and 1 have all K members in loud blocks (norm 10 .. 1000) next to quiet ones (norm 0.01), within
    0.003 ||q|| of the K-th score: with a neighbour's norm a third of them is lost (test_screen_bf16_cpu.py).  A table of this size
    takes the pilot plan, whose sample walks every 8th block in sample_block's permuted order; the scan bytes say so."""
    fx, _, _ = sharp(ctx, dim)
    _, scanned = sharp_check(ctx, dim, nq)
    assert scanned == plan_bytes(fx.rows, dim, K, True)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("nq", [8, 200])
def test_block_norms_that_differ_sampled_plan_with_refinement(ctx, dim, nq):
    """(a) The sampled plan forced as test_recall_threshold_refinement_any_row_order forces it: an eighth of the blocks as the pilot
    sample, the full pass split after its first quarter and the thresholds raised (refine_min_rows 0).  That the sampled plan ran
    shows in the scan bytes — sample + one whole pass of the shadow; the growing-chunk plan would stream 4096 rows exactly and the
    rest of the shadow once, 16 KB x dim less — and, for a developer, in debug_scan's "plan 0 scan launch" lines on stderr."""
    fx, _, _ = sharp(ctx, dim)
    for name, v in (("refine_min_rows", "0"), ("pilot_fraction", "0.125")):
        ctx.set_option(name, v)
    try:
        _, scanned = sharp_check(ctx, dim, nq)
        assert scanned == plan_bytes(fx.rows, dim, K, True)
        grow = dim * (4096 * 4 + (fx.rows - 4096) * 2)
        assert scanned > grow
    finally:
        ctx.set_option("refine_min_rows", str(1 << 24))
        ctx.set_option("pilot_fraction", "0")


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("tail", [32, 1, 31])
def test_ragged_ends(ctx, dim, tail):
    """(b) rows = 0, 1, 31 (mod 32): the last block is loud and its last row — at remainder 1 its only row — is the best row of
    sharp query 0; no row past the end is reported."""
    fx = ref.Sharp(dim, rows=ref.ragged_rows(tail))
    assert fx.rows % 32 == tail % 32 and fx.last_owner == 0
    t = pa.Table(ctx, fx.rows, dim)
    t.upload(fx.tab)
    rows, _ = check(ctx, t, fx.tab, fx.q[:8], K)
    assert rows[0, 0] == fx.rows - 1
    t.destroy()


@pytest.mark.parametrize("dim", DIMS)
def test_a_table_that_changes(ctx, dim):
    """(c) One loud row (norm 1000, at 0.1999 ||q|| along sharp query 0: inside the answer, next to the K-th score) uploaded into a
    quiet block, before and after a swap: the block's norm must follow, the new row must come back."""
    fx = ref.Sharp(dim)
    other = ref.Sharp(dim, seed=8)
    q = fx.q[:8]
    ta, tb = pa.Table(ctx, fx.rows, dim), pa.Table(ctx, fx.rows, dim)
    ta.upload(fx.tab)
    tb.upload(other.tab)
    check(ctx, ta, fx.tab, q, K)                                  # builds ta's shadow and block norms
    check(ctx, tb, other.tab, q, K)
    tab = fx.tab.copy()
    r = 32 * 302 + 9                                              # block 302 = 2 (mod 3): quiet
    tab[r] = fx.loud_row(1, 1000.0, 0.1999)
    ta.upload(tab[r:r + 1], row0=r)
    rows, _ = check(ctx, ta, tab, q, K)
    assert r in rows[0].tolist()
    ta.swap(tb)                                                   # tb now holds `tab`, ta the other table
    check(ctx, ta, other.tab, q, K)
    r2 = 32 * 1502 + 31
    tab[r2] = fx.loud_row(2, 1000.0, 0.1999)
    tb.upload(tab[r2:r2 + 1], row0=r2)
    rows, _ = check(ctx, tb, tab, q, K)
    assert r in rows[0].tolist() and r2 in rows[0].tolist()
    ta.destroy()
    tb.destroy()


@pytest.mark.parametrize("dim", DIMS)
def test_a_winner_in_every_row_position_for_every_query(dim):
    """Cover argument of (d), checked on the planted table itself (no GPU): for each of the 256 queries j a planted row sits at each of
    the 32 positions p of a block.  In screen_kernel's 32x32 output layout position p is register r with (r & 3) + 8 (r >> 2) + 4 h =
    p — r = (p & 3) + 4 (p >> 3), half h = (p >> 2) & 1 — and query j is column block j >> 5, lane & 31 = j & 31: all 32 x 256
    (register, half, lane, column block) slots hold a true top-K row once."""
    _, _, plants = ref.planted(dim)
    seen = {(int(j), int(r % 32)) for j, r in plants}
    assert seen == {(j, p) for j in range(256) for p in range(32)}
    assert len({int(r) for _, r in plants}) == 256 * 32           # no two plants share a row
    slots = {(j >> 5, j & 31, (p & 3) + 4 * (p >> 3), (p >> 2) & 1) for j, p in seen}
    assert len(slots) == 8 * 32 * 16 * 2


@pytest.mark.parametrize("dim", DIMS)
def test_every_lane_register_and_column_slot(ctx, dim):
    """(d) 256 queries, K = 32: the answer of query j is exactly its 32 plants, one per row position of a block"""
    tab, q, plants = ref.planted(dim)
    t = pa.Table(ctx, len(tab), dim)
    t.upload(tab)
    rows, _ = check(ctx, t, tab, q, 32)
    mine = {}
    for j, r in plants:
        mine.setdefault(j, []).append(r)
    for j in range(256):
        assert sorted(rows[j].tolist()) == sorted(mine[j])
    t.destroy()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("nq", [1, 31, 32, 33, 64, 65, 128, 129, 143, 145, 200, 255, 256])
def test_query_counts(ctx, dim, nq):
    """(e) The four instantiations per dim — <D, 1, 8> up to 32 queries, <D, 2, 8> up to 64, <D, 4, 8> up to 128, <D, 8, 4> beyond —
    with the last column block just full, one over, nearly empty: first, middle and last query against the oracle, K answers for
    every query (check: cnt == K; an inactive column that added suspects or failed a plan would show in the counters)."""
    sharp_check(ctx, dim, nq, sorted({0, nq // 2, nq - 1}))


def growing_chunks(ctx):
    """the growing-chunk plan instead of the pilot plan: its later chunks are screened against the K-th best score of the rows
    before them — the highest threshold a row can meet"""
    class _Ctx:
        def __enter__(self):
            ctx.set_option("no_pilot", 1)

        def __exit__(self, *a):
            ctx.set_option("no_pilot", 0)
    return _Ctx()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("nq", [72, 200])
def test_hostile_values(ctx, dim, nq):
    """(f) Near-duplicates below bf16 resolution with a query along and one against them, exact duplicates, zero rows, a zero query,
    -0.0 components, a one-component query, and blocks of rows scaled by 1e-30 — their fp32 sum of squares is zero — with three
    queries whose best scores are the zero rows' and then those rows', ~ -1e-31.  Under the default plans, and under the
    growing-chunk plan, where the late 1e-30 rows meet a threshold that is one of the early ones' scores: with a margin of zero
    for such a block members are lost (test_screen_bf16_cpu.py shows which)."""
    tab, q = ref.hostile(dim, nq)
    t = pa.Table(ctx, len(tab), dim)
    t.upload(tab)
    want = o.recall_topk(tab, q, K)
    check(ctx, t, tab, q, K, want=want)
    with growing_chunks(ctx):
        check(ctx, t, tab, q, K, want=want)
    t.destroy()


@pytest.mark.parametrize("dim", DIMS)
def test_the_guards_from_both_sides(ctx, dim):
    """(g) Queries of norm 1e30 (eps_unit 8e27: screened) and 2e30 (stands aside) on unit rows; 1e27 (eps_unit x max_norm = 8e34:
    screened) and 2e27 (stands aside) on a table with rows of norm 1e10; ordinary queries between them, in one batch each.
    Which side each falls on is asserted on the model (test_screen_bf16_cpu.py)."""
    for tab, q, _, _ in ref.guard_tables(dim):
        t = pa.Table(ctx, len(tab), dim)
        t.upload(tab)
        check(ctx, t, tab, q, 100)
        t.destroy()


@pytest.mark.parametrize("dim", DIMS)
def test_filtered_in_place_and_through_a_view(ctx, dim):
    """(h) A flag column that admits every other loud block: one WhereClause recall served in place (the compact copy switched off)
    and one view, against the oracle on the admitted rows."""
    fx, t, _ = sharp(ctx, dim)
    idx = np.nonzero(fx.flag == 1)[0]
    assert fx.outlier_row is None or fx.flag[fx.outlier_row] == 1        # the view must leave the int8 shadow too
    nq = 40
    q = fx.q[:nq]
    orow, osc = o.recall_topk(fx.tab[idx], q, K)
    want_rows = idx[orow.astype(np.int64)].astype(np.uint64)
    feats = pa.Features(ctx, fx.rows)
    feats.set_column("flag", pa.F_I32, fx.flag)
    ctx.set_option("where_compact_max_rows", 0)
    try:
        (rows, sc, cnt), _ = recall_on_the_shadow(ctx, t, lambda: t.recall_topk_where(feats, "flag", "==", 1, q, K))
    finally:
        ctx.set_option("where_compact_max_rows", 8 << 20)
    assert cnt.tolist() == [K] * nq
    assert np.array_equal(rows, want_rows) and np.array_equal(bits(sc), bits(osc))
    v = t.view(feats, "flag", "==", 1)
    assert v.rows == idx.size
    (rows, sc, cnt), _ = recall_on_the_shadow(ctx, v, lambda: v.recall_topk(q, K))
    assert cnt.tolist() == [K] * nq
    assert np.array_equal(rows, want_rows) and np.array_equal(bits(sc), bits(osc))
    v.destroy()
    feats.destroy()


def exact_answer(ctx, t, q, k):
    ctx.set_option("recall_exact", 1)
    try:
        return t.recall_topk(q, k)
    finally:
        ctx.set_option("recall_exact", 0)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("name", sorted(ref.SUBNORMAL_M))
def test_subnormal_rows(ctx, dim, name):
    """(i) Rows whose only component is an fp32 subnormal (1.01e-39) or one of the smallest normals (1.19e-38): a bf16 keeps an
    absolute 2^-134 of them, not a relative 2^-9, and the block's fp32 sum of squares is zero.  Their scores against query 0
    (-2^90 e_0) are the only positive ones; the K = 16 best sit in block 500, which the growing-chunk plan screens against the
    score of rows 100-115 — 3 % (0.2 %) above every bf16 score of the block.  The screened answer must equal the exact scan's
    (recall_exact), and both the oracle's, under the default plans and under the growing-chunk plan."""
    tab, q = ref.subnormal(dim, ref.SUBNORMAL_M[name])
    t = pa.Table(ctx, len(tab), dim)
    t.upload(tab)
    k = 16
    erows, esc, _ = exact_answer(ctx, t, q, k)
    orow, osc = o.recall_topk(tab, q, k)
    assert orow[0].tolist() == list(range(16031, 16015, -1))
    for plan in ("default", "growing chunks"):
        if plan == "default":
            (rows, sc, cnt), _ = recall_on_the_shadow(ctx, t, lambda: t.recall_topk(q, k))
        else:
            with growing_chunks(ctx):
                (rows, sc, cnt), _ = recall_on_the_shadow(ctx, t, lambda: t.recall_topk(q, k))
        assert cnt.tolist() == [k] * len(q)
        assert np.array_equal(rows, erows) and np.array_equal(bits(sc), bits(esc)), "%s: the screen lost or reordered a row the exact scan keeps" % plan
    assert np.array_equal(erows, orow) and np.array_equal(bits(esc), bits(osc)), "the exact scan differs from the oracle"
    t.destroy()
