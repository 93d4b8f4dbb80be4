"""GPU tests of the SSDSort stage (csrc/ssd.hip: pg_ssd_sort_dev) against tests/ssd_stage_ref.py, by bits: every
element of d_out_pos, d_out_count, d_out_rows and d_out_quality.  Embeddings are clustered and GAMMA is test_gpu_ssd.py's, and every
case asserts on the REFERENCE that its re-ranked requests leave the arriving order, so an identity answer cannot pass.  Counts sit
on the grid kernel's edges (0, 1, 2, a wave of 64 and its neighbours, two workgroups and one lane), several travel in one call, the
slots behind a count hold garbage, and every output carries a guard region behind it that must stay untouched."""
import numpy as np
import pytest

import pairec_amd as pa
import ssd_stage_ref as ref
from oracle import oracle as o
from pairec_amd._lib import PgError
from test_gpu_mixsort import Guarded
from test_gpu_ssd import GAMMA, GRID, counters, moved, only

pytestmark = pytest.mark.gpu

N_TAB, OUTSIDE = 1500, 60
HUGE = np.uint64((1 << 40) + 5)
INVALID, UNSUPPORTED = -1, -4


class World:
    pass


@pytest.fixture(scope="module")
def world(ctx):
    """one clustered table per width (12 centres + 0.2 x noise, as test_gpu_ssd.make_inputs), uploaded once"""
    w = World()
    w.tab, w.t = {}, {}
    for dim in (64, 128):
        rng = np.random.default_rng(900 + dim)
        centers = rng.standard_normal((12, dim)).astype(np.float32)
        w.tab[dim] = (centers[rng.integers(0, 12, N_TAB)] + 0.2 * rng.standard_normal((N_TAB, dim))).astype(np.float32)
        w.t[dim] = pa.Table(ctx, N_TAB, dim)
        w.t[dim].upload(w.tab[dim])
    yield w
    for t in w.t.values():
        t.destroy()


def make_case(rng, nq, cap, counts=None, order=True, source=True, garbage=True):
    """Every request: its count's worth of distinct table rows with pairwise distinct scores, descending along the list, scattered
    over the elements by a permutation; the slots behind the count hold garbage rows (inside the table too) and garbage scores."""
    rows = np.full((nq, cap), ref.PAD64, np.uint64)
    score = np.zeros((nq, cap))
    ordr = np.zeros((nq, cap), np.uint32)
    for q in range(nq):
        c = cap if counts is None else int(counts[q])
        perm = rng.permutation(cap) if order else np.arange(cap)
        ordr[q] = perm
        rows[q, perm[:c]] = rng.choice(N_TAB, c, replace=False)
        score[q, perm[:c]] = np.sort(rng.choice(np.arange(1, 100000), c, replace=False) / 100000.0)[::-1]
        if garbage and c < cap:
            rows[q, perm[c:]] = rng.integers(0, N_TAB + OUTSIDE, cap - c)
            score[q, perm[c:]] = rng.choice([np.nan, np.inf, -np.inf, 1e300, 0.0, 77.5], cap - c)
            ordr[q, c:] = np.where(rng.random(cap - c) < 0.3, cap + rng.integers(0, 1 << 20, cap - c), perm[c:])
    return dict(nq=nq, cap=cap, rows=rows, score=score, order=ordr if order else None,
                source=rng.integers(0, 5, (nq, cap)).astype(np.uint8) if source else None,
                count=None if counts is None else np.asarray(counts, dtype=np.uint32), enable=None)


def run_dev(ctx, table, case, p, rows_out=True, quality_out=True):
    nq, cap = case["nq"], case["cap"]
    outs = [np.empty((nq, cap), np.uint32), np.empty(nq, np.uint32), np.empty((nq, cap), np.uint64) if rows_out else None,
            np.empty((nq, cap), np.uint64) if quality_out else None]
    g = Guarded(ctx)
    try:
        d_in = [g.put(case[k]) for k in ("order", "rows", "score", "source", "count", "enable")]
        d_out = [g.out(a) if a is not None else 0 for a in outs]
        ctx.ssd_sort_dev(table, nq, cap, *d_in, p["gamma"], p["topn"], p["window"], *d_out,
                         **{k: p[k] for k in p if k not in ("gamma", "topn", "window")})
        g.fetch()
    finally:
        g.free()
    return outs


def check(ctx, w, dim, case, p, rerank="all", tiny=False):
    """device == restatement by bits; rerank: which requests the reference must have re-ranked ("all" of those with entries, a
    list, or None for "do not care"); unless tiny, every re-ranked request of more than 8 picks must leave the arriving order, and
    at least one such request must exist"""
    pos, cnt, orow, qbits, picks = ref.stage(w.tab[dim], 0, case["rows"], case["score"], p, order=case["order"], source=case["source"],
                                             count=case["count"], enable=case["enable"])
    if rerank == "all":
        rerank = [q for q in range(case["nq"]) if case["count"] is None or case["count"][q] > 0]
    if rerank is not None:
        assert [q for q in range(case["nq"]) if picks[q] is not None] == list(rerank), "precondition: which requests are re-ranked"
    moved_ = [q for q in range(case["nq"]) if picks[q] is not None and len(picks[q]) > 8]
    for q in moved_:
        assert len(set(picks[q])) == len(picks[q])
        assert picks[q] != list(range(len(picks[q]))), "precondition: the reference's picks of request %d are the identity" % q
    assert tiny or moved_, "precondition: no request of the case is re-ranked over more than 8 picks"
    g_pos, g_cnt, g_row, g_q = run_dev(ctx, w.t[dim], case, p)
    assert np.array_equal(g_cnt, cnt)
    for q in range(case["nq"]):
        assert np.array_equal(g_pos[q], pos[q]), "request %d: positions differ (count %d): device %s, reference %s" % (
            q, cnt[q], g_pos[q][:8].tolist(), pos[q][:8].tolist())
    assert np.array_equal(g_row, orow)
    assert np.array_equal(g_q, qbits)
    return pos, cnt, picks


def test_ragged_counts_in_one_batch(ctx, world):
    """nq 8, cap 200, counts 0, 1, 2, 63, 64, 65, 129, 200 in one launch: d1 = 65, window 5, topn 20 — the window pop runs wherever
    n_q allows; the slots behind a count hold garbage rows and scores"""
    rng = np.random.default_rng(1)
    case = make_case(rng, 8, 200, counts=[0, 1, 2, 63, 64, 65, 129, 200])
    _, cnt, _ = check(ctx, world, 64, case, ref.params(gamma=GAMMA, topn=20, window=5))
    assert cnt.tolist() == [0, 1, 2, 20, 20, 20, 20, 20]


@pytest.mark.parametrize("star", [False, True], ids=["ssd", "star"])
@pytest.mark.parametrize("window", [2, 16])
@pytest.mark.parametrize("d1", [64, 65, 128, 129])
def test_widths_windows_star(ctx, world, d1, window, star):
    """every instantiation of the grid kernel with a count per request: nq 3, cap 130 (G = 3), counts 130, 65, 37"""
    rng = np.random.default_rng(d1 * 100 + window)
    case = make_case(rng, 3, 130, counts=[130, 65, 37])
    check(ctx, world, d1 & ~1, case, ref.params(gamma=GAMMA, topn=30, window=window, use_ssd_star=star, ensure_pos_similarity=bool(d1 & 1)))


@pytest.mark.parametrize("d1", [65, 128])
def test_topn_one_and_topn_beyond_the_list(ctx, world, d1):
    rng = np.random.default_rng(d1)
    case = make_case(rng, 3, 130, counts=[130, 65, 37])
    p = ref.params(gamma=GAMMA, topn=1, window=5, ensure_pos_similarity=bool(d1 & 1))
    _, cnt, _ = check(ctx, world, d1 & ~1, case, p, tiny=True)
    assert cnt.tolist() == [1, 1, 1]
    pos, cnt, _ = check(ctx, world, d1 & ~1, case, dict(p, topn=130))       # everything is picked, each entry once
    assert cnt.tolist() == [130, 65, 37]
    for q in range(3):
        assert sorted(pos[q, :cnt[q]].tolist()) == sorted(case["order"][q, :cnt[q]].tolist())


@pytest.mark.parametrize("mode,flat", [(1, 0.0), (1, 0.5), (2, 0.0), (2, 0.5)], ids=["std-zeros", "std-equal", "minmax-zeros", "minmax-equal"])
def test_normalisation_and_its_bail_out(ctx, world, mode, flat):
    """modes 1 and 2: d_out_quality bits equal the oracle's; the middle request's scores are all `flat` (mean 0 / variance 0 / span 0):
    it returns its cut list unchanged while its neighbours are re-ranked"""
    rng = np.random.default_rng(10 + mode)
    case = make_case(rng, 3, 150, counts=[150, 90, 131])
    real = case["order"][1, :90]
    case["score"][1, real] = flat
    p = ref.params(gamma=GAMMA, topn=25, window=5, norm_quality_score=mode, candidate_count=70)
    pos, cnt, _ = check(ctx, world, 64, case, p, rerank=[0, 2])
    assert cnt.tolist() == [25, 70, 25] and np.array_equal(pos[1, :70], real[:70])


CUT_CASES = {
    # candidate_count below topn (cut to topn), between, above the list; the min-percent cut on top of it
    "cc<topn": dict(p=dict(topn=20, candidate_count=7)),
    "cc": dict(p=dict(topn=20, candidate_count=64)),
    "cc>list": dict(p=dict(topn=20, candidate_count=500)),
    "pct": dict(p=dict(topn=20, min_score_percent=0.6)),
    "cc+pct": dict(p=dict(topn=20, candidate_count=100, min_score_percent=0.35)),
    "pct-at-topn": dict(p=dict(topn=20, min_score_percent=0.999999)),          # the first index looked at fails: exactly topn remain
    "pct-negative-top": dict(p=dict(topn=20, min_score_percent=0.6), shift=-200.0),      # quotients >= 1: nothing is cut
    # the split
    "split": dict(p=dict(topn=20, filter_source_mask=0b01010)),
    "split+cuts": dict(p=dict(topn=20, filter_source_mask=0b00110, candidate_count=50, min_score_percent=0.3, norm_quality_score=2)),
    "only-backup": dict(p=dict(topn=20, filter_source_mask=0b01010), all_source=3, rerank=[0, 2]),
    "mask-without-source": dict(p=dict(topn=20, filter_source_mask=0b11111), source=False),
    # the gates
    "enable": dict(p=dict(topn=20, filter_source_mask=0b00010), enable=[1, 0, 1], rerank=[0, 2]),
    "abort": dict(p=dict(topn=20, abort_run_cnt=90), rerank=[0, 2]),                # request 1 holds exactly 90 real entries, request 2 91
    "gamma0": dict(p=dict(topn=20, gamma=0.0, candidate_count=30, filter_source_mask=0b00100), rerank=[]),
    # padding inside the count, no order
    "padding": dict(p=dict(topn=20), pads=True),
    "no-order": dict(p=dict(topn=20, candidate_count=60), order=False),
}


@pytest.mark.parametrize("name", list(CUT_CASES))
def test_cuts_split_gates_and_padding(ctx, world, name):
    c = CUT_CASES[name]
    rng = np.random.default_rng(33)
    case = make_case(rng, 3, 180, counts=[180, 90, 91], order=c.get("order", True), source=c.get("source", True))
    if "shift" in c:
        for q in range(3):
            real = (case["order"][q] if case["order"] is not None else np.arange(180))[:case["count"][q]]
            case["score"][q, real] += c["shift"]
    if "all_source" in c:
        case["source"][1, :] = c["all_source"]
    if "enable" in c:
        case["enable"] = np.asarray(c["enable"], dtype=np.uint8)
    if c.get("pads"):                       # UINT64_MAX rows and rows outside the table inside the count: they leave the list first
        for q in range(3):
            real = case["order"][q, :case["count"][q]]
            case["rows"][q, real[3::7]] = ref.PAD64
            case["rows"][q, real[5::11]] = N_TAB + 3
            case["rows"][q, real[0]] = HUGE
    p = ref.params(**dict(dict(gamma=GAMMA, window=5), **c["p"]))
    pos, cnt, picks = check(ctx, world, 64, case, p, rerank=c.get("rerank", "all"), tiny=name == "gamma0")
    if name == "abort":
        assert cnt.tolist() == [20, 90, 20]
    if name == "pct-at-topn":
        assert all(len(pk) == 20 for pk in picks) and cnt.tolist() == [20, 20, 20]
    if name == "pct-negative-top":
        assert cnt.tolist() == [20, 20, 20] and max(max(pk) for pk in picks) >= 20
    if name == "only-backup":
        assert cnt[1] == 90 and np.array_equal(pos[1, :90], case["order"][1, :90])
    if name == "split":
        assert cnt.min() > 20                                           # picks, then the backup in order


def test_two_launches_in_one_call(ctx, world):
    """nq 256, cap 320 (G = 5: a launch holds 4 workgroups per CU / 5 = 204 requests on 256 CUs, so the call takes two and the
    per-request words move with the slice), topn 8, ragged counts: all 256 equal the reference"""
    rng = np.random.default_rng(77)
    counts = rng.integers(0, 321, 256)
    counts[[0, 100, 204, 205, 255]] = [320, 0, 1, 320, 319]
    case = make_case(rng, 256, 320, counts=counts, source=False)
    pos, cnt, picks = check(ctx, world, 64, case, ref.params(gamma=GAMMA, topn=8, window=5), tiny=True)
    assert sum(pk is not None and pk != list(range(len(pk))) for pk in picks) > 200


def test_the_chain_feeds_the_stage(ctx, world):
    """pg_recommend_candidates_dnn3_dev's order, fused scores and rows go straight into the stage on the device; the result equals
    the restatement applied to the downloaded outputs"""
    nq, cap, dim = 4, 160, 128
    rng = np.random.default_rng(5)
    counts = np.array([160, 97, 0, 129], np.uint32)
    rows = np.full((nq, cap), ref.PAD64, np.uint64)
    for q in range(nq):
        rows[q, :counts[q]] = rng.choice(N_TAB, counts[q], replace=False)
    rows[0, 7] = N_TAB + 9                                              # a row outside the table inside the count
    score = rng.random((nq, cap))
    users = rng.standard_normal((nq, dim)).astype(np.float32)
    wts = o.Dnn3Weights()
    m = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_F32, pa.pack_dnn3(wts.w1, wts.b1, wts.w2, wts.b2, wts.w3, wts.b3, 128))
    ex = pa.Expr("${gpu_dnn}*0.7+${current_score}*0.3")
    p = ref.params(gamma=GAMMA, topn=24, window=5, candidate_count=80, norm_quality_score=1)
    fused, order = np.empty((nq, cap)), np.empty((nq, cap), np.uint32)
    outs = [np.empty((nq, cap), np.uint32), np.empty(nq, np.uint32), np.empty((nq, cap), np.uint64), np.empty((nq, cap), np.uint64)]
    g = Guarded(ctx)
    try:
        d_u, d_rows, d_score, d_cnt = g.put(users), g.put(rows), g.put(score), g.put(counts)
        d_rk, d_fu, d_or = g.out(np.empty((nq, cap), np.float32)), g.out(fused), g.out(order)
        pa._lib.check(ctx.L.pg_recommend_candidates_dnn3_dev(ctx.h, world.t[dim].h, m.h, ex.h, b"gpu_dnn", d_u, nq, cap, d_rows, d_score, d_cnt,
                                                             d_rk, d_fu, d_or))
        d_out = [g.out(a) for a in outs]
        ctx.ssd_sort_dev(world.t[dim], nq, cap, d_or, d_rows, d_fu, 0, d_cnt, 0, p["gamma"], p["topn"], p["window"], *d_out,
                         ensure_pos_similarity=True, candidate_count=80, norm_quality_score=1)
        g.fetch()
    finally:
        g.free()
        ex.free()
        m.destroy()
    pos, cnt, orow, qbits, picks = ref.stage(world.tab[dim], 0, rows, fused, p, order=order, count=counts)
    assert [pk is not None for pk in picks] == [True, True, False, True] and all(pk != list(range(24)) for pk in picks if pk)
    assert np.array_equal(outs[1], cnt) and np.array_equal(outs[0], pos) and np.array_equal(outs[2], orow) and np.array_equal(outs[3], qbits)
    assert cnt.tolist() == [24, 24, 0, 24] and not (orow == np.uint64(N_TAB + 9)).any()


def test_counters_and_refusals(ctx, world):
    """ssd_grid_calls grows by one per call (two launches or one), the register and generic counters stay; every refusal returns
    its code with the outputs untouched and the context usable"""
    rng = np.random.default_rng(3)
    case = make_case(rng, 2, 100, counts=[100, 40])
    p = ref.params(gamma=GAMMA, topn=10, window=5)
    before = counters(ctx)
    check(ctx, world, 64, case, p)
    assert moved(before, counters(ctx)) == only(GRID)
    t192 = pa.Table(ctx, 64, 192)
    feats = pa.Features(ctx, N_TAB)
    feats.set_column("cat", pa.F_I32, (np.arange(N_TAB) % 4).astype(np.int32))
    view = world.t[64].view(feats, "cat", "==", 1)
    t64 = world.t[64]
    refusals = [
        (UNSUPPORTED, "nq", t64, dict(nq=257), {}),
        (UNSUPPORTED, "cap", t64, dict(cap=16385), {}),
        (UNSUPPORTED, "8192", t64, dict(cap=8193), {}),                     # n_max = cap without a candidate_count
        (UNSUPPORTED, "8192", t64, dict(cap=9000), dict(candidate_count=8193)),
        (UNSUPPORTED, "batchable", t192, {}, {}),
        (UNSUPPORTED, "batchable", t64, {}, dict(window=17)),
        (UNSUPPORTED, "view", view, {}, {}),
        (INVALID, "topn", t64, {}, dict(topn=0)),
        (INVALID, "norm_quality_score", t64, {}, dict(norm_quality_score=3)),
        (INVALID, "norm_quality_score", t64, {}, dict(norm_quality_score=-1)),
    ]
    nq, cap = case["nq"], case["cap"]
    g = Guarded(ctx)
    try:
        d_in = [g.put(case[k]) for k in ("order", "rows", "score", "source", "count", "enable")]
        outs = [np.empty((nq, cap), np.uint32), np.empty(nq, np.uint32), np.empty((nq, cap), np.uint64), np.empty((nq, cap), np.uint64)]
        d_out = [g.out(a) for a in outs]
        before = counters(ctx)
        for code, word, table, shape, change in refusals:
            q = dict(p, **change)
            with pytest.raises(PgError) as ei:
                ctx.ssd_sort_dev(table, shape.get("nq", nq), shape.get("cap", cap), *d_in, q["gamma"], q["topn"], q["window"], *d_out,
                                 **{k: q[k] for k in q if k not in ("gamma", "topn", "window")})
            assert ei.value.code == code and word in str(ei.value), (word, str(ei.value))
        assert counters(ctx) == before
        g.fetch()
        for a in outs:
            assert np.all(a.reshape(-1).view(np.uint8) == 0xA5), "a refused call wrote an output"
    finally:
        g.free()
        view.destroy()
        feats.destroy()
        t192.destroy()
    # the limit itself is served: a cut list bounded at 8 192 by the candidate count ... on a small cap the bound is the cap
    before = counters(ctx)
    check(ctx, world, 64, case, dict(p, candidate_count=8192))
    assert moved(before, counters(ctx)) == only(GRID)


class _Tensor:
    """what ssd_sort_dev needs of a torch tensor: its device address"""

    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


def test_the_python_layers(ctx, world):
    """ctx.ssd_sort_dev on objects with .data_ptr() in place of addresses: it returns the outputs it was given, (pos, count[, rows]
    [, quality])"""
    rng = np.random.default_rng(8)
    case = make_case(rng, 3, 120, counts=[120, 64, 0])
    p = ref.params(gamma=GAMMA, topn=16, window=5, norm_quality_score=2, filter_source_mask=0b100)
    pos, cnt, _, qbits, _ = ref.stage(world.tab[64], 0, case["rows"], case["score"], p, order=case["order"], source=case["source"], count=case["count"])
    opts = {k: p[k] for k in p if k not in ("gamma", "topn", "window")}
    out_pos, out_cnt, out_q = np.empty((3, 120), np.uint32), np.empty(3, np.uint32), np.empty((3, 120), np.uint64)
    g = Guarded(ctx)
    try:
        d_in = [_Tensor(g.put(case[k])) for k in ("order", "rows", "score", "source", "count")]
        outs = (_Tensor(g.out(out_pos)), _Tensor(g.out(out_cnt)), _Tensor(g.out(out_q)))
        ret = ctx.ssd_sort_dev(world.t[64], 3, 120, *d_in, None, GAMMA, 16, 5, outs[0], outs[1], d_out_quality=outs[2], **opts)
        assert ret == outs
        g.fetch()
    finally:
        g.free()
    assert np.array_equal(out_pos, pos) and np.array_equal(out_cnt, cnt) and np.array_equal(out_q, qbits)
