"""GPU tests of the candidate trim and of the coarse-rank cascade (csrc/trim.hip, pg_candidates_trim_dev,
pg_recommend_cascade_dnn3_dev) against tests/trim_ref.py: every output array is compared by bits, padding and counts included.
The sizes sit on the kernel's edges — a wave of 64 lanes, its chunk of 1 024 positions, the largest cap of 16 384."""
import numpy as np
import pytest

import fanin_ref
import pairec_amd as pa
import trim_ref as ref
from oracle import oracle as o
from pairec_amd._lib import PgError
from test_gpu_fanin import FUSION_TOL      # the device pow's ulps against operands below 5

pytestmark = pytest.mark.gpu

U64MAX = ref.U64MAX
FIX, ACC, ANY = ref.FIX, ref.ACCUMULATE, ref.ANY


def random_case(rng, nq, cap, n_src, pad=0.05, with_count=True, n64=3, n32=2):
    """(rows, score, source, count, planes_f64, source_mask, planes_f32): a handful of distinct scores beside continuous ones, so
    that ties occur inside a source, across sources and across chunk boundaries"""
    rows = rng.integers(0, 1 << 40, (nq, cap)).astype(np.uint64)
    rows[rng.random((nq, cap)) < pad] = U64MAX
    score = rng.standard_normal((nq, cap))
    tie = rng.random((nq, cap)) < 0.4
    score[tie] = rng.integers(-2, 3, (nq, cap))[tie] * 0.5
    source = rng.integers(0, n_src, (nq, cap)).astype(np.uint8)
    count = rng.integers(cap // 2, cap + 1, nq).astype(np.uint32) if with_count else None
    return (rows, score, source, count, rng.standard_normal((n64, nq, cap)), rng.integers(0, 256, (nq, cap)).astype(np.uint32),
            rng.standard_normal((n32, nq, cap)).astype(np.float32))


def check(ctx, rules, case, optional=False):
    rows, score, source, count, p64, mask, p32 = case
    got = ctx.candidates_trim(rules, rows, score, source, count, p64, mask, p32)
    ref.same(got, ref.trim(rules, rows, score, source, count, p64, mask, p32))
    if optional:
        # every optional array absent (the source stays where rules name sources), and one at a time
        src = None if rules[0][0] == ANY else source
        ref.same(ctx.candidates_trim(rules, rows, score, src), ref.trim(rules, rows, score, src))
        ref.same(ctx.candidates_trim(rules, rows, score, source, count), ref.trim(rules, rows, score, source, count))
        ref.same(ctx.candidates_trim(rules, rows, score, source, None, p64), ref.trim(rules, rows, score, source, None, p64))
        ref.same(ctx.candidates_trim(rules, rows, score, source, None, None, mask), ref.trim(rules, rows, score, source, None, None, mask))
        ref.same(ctx.candidates_trim(rules, rows, score, src, None, None, None, p32), ref.trim(rules, rows, score, src, None, None, None, p32))
    return got


def mixed_rules(n_src, cap):
    """the reference's documented shape: a fix quota first, then accumulators that fill up to running totals"""
    rules = [(0, FIX, max(1, cap // 5))]
    for s in range(1, n_src):
        rules.append((s, ACC, (cap * s) // (2 * n_src) + 1))
    return rules


# ---- sizes and sources --------------------------------------------------------------------------------------------------------------

SIZES = [(nq, cap) for cap in (1, 63, 64, 65, 1023, 1024, 1025, 2049, 16384) for nq in (1, 3, 256) if nq < 256 or cap <= 1025]


@pytest.mark.parametrize("nq,cap", SIZES)
def test_sizes_and_sources(ctx, nq, cap):
    rng = np.random.default_rng(1000 * nq + cap)
    n_src = 1 + (cap + nq) % 8                                       # 1 .. 8 sources over the cases
    case = random_case(rng, nq, cap, n_src, n64=n_src, n32=1)
    check(ctx, mixed_rules(n_src, cap), case, optional=nq == 3)
    check(ctx, [(ANY, FIX, max(1, cap // 3))], case)


@pytest.mark.parametrize("n_src", range(1, 9))
def test_one_to_eight_sources(ctx, n_src):
    rng = np.random.default_rng(n_src)
    case = random_case(rng, 3, 1500, n_src, n64=n_src)
    check(ctx, mixed_rules(n_src, 1500), case)
    check(ctx, [(s, FIX, 100 + s) for s in reversed(range(n_src))], case)        # rule order is not source order


# ---- rule sets ----------------------------------------------------------------------------------------------------------------------

CAP_R = 1500
RULES = {
    "fix only": [(0, FIX, 100), (1, FIX, 200), (2, FIX, 50), (3, FIX, 1), (4, FIX, 300)],
    "accumulate only": [(0, ACC, 100), (1, ACC, 300), (2, ACC, 350), (3, ACC, 351), (4, ACC, 900)],
    "fix, then accumulators": [(2, FIX, 150), (0, ACC, 200), (1, ACC, 500), (3, ACC, 600)],
    "a source without entries": [(7, FIX, 100), (0, ACC, 200), (6, ACC, 300), (1, ACC, 400)],
    "sources no rule names": [(3, ACC, 80)],
    "a count of 0": [(0, FIX, 0), (1, ACC, 0), (2, ACC, 80), (3, FIX, 0)],
    "counts above the class sizes": [(0, FIX, 5000), (1, ACC, 100000), (2, ACC, 0xFFFFFFFF)],
    "an accumulate count equal to the previous one": [(0, ACC, 250), (1, ACC, 250), (2, FIX, 10), (3, ACC, 250), (4, ACC, 251)],
    "a full accumulator behind a short class": [(4, ACC, 10), (0, ACC, 10), (1, ACC, 11)],
    "any 1": [(ANY, FIX, 1)], "any cap-1": [(ANY, FIX, CAP_R - 1)], "any cap": [(ANY, FIX, CAP_R)], "any cap+1": [(ANY, FIX, CAP_R + 1)],
    "any accumulate": [(ANY, ACC, 700)],
}


@pytest.fixture(scope="module")
def rule_case():
    return random_case(np.random.default_rng(7), 3, CAP_R, 5)


@pytest.mark.parametrize("name", list(RULES))
def test_rule_sets(ctx, rule_case, name):
    got = check(ctx, RULES[name], rule_case)
    if name == "sources no rule names":
        assert np.all(np.isin(got[2], (3, 0xFF))) and np.all(got[6] == 80)
    if name == "a count of 0":
        assert np.all(got[6] == 80) and np.all(got[2] == 2)
    if name == "any cap+1":
        assert got[0].shape == (3, CAP_R) and np.all(got[6] < CAP_R)             # (padding was dropped: fewer than cap are real)


def test_nothing_kept(ctx, rule_case):
    got = check(ctx, [(ANY, FIX, 0)], rule_case)
    assert got[0].shape == (3, 0) and got[6].tolist() == [0, 0, 0]


# ---- hostile scores -----------------------------------------------------------------------------------------------------------------

SPECIAL = np.array([0x7FF8000000000001, 0x7FF4DEADBEEF0001, 0xFFF8000000000123, 0x7FF0000000000000, 0xFFF0000000000000,
                    0x8000000000000000, 0x0000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x0010000000000000,
                    0x3FF0000000000001, 0x3FF0000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF], np.uint64).view(np.float64)
HOSTILE_RULES = ([(1, FIX, 300), (0, ACC, 500), (2, ACC, 900)], [(ANY, FIX, 1100)])


def test_all_scores_equal(ctx):
    rng = np.random.default_rng(11)
    rows, score, source, count, p64, mask, p32 = random_case(rng, 3, 2049, 3)
    score[:] = 0.75
    for rules in HOSTILE_RULES:
        got = check(ctx, rules, (rows, score, source, count, p64, mask, p32))
    # ties keep input position: the top-N of equal scores is the first N real entries
    real = [i for i in range(int(count[0])) if rows[0, i] != U64MAX][:1100]
    assert got[0][0, :len(real)].tolist() == rows[0, real].tolist()
    # equal within one source only, and equal across sources with every source's entries distinct from each other
    score2 = rng.standard_normal(score.shape)
    score2[source == 1] = -0.125
    score3 = np.broadcast_to(np.arange(2049, dtype=np.float64) // 3, score.shape).copy()
    for sc in (score2, score3):
        for rules in HOSTILE_RULES:
            check(ctx, rules, (rows, sc, source, count, p64, mask, p32))


def test_special_values_travel_as_bits(ctx):
    rng = np.random.default_rng(12)
    rows, score, source, count, p64, mask, p32 = random_case(rng, 2, 1400, 3, pad=0.02)
    score[:] = SPECIAL[rng.integers(0, SPECIAL.size, score.shape)]
    p64[:] = SPECIAL[rng.integers(0, SPECIAL.size, p64.shape)]
    f32 = np.array([0x7FC00001, 0xFFC12345, 0x7FA00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x3F800001], np.uint32).view(np.float32)
    p32[:] = f32[rng.integers(0, f32.size, p32.shape)]
    for rules in HOSTILE_RULES + ([(0, FIX, 2000), (1, FIX, 2000), (2, FIX, 2000)],):
        got = check(ctx, rules, (rows, score, source, count, p64, mask, p32), optional=True)
    # NaNs last whatever their sign and payload, -0.0 beside +0.0 in input order, both infinities at the ends
    c = int(got[6][0])
    s0 = got[1][0, :c][got[2][0, :c] == 0]
    nan = np.isnan(s0)
    assert nan.any() and not nan[:np.count_nonzero(~nan)].any() and s0[0] == np.inf
    assert {0x8000000000000000, 0} <= set(got[1].view(np.uint64)[0, :c].tolist())


def test_padding_in_the_middle_and_the_counts(ctx):
    rng = np.random.default_rng(13)
    rows, score, source, _, p64, mask, p32 = random_case(rng, 4, 1100, 4, pad=0.0)
    rows[:, 5:900:3] = U64MAX                                        # padding in the middle of every list
    rows[3] = U64MAX                                                 # request 3: padding only
    count = np.array([0, 1100, 1023, 1100], np.uint32)               # d_count[q] = 0 and = cap
    for rules in ([(0, FIX, 50), (3, ACC, 120), (1, ACC, 400)], [(ANY, FIX, 700)]):
        got = check(ctx, rules, (rows, score, source, count, p64, mask, p32))
        assert got[6][0] == 0 and got[6][3] == 0 and np.all(got[0][[0, 3]] == U64MAX) and np.all(got[2][[0, 3]] == 0xFF)
        assert np.all(got[1].view(np.uint64)[[0, 3]] == ref.NEG_INF_BITS) and np.all(got[3].view(np.uint64)[:, [0, 3]] == ref.NAN_BITS)
        assert not np.any(got[4][[0, 3]]) and not np.any(got[5].view(np.uint32)[:, [0, 3]])
        check(ctx, rules, (rows, score, source, None, p64, mask, p32))
    # a count beyond cap is cap
    big = np.array([5000, 1101, 0xFFFFFFFF, 7], np.uint32)
    check(ctx, [(ANY, FIX, 700)], (rows, score, source, big, p64, mask, p32))


# ---- behind the fan-in --------------------------------------------------------------------------------------------------------------

def test_quotas_over_a_fanin_merge(ctx):
    rng = np.random.default_rng(14)
    nq, ks = 2, (5000, 2000, 1000)
    src, seen = [], None
    for i, k in enumerate(ks):
        rows = np.empty((nq, k), np.uint64)
        for q in range(nq):
            fresh = rng.choice(1 << 30, k, replace=False).astype(np.uint64) + np.uint64(1 << 20)
            if seen is not None:
                n_old = int(0.3 * k)                                 # 30 % of a list repeats ids of the lists before it
                fresh[:n_old] = rng.choice(seen[q], n_old, replace=False)
                rng.shuffle(fresh)
            rows[q] = fresh
        sc = rng.standard_normal((nq, k))
        src.append((rows, sc if i == 1 else sc.astype(np.float32)))
        seen = rows if seen is None else np.concatenate([seen, rows], axis=1)
    rules = [(0, FIX, 600), (1, ACC, 1500), (2, ACC, 2000)]
    m_rows, m_score, m_source, m_planes, m_mask, m_count = ctx.fanin_merge(src)
    w = fanin_ref.merge(src)
    got = ctx.candidates_trim(rules, m_rows, m_score, m_source, m_count, m_planes, m_mask)
    ref.same(got, ref.trim(rules, w[0], w[1], w[2], w[5], w[3], w[4]))
    assert got[0].shape == (nq, 2600) and np.all(got[6] == 2600)
    assert np.all(got[2][:, :600] == 0) and np.all(np.diff(got[2].astype(np.int64), axis=1) >= 0)          # quota after quota


def test_argument_errors_leave_the_context_usable(ctx):
    d = ctx.malloc(1 << 16)
    ok = [(0, FIX, 4)]

    def call(rules=ok, nq=1, cap=16, **kw):
        a = dict(d_rows=d, d_score=d, d_source=d, d_count=0, d_planes_f64=0, n_f64=0, d_source_mask=0, d_planes_f32=0, n_f32=0,
                 d_out_rows=d, d_out_score=d, d_out_source=d, d_out_planes_f64=0, d_out_source_mask=0, d_out_planes_f32=0, d_out_count=d)
        a.update(kw)
        ctx.candidates_trim_dev(rules, nq, cap, **a)

    refused = [dict(rules=[]), dict(rules=[(0, ACC, 5), (1, ACC, 4)]), dict(rules=[(0, FIX, 1), (0, FIX, 1)]),
               dict(rules=[(ANY, FIX, 1), (1, FIX, 1)]), dict(rules=[(8, FIX, 1)]), dict(rules=[(0, 7, 1)]),
               dict(rules=[(s % 8, FIX, 1) for s in range(9)]), dict(nq=0), dict(nq=257), dict(cap=0), dict(cap=16385),
               dict(d_rows=0), dict(d_score=0), dict(d_out_rows=0), dict(d_out_score=0), dict(d_out_count=0),
               dict(d_source=0, d_out_source=0), dict(d_out_source=0), dict(rules=[(ANY, FIX, 3)], d_source=0),
               dict(d_planes_f64=d, n_f64=1), dict(d_planes_f64=d, d_out_planes_f64=d, n_f64=0), dict(d_planes_f64=d, d_out_planes_f64=d, n_f64=9),
               dict(d_planes_f32=d, d_out_planes_f32=d, n_f32=9), dict(d_out_planes_f32=d, n_f32=1), dict(d_source_mask=d), dict(d_out_source_mask=d)]
    for kw in refused:
        with pytest.raises(PgError) as ei:
            call(**kw)
        assert ei.value.code in (-1, -4) and "pg_candidates_trim_dev" in str(ei.value), kw
    # what the checks of the candidate lists answer, code and text (recorded from the build before cand_lists.hpp stated them once)
    for kw, code, text in ((dict(d_out_source=0), -1, "d_source / d_source_mask and their outputs come in pairs"),
                           (dict(d_source_mask=d), -1, "d_source / d_source_mask and their outputs come in pairs"),
                           (dict(d_planes_f64=d, n_f64=1), -1, "a carried plane set and its output come in pairs"),
                           (dict(d_planes_f64=d, d_out_planes_f64=d, n_f64=0), -1, "a carried plane set holds 1..8 planes"),
                           (dict(d_planes_f64=d, d_out_planes_f64=d, n_f64=9), -1, "a carried plane set holds 1..8 planes"),
                           (dict(d_rows=0), -1, "NULL argument"), (dict(nq=0), -1, "nq=0 must be in [1,256]"),
                           (dict(cap=0), -4, "cap=0 unsupported (1..16384)")):
        with pytest.raises(PgError) as ei:
            call(**kw)
        assert ei.value.code == code and str(ei.value).endswith(": pg_candidates_trim_dev: " + text), kw
    ctx.free(d)
    check(ctx, ok, random_case(np.random.default_rng(15), 2, 16, 2))


# ---- the cascade --------------------------------------------------------------------------------------------------------------------

N, DIM = 20000, 128
E_COARSE = "${coarse}*(1+${current_score})^0.1"
E_FINE = "${fine}*(1+${current_score})^0.1+0.5*${coarse}"


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(ctx):
    s = Scene()
    s.t = pa.Table(ctx, N, DIM)
    s.t.fill_synthetic(o.SEED_TABLE)
    s.users = o.synth_rows(o.SEED_QUERY, 3, 3, DIM)
    wc = o.Dnn3Weights(h1=128, h2=128, seed=o.SEED_WEIGHTS ^ 0x77)
    wf = o.Dnn3Weights()
    s.coarse = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_F32, pa.pack_dnn3(wc.w1, wc.b1, wc.w2, wc.b2, wc.w3, wc.b3, 128))
    s.fine = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_F32, pa.pack_dnn3(wf.w1, wf.b1, wf.w2, wf.b2, wf.w3, wf.b3, 128))
    yield s
    s.fine.destroy()
    s.coarse.destroy()
    s.t.destroy()


def candidates(nq, cap):
    """distinct rows of the table per request, recall scores in [0, 1), padding in the middle and behind the counts"""
    rng = np.random.default_rng(cap + nq)
    rows = np.stack([rng.permutation(N)[:cap] for _ in range(nq)]).astype(np.uint64)
    rows[:, 7:cap:41] = U64MAX
    score = rng.random((nq, cap))
    source = rng.integers(0, 3, (nq, cap)).astype(np.uint8)
    count = np.array([cap, cap - 5, cap - 300][:nq], np.uint32)
    return rows, score, source, count


@pytest.mark.parametrize("nq", [1, 3])
@pytest.mark.parametrize("cap,n_keep", [(1500, 400), (1025, 1025)])
def test_cascade_equals_its_stages_one_by_one(ctx, scene, nq, cap, n_keep):
    rows, score, source, count = candidates(nq, cap)
    users = scene.users[:nq]
    ec, ef = pa.Expr(E_COARSE), pa.Expr(E_FINE)
    got = pa.recommend_cascade_dnn3(ctx, scene.t, scene.coarse, ec, "coarse", scene.fine, ef, "fine", users, rows, score, n_keep, source, count)
    g_rows, g_cfused, g_crank, g_source, g_frank, g_fused, g_order, g_count = got
    # the coarse half alone, then the reference's cut over its outputs
    rk, fu, _ = pa.recommend_candidates_dnn3(ctx, scene.t, scene.coarse, ec, "coarse", users, rows, score, count)
    ec.free()
    ef.free()
    w = ref.trim([(ANY, FIX, n_keep)], rows, fu, source, count, None, None, rk[None])
    ref.same((g_rows, g_cfused, g_source, None, None, g_crank[None], g_count), w)
    ast = o.expr_parse(E_FINE)
    for q in range(nq):
        c = int(g_count[q])
        assert c == min(n_keep, np.count_nonzero(rows[q, :int(count[q])] != U64MAX))
        # PREC_F32: the fine model's scores of pg_rank_dnn3 on the surviving rows, bit for bit; padding slots 0 / NaN
        fr = scene.fine.rank_dnn3(scene.t, users[q:q + 1], g_rows[q, :c].astype(np.uint32), np.array([0, c], np.uint32))
        assert np.array_equal(g_frank[q, :c].view(np.uint32), fr.view(np.uint32))
        assert np.all(g_frank[q, c:].view(np.uint32) == 0) and np.all(g_fused[q, c:].view(np.uint64) == ref.NAN_BITS)
        want = np.array([o.expr_eval(ast, {"fine": float(g_frank[q, j]), "coarse": float(g_crank[q, j]), "current_score": g_cfused[q, j]}.get)
                         for j in range(c)])
        assert np.max(np.abs(g_fused[q, :c] - want)) <= FUSION_TOL
        assert np.array_equal(g_order[q, :c], o.sort_scores(g_fused[q, :c], True))
        assert sorted(g_order[q, c:].tolist()) == list(range(c, n_keep))
    if n_keep == cap:
        assert np.all(g_count < n_keep)                              # nothing cut: the padding that was dropped is behind the survivors


def test_cascade_without_source_and_without_the_fine_variable(ctx, scene):
    rows, score, source, count = candidates(3, 1500)
    ec, ef = pa.Expr(E_COARSE), pa.Expr("${current_score}+2*${coarse}")
    got = pa.recommend_cascade_dnn3(ctx, scene.t, scene.coarse, ec, "coarse", scene.fine, ef, "fine", scene.users, rows, score, 400, None, None)
    rk, fu, _ = pa.recommend_candidates_dnn3(ctx, scene.t, scene.coarse, ec, "coarse", scene.users, rows, score)
    w = ref.trim([(ANY, FIX, 400)], rows, fu, None, None, None, None, rk[None])
    assert got[3] is None
    ref.same((got[0], got[1], None, None, None, got[2][None], got[7]), w)
    assert np.all(got[7] == 400)
    want = got[1] + 2.0 * got[2].astype(np.float64)                  # (one rounding per operation on either side)
    assert np.array_equal(got[5].view(np.uint64), want.view(np.uint64))
    for q in range(3):
        assert np.array_equal(got[6][q], o.sort_scores(got[5][q], True))
    ec.free()
    ef.free()


def test_cascade_refusals(ctx, scene):
    rows, score, source, count = candidates(3, 1500)
    ec, ef = pa.Expr(E_COARSE), pa.Expr(E_FINE)

    def run(table=scene.t, e_c=ec, e_f=ef, fine_var="fine", n_keep=400):
        return pa.recommend_cascade_dnn3(ctx, table, scene.coarse, e_c, "coarse", scene.fine, e_f, fine_var, scene.users, rows, score, n_keep,
                                         source, count)

    feats = pa.Features(ctx, N)
    feats.set_column("cat", pa.F_I32, (np.arange(N) % 4).astype(np.int32))
    v = scene.t.view(feats, "cat", "==", 1)
    with pytest.raises(PgError) as ei:
        run(table=v)
    assert ei.value.code == -4 and "view" in str(ei.value)
    zc = pa.Expr("${coarse}/(${current_score}-${current_score})")
    zf = pa.Expr("${fine}/(${coarse}-${coarse})")
    unknown = pa.Expr("${fine}+${nobody}")
    for kw in (dict(e_c=zc), dict(e_f=zf)):
        with pytest.raises(PgError) as ei:
            run(**kw)
        assert ei.value.code == -5
    for kw in (dict(fine_var="coarse"), dict(n_keep=0), dict(n_keep=1501), dict(e_f=unknown)):
        with pytest.raises(PgError) as ei:
            run(**kw)
        assert ei.value.code == -1 and "pg_recommend_cascade_dnn3_dev" in str(ei.value)
    assert np.all(run()[7] == 400)                                   # the context serves on
    for e in (ec, ef, zc, zf, unknown):
        e.free()
    v.destroy()
    feats.destroy()
