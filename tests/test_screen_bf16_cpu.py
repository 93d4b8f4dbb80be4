"""The bf16 screen's bound on the CPU (no GPU): on every fixture that test_gpu_screen_bf16.py runs, for every query that does not
stand aside and every row,

    |x^.q^ - fl(x.q)| + gamma_d sum|x^_i q^_i|  <=  eps_unit_q * max(sqrt(blk_norm2), 1e-16) * 1.0002

(x^, q^ the bf16 operands, x^.q^ in fp64, fl(x.q) the specification's fp32 fmaf chain, gamma_d the fp32 accumulation of the matrix
pipe in whatever order it uses), no top-K member is cut by the modelled rule, and the fixtures marked sharp lose members as soon as
a block is screened with its neighbour's norm."""
import functools

import numpy as np
import pytest

import screen_bf16_ref as ref
import table_derived_ref
from oracle import oracle as o

F = np.float32
DIMS = (64, 128)
NQ_CHECKED = 8                   # queries of the big fixtures that the bound is checked on (the sharp ones lead)


@functools.lru_cache(maxsize=None)
def case(name, dim):
    """(table, queries, K) of a fixture; the queries limited to the ones checked here"""
    if name == "sharp":
        fx = ref.Sharp(dim)
        return fx.tab, fx.q[:NQ_CHECKED], ref.Sharp.K
    if name.startswith("ragged"):
        fx = ref.Sharp(dim, rows=ref.ragged_rows(int(name[6:])))
        return fx.tab, fx.q[:4], ref.Sharp.K
    if name == "planted":
        tab, q, _ = ref.planted(dim)
        return tab, q[::23], 32
    if name == "hostile":
        tab, q = ref.hostile(dim, 72)
        return tab, q[:24], 300
    if name.startswith("guard"):
        tab, q, _, _ = ref.guard_tables(dim)[int(name[5:])]
        return tab, q, 100
    if name in ref.SUBNORMAL_M:
        tab, q = ref.subnormal(dim, ref.SUBNORMAL_M[name])
        return tab, q, 16
    raise KeyError(name)


CASES = ["sharp", "ragged1", "ragged31", "planted", "hostile", "guard0", "guard1", "subnormal", "smallest_normal"]


@functools.lru_cache(maxsize=None)
def modelled(name, dim):
    """per query: (stands aside, eps_unit, K-th score, members, exact scores, acc, sum|x^ q^|), and the block norms"""
    tab, q, k = case(name, dim)
    xh, qh = ref.bf16_rne(tab), ref.bf16_rne(q)
    norm2 = ref.blk_norm2(tab)
    eu = ref.eps_unit(q)
    exact = o.dot_scores(tab, q)                                  # [nq][rows], the fp32 fmaf chain
    orow, osc = o.recall_topk(tab, q, k)
    with np.errstate(over="ignore", invalid="ignore"):
        acc = (xh.astype(np.float64) @ qh.astype(np.float64).T).T
        mag = (np.abs(xh).astype(np.float64) @ np.abs(qh).astype(np.float64).T).T
    aside = ref.stands_aside(osc[:, -1], eu, ref.max_norm_of(norm2))
    return norm2, [(bool(aside[i]), eu[i], osc[i, -1], orow[i].astype(np.int64), exact[i], acc[i], mag[i]) for i in range(len(q))]


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("name", CASES)
def test_the_bound_the_kernel_relies_on_holds_for_every_row(name, dim):
    norm2, per_query = modelled(name, dim)
    nb = np.repeat(ref.norm_used(norm2).astype(np.float64), ref.BLK)
    checked = 0
    for i, (aside, eu, _, _, exact, acc, mag) in enumerate(per_query):
        if aside:
            continue
        checked += 1
        lhs = np.abs(acc - exact.astype(np.float64)) + ref.gamma(dim) * mag
        rhs = float(eu) * nb[:len(lhs)]
        bad = np.flatnonzero(~(lhs <= rhs))
        assert bad.size == 0, "%s dim %d query %d row %d: error %.6g above the margin %.6g (%d rows in all)" % (
            name, dim, i, bad[0], lhs[bad[0]], rhs[bad[0]], bad.size)
    assert checked >= 2


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("name", CASES)
def test_no_member_is_cut_by_the_modelled_rule(name, dim):
    """thr = the final K-th score, the highest threshold a launch can screen against"""
    norm2, per_query = modelled(name, dim)
    for i, (aside, eu, kth, members, _, acc, _) in enumerate(per_query):
        thr_s = F(-np.inf) if aside else kth
        kept = ref.keep(acc, thr_s, eu, norm2)
        assert np.all(kept[members]), "%s dim %d query %d: %d members cut" % (name, dim, i, int((~kept[members]).sum()))


def lost_at_the_running_threshold(name, dim, queries, floor):
    """members that a screened chunk of the growing-chunk plan cuts: chunk [b, e) is screened against the K-th best of rows < b"""
    tab, q, k = case(name, dim)
    norm2, per_query = modelled(name, dim)
    lost = 0
    for b, e in ref.grow_schedule(len(tab), k)[1:]:
        _, osc = o.recall_topk(tab[:b], q[list(queries)], k)
        for n, i in enumerate(queries):
            aside, eu, _, members, _, acc, _ = per_query[i]
            kept = ref.keep(acc, F(-np.inf) if aside else osc[n, -1], eu, norm2, floor=floor)
            lost += int((~kept[members[(members >= b) & (members < e)]]).sum())
    return lost


@pytest.mark.parametrize("dim", DIMS)
def test_blocks_whose_sum_of_squares_underflows_need_the_floor(dim, capsys):
    """The fixtures of (f) and (i) are sharp for the floor under the block norm: at the thresholds the growing-chunk plan screens
    with, the rule without the floor cuts members, the kernel's rule none."""
    lines = []
    for name, queries in (("hostile", (ref.TINY_SHARP,)), ("subnormal", (0,)), ("smallest_normal", (0,))):
        with_floor = lost_at_the_running_threshold(name, dim, queries, True)
        without = lost_at_the_running_threshold(name, dim, queries, False)
        lines.append("dim %d %s: members lost at the running thresholds — with the floor %d, without %d" % (dim, name, with_floor, without))
        assert with_floor == 0 and without >= 1, lines[-1]
    assert ref.grow_schedule(60_003, 300)[-1] == (32768, 60_003) and (8192, 16384) in ref.grow_schedule(20_000, 16)
    with capsys.disabled():
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("dim", DIMS)
def test_sharp_fixture_loses_members_under_a_neighbours_norm(dim, capsys):
    norm2, per_query = modelled("sharp", dim)
    lines = []
    for i in ref.Sharp.SHARP:
        aside, eu, kth, members, _, acc, _ = per_query[i]
        assert not aside
        lost = {v: int((~ref.keep(acc, kth, eu, norm2, v)[members]).sum()) for v in (0, -1, +1)}
        lines.append("dim %d sharp query %d: members lost of %d — own norm %d, block b-1's %d, block b+1's %d" % (
            dim, i, len(members), lost[0], lost[-1], lost[1]))
        assert lost[0] == 0 and lost[-1] >= 1 and lost[1] >= 1, lines[-1]
    with capsys.disabled():
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("dim", DIMS)
def test_members_of_a_sharp_query_sit_in_loud_blocks_with_the_last_row_on_top(dim):
    for name in ("sharp", "ragged1", "ragged31"):
        tab, _, _ = case(name, dim)
        _, per_query = modelled(name, dim)
        for i in ref.Sharp.SHARP:
            members = per_query[i][3]
            assert np.all((members // ref.BLK) % 3 == i), (name, i)
        owner = (ref.blocks_of(len(tab)) - 1) % 3
        assert owner == (1 if name == "sharp" else 0)
        assert per_query[owner][3][0] == len(tab) - 1             # (b): the last row of the last block is its sharp query's best


def test_every_fixture_is_routed_to_the_bf16_shadow():
    """ensure_table_stats keeps a dim-128 table on the int8 shadow unless its largest element is far above the typical row: every
    fixture, and the rows the filter of (h) admits, must leave it (dim 64 has no other shadow)"""
    for name in CASES:
        assert table_derived_ref.route(case(name, 128)[0]) == 2, name
    fx = ref.Sharp(128)
    assert table_derived_ref.route(fx.tab[fx.flag == 1]) == 2
    assert table_derived_ref.route(ref.Sharp(128, seed=8).tab) == 2


def test_guards_fall_on_the_side_the_fixture_says():
    """screen_thr_kernel: e > 1e28 and e * max_norm >= 1e35, approached from both sides; a guard that moved is noticed here"""
    for dim in DIMS:
        for t, (tab, q, active, aside) in enumerate(ref.guard_tables(dim)):
            _, per_query = modelled("guard%d" % t, dim)
            got = [p[0] for p in per_query]
            assert [i for i, a in enumerate(got) if a] == sorted(aside), (dim, t, got)
            eu = ref.eps_unit(q)
            mn = ref.max_norm_of(ref.blk_norm2(tab))
            for i in active:                                      # close to the guard, on the screened side
                assert (eu[i] > 5e27 and t == 0) or (float(eu[i]) * float(mn) > 5e34 and t == 1)
    # NaN / inf queries and thresholds stand aside, ordinary ones do not
    eu = ref.eps_unit(np.array([[1.0, 2.0], [np.nan, 0.0], [np.inf, 0.0], [3e38, 3e38]], dtype=F))
    assert ref.stands_aside(np.zeros(4, F), eu, F(1.0)).tolist() == [False, True, True, True]
    assert ref.stands_aside(np.array([np.nan, -np.inf], F), eu[:1].repeat(2), F(1.0)).tolist() == [True, False]


def test_bf16_rounding_and_the_cut_round_down():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.4e38, 0.0, -0.0, 1e-40], dtype=F)
    want = np.array([1.0, 1.0, 1.015625, -1.0, np.inf, 0.0, -0.0, 1e-40], dtype=F)
    got = ref.bf16_rne(x)
    assert np.array_equal(got[:7].view(np.uint32), want[:7].view(np.uint32))       # ties to even, overflow to inf, signed zeros
    assert abs(float(got[7]) - 1e-40) <= 2.0 ** -134                                # bf16 subnormals: an absolute step of 2^-133
    nan = np.array([0x7F800001, 0xFFC12345], dtype=np.uint32).view(F)
    assert np.all(np.isnan(ref.bf16_rne(nan)))
    for thr in (1.0, -1.0, 0.0, 1e30, -1e-30):
        c = ref.cut_of(F(thr), F(0.0), np.ones(1, F))
        assert c[0] < F(thr)                                                        # strictly below, also at zero
    assert ref.cut_of(F(-np.inf), F(1.0), np.ones(1, F))[0] == -np.inf
    assert ref.cut_of(F(np.inf), F(0.0), np.ones(1, F))[0] == np.inf                # an inactive column is never a suspect


def test_largest_relative_error_stays_under_the_analytic_ceiling(capsys):
    """|x^.q^ - x.q| / (||x|| ||q||) over every fixture whose operands are normal numbers: the ceiling is 2 x 2^-9 + 2^-18 ~ 0.0039
    against the code's 0.008.  (The fixtures with subnormal components are left out: below 2^-126 a bf16 keeps an absolute 2^-134,
    not a relative 2^-9 — they are what the floor under the block norm is for.)"""
    worst = (0.0, "")
    for name in CASES[:7]:
        for dim in DIMS:
            tab, q, _ = case(name, dim)
            _, per_query = modelled(name, dim)
            x64 = tab.astype(np.float64)
            xn = np.sqrt((x64 ** 2).sum(axis=1))
            ok = xn > 0
            true = (x64 @ q.astype(np.float64).T).T
            for i, (aside, _, _, _, _, acc, _) in enumerate(per_query):
                qn = float(np.sqrt((q[i].astype(np.float64) ** 2).sum()))
                if aside or qn == 0.0:
                    continue
                r = float((np.abs(acc - true[i])[ok] / (xn[ok] * qn)).max())
                if r > worst[0]:
                    worst = (r, "%s dim %d query %d" % (name, dim, i))
    with capsys.disabled():
        print("\nlargest |x^.q^ - x.q| / (||x|| ||q||) over the fixtures: %.6f (%s)" % worst)
    assert 0.0 < worst[0] <= 0.0039
