"""CPU tests of the inputs tests/test_gpu_dpp_greedy.py runs on the device: two references that share no code
(oracle/oracle.c:dpp_once and the hand model of tests/dpp_ref.py) agree on every exact rank-deficient page, and each
page is on the path it exists for — the `dj < epsilon` break and the fill by index (dpp_sort.go:517, :539-548),
exhausted windows, first-maximum ties — so that the GPU cases cannot drift off it when a generator changes."""
import numpy as np
import pytest

import dpp_ref as ref
from oracle import oracle as o


def oracle_hook_picks(hook, topn, window):
    F = o.dpp_features(None, hook, False, False)
    L = o.dpp_kernel_matrix_f(F, np.zeros(hook.shape[0]), 0.0)
    with np.errstate(all="ignore"):
        return o.dpp_with_window(L, topn, window).tolist()


def hook_id(c):
    return "%dx%d-top%d-w%d" % (c[0], c[1], c[2], c[3])


def tie_id(c):
    return "%d-%s-w%d" % (c[0], "_".join(map(str, c[2])) or "all", c[4])


@pytest.mark.parametrize("case", ref.HOOK_CASES, ids=hook_id)
def test_hand_model_equals_oracle_on_exact_pages(case):
    hook, kinds, exps, topn, window = ref.hook_case(case)
    n, h = hook.shape
    # the construction: one power of two per row at most, distinct exponents within +-h/2
    assert ((hook != 0).sum(axis=1) <= 1).all()
    assert len(set(exps.tolist())) == h and max(abs(int(e)) for e in exps) <= h / 2
    nz = hook[hook != 0]
    assert np.array_equal(np.exp2(np.round(np.log2(nz))), nz)
    trace = []
    hand = ref.greedy_by_hand(kinds, exps, topn, window, trace)
    assert hand == oracle_hook_picks(hook, topn, window)
    assert ref.kernel_of(n, window) == case[5]
    filled = ref.filled_windows(hand, n, trace)
    what = case[6]
    if what == "single":                     # one item: the window has one pick, nothing to break out of or to fill
        assert hand == [0] and n == 1
        return
    if what == "exhausted":                  # windows with nothing left: item 0 repeated, or fewer picks than asked for
        assert len(hand) < topn or len(set(hand)) < len(hand)
        assert trace[-1]["greedy"] == trace[-1]["len"] or trace[-1]["len"] < ref.windows_of(n, topn, window)[-1]
    if what == "every window":
        assert filled == list(range(len(trace))) and len(trace) >= 3
    if n > 5:
        assert filled, "no window of this case breaks and fills"
    for w in filled:
        assert trace[w]["greedy"] < min(window, ref.windows_of(n, topn, window)[w])


def test_the_five_item_page_returns_nineteen_of_twenty():
    """(n 5, topn 20, window 3): three picks, two (the window breaks with nothing left to fill), then windows over NaN
    alone that append item 0 — both references count 19."""
    hook, kinds, exps, topn, window = ref.hook_case(ref.HOOK_CASES[5])
    assert (hook.shape[0], topn, window) == (5, 20, 3)
    hand = ref.greedy_by_hand(kinds, exps, topn, window)
    assert len(hand) == 19 and sorted(hand[:5]) == [0, 1, 2, 3, 4] and hand[5:] == [0] * 14
    assert hand == oracle_hook_picks(hook, topn, window)


@pytest.mark.parametrize("case", ref.TIE_CASES, ids=tie_id)
def test_hand_model_equals_oracle_on_ties(case):
    hook, kinds, exps, topn, window = ref.tie_case(case)
    n, top = case[0], case[2]
    trace = []
    hand = ref.greedy_by_hand(kinds, exps, topn, window, trace)
    assert hand == oracle_hook_picks(hook, topn, window)
    assert ref.kernel_of(n, window) == case[6]
    # the tied maxima come out lowest index first, then the first occurrence of every other column, ascending
    assert hand[:len(top)] == sorted(top)
    firsts = sorted(int(np.nonzero(kinds == k)[0][0]) for k in range(len(top), hook.shape[1]) if (kinds == k).any())
    assert hand[len(top):len(top) + len(firsts)] == firsts
    assert len(top) + len(firsts) < window
    assert ref.filled_windows(hand, n, trace), "no window of this case breaks and fills"


@pytest.mark.parametrize("case", ref.DUP_CASES, ids=lambda c: "%dof%d-d%d-w%d" % (c[0], c[1], c[2], c[4]))
@pytest.mark.parametrize("hook_dim", [0, 5])
def test_duplicate_rows_break_and_fill_in_every_window(case, hook_dim):
    n, m, d, topn, window = case[:5]
    tab, cand, rel, hook = ref.dup_case(case, hook_dim=hook_dim)
    assert len(set(cand.tolist())) == m < window
    F = o.dpp_features(tab[cand], hook, True, True)
    with np.errstate(all="ignore"):
        want = o.dpp_with_window(o.dpp_kernel_matrix_f(F, rel, 0.0), topn, window).tolist()
    assert len(want) == min(topn, n)
    ref.check_duplicates_fill_every_window(want, cand, topn, window)
    assert ref.kernel_of(n, window) == case[5]


def test_the_edge_cases_hold_every_dispatch_boundary():
    have = {(n, w): ref.kernel_of(n, w) for n, w, _ in ref.EDGE_CASES}
    for key, kind in ref.BOUNDARIES.items():
        assert have[key] == kind
    assert {w for _, w, _ in ref.EDGE_CASES} >= {0, 1, 11, 13, 16, 17}
    assert {n for n, _, _ in ref.EDGE_CASES} == {1, 2, 63, 64, 65, 512, 513, 1024, 1025}
