"""A second reference for DPPSort's greedy MAP inference (sort/dpp_sort.go:477-551) that shares nothing with
oracle/oracle.c: inputs on which the whole computation is exact, and the pick sequence worked out from their structure.

The inputs are hook embeddings whose row i is all zero or 2**e_k in ONE column k.  Fed to KernelMatrix without a table,
without normalisation, without EnsurePositiveSim and with alpha = 0 they give F = [hook, 0] and r = 1, so
    L_ij = 4**e_k  when i and j sit in the same column k,  0  otherwise
and every product, square root and quotient of the greedy update is a power of two or zero: nothing rounds, on any
machine.  Picking j of column k gives e_n = L_jn / sqrt(d2_j) = 2**e_k for the items of column k and 0 elsewhere, so
d2_n - e_n**2 is exactly 0 for column k and unchanged for every other item; the correction <c_j, c_n> of the later picks
is a sum of products with a zero factor.  A window therefore picks the columns by descending exponent (first index
first), every item of a picked column ties at 0 with the zero rows, and the pick after the last live column has
d2 = 0 < 1e-10: the loop breaks and the window is filled by ascending unused index.

This file holds generators and the hand model only; it calls neither the oracle nor the device."""
import numpy as np

EPSILON = 1e-10          # dpp_sort.go:494


def hooks_of(kinds, exps, h):
    """The embedding rows of a structure: kinds[i] = the column of item i, or -1 for a zero row; exps[k] = column k's
    exponent.  [n][h] fp64."""
    hook = np.zeros((len(kinds), h))
    for i, k in enumerate(kinds):
        if k >= 0:
            hook[i, k] = 2.0 ** int(exps[k])
    return hook


def exact_hooks(n, h, seed):
    """n rows over h columns: a row is zero with probability 1 / (h + 1), otherwise it sits in a random column.  The
    columns' exponents are distinct and lie within +-h/2.  -> (hook [n][h] fp64, kinds [n], exps [h])"""
    rng = np.random.default_rng(seed)
    exps = rng.permutation(np.arange(h) - h // 2)
    kinds = rng.integers(-1, h, n)
    return hooks_of(kinds, exps, h), kinds, exps


def tie_hooks(n, h, top, seed):
    """Ties: the items `top` each sit in a column of their own, all with exponent +2; every other item is a zero row or
    sits in one of h further columns that share the exponent -1.  The maxima of every argmax are equal values in
    different lanes and element slots.  -> (hook [n][len(top) + h], kinds, exps)"""
    rng = np.random.default_rng(seed)
    t = len(top)
    exps = np.array([2] * t + [-1] * h)
    kinds = rng.integers(-1, h, n)
    kinds[kinds >= 0] += t
    for c, i in enumerate(top):
        kinds[i] = c
    return hooks_of(kinds, exps, t + h), kinds, exps


def greedy_by_hand(kinds, exps, topn, window, trace=None):
    """DPPWithWindow's pick sequence on hooks_of(kinds, exps), from the structure alone (window >= 1: the default of 10
    for 0 belongs to the caller).  -> list of picks; its length is the count.  `trace`, a list, receives per window
    {"start", "greedy", "len", "broke"}: where the window begins in the result, how many of its picks the argmax made,
    how many picks it has, whether it left the loop through the epsilon test."""
    n = len(kinds)
    result = []

    def once(t):
        t = min(t, n)
        if t == 0:
            return
        start = len(result)
        gone = set(result)                  # d2 = NaN: picked by an earlier window, or picked and processed by this one
        dead = set()                        # columns a pick of this window has zeroed
        state = {"poisoned": False}         # an all-NaN argmax picked item 0 with d2 = NaN: every d2 is NaN from there

        def value(i):
            if state["poisoned"] or i in gone:
                return None
            if kinds[i] < 0 or kinds[i] in dead:
                return 0.0
            return 4.0 ** int(exps[kinds[i]])

        def max_idx():                      # floats.MaxIdx: first maximum, NaN skipped, nothing left -> index 0 (d2 = NaN)
            best, bv = 0, None
            for i in range(n):
                v = value(i)
                if v is not None and (bv is None or v > bv):
                    best, bv = i, v
            return best, bv

        Y = []
        j, dj = max_idx()
        Y.append(j)
        broke = False
        while len(Y) < t:
            if dj is not None and dj < EPSILON:
                broke = True
                break
            if dj is None:
                state["poisoned"] = True
            else:
                dead.add(kinds[j])
            gone.add(j)
            j, dj = max_idx()
            Y.append(j)
        greedy = len(Y)
        if len(Y) < t:
            for i in range(n):
                if i not in gone and i not in Y:
                    Y.append(i)
                    if len(Y) == t:
                        break
        if trace is not None:
            trace.append({"start": start, "greedy": greedy, "len": len(Y), "broke": broke})
        result.extend(Y)

    if topn <= window:
        once(topn)
    else:
        for _ in range(topn // window):
            once(window)
        if topn % window:
            once(topn % window)
    return result


def filled_windows(seq, n, trace):
    """The windows of `trace` that ran break-and-fill with something to fill, checked on the sequence itself: the window
    left the loop through the epsilon test after fewer picks than it has, and the rest of it is the ascending run of the
    indices that nothing before had used."""
    out = []
    for w, t in enumerate(trace):
        if not t["broke"] or t["greedy"] >= t["len"]:
            continue
        cut = t["start"] + t["greedy"]
        used = set(seq[:cut])
        want = [i for i in range(n) if i not in used][:t["len"] - t["greedy"]]
        assert list(seq[cut:t["start"] + t["len"]]) == want, (w, t)
        out.append(w)
    return out


# ---- the cases both test files use -------------------------------------------------------------------------------
WAVE8, WAVE16, BLOCK = "dpp_wave8_calls", "dpp_wave16_calls", "dpp_block_calls"


def kernel_of(n, window):
    """dpp_run_locked's rule, restated (csrc/dpp.hip; window 0 -> 10 first)"""
    window = window or 10
    if n <= 512 and window <= 16:
        return WAVE8
    if n <= 1024 and window <= 10:
        return WAVE16
    return BLOCK


#   n, h, topn, window, seed, kernel, what the case must show besides the equal sequences
HOOK_CASES = [
    (200, 6, 40, 10, 1, WAVE8, "fill"),
    (200, 6, 16, 16, 2, WAVE8, "fill"),                  # topn = window = 16: one window, LDS rows for 16 picks
    (513, 5, 30, 10, 3, WAVE16, "fill"),
    (600, 7, 40, 20, 4, BLOCK, "fill"),
    (1100, 4, 25, 10, 5, BLOCK, "fill"),
    (5, 2, 20, 3, 6, WAVE8, "exhausted"),                # 19 of 20: item 0 again and again once nothing is left
    (1, 1, 4, 10, 7, WAVE8, "single"),                   # one item: one pick, no loop
    (63, 3, 63, 10, 8, WAVE8, "fill"),                   # every item picked, lanes without an item
    (65, 70, 65, 13, 9, WAVE8, "fill"),                  # thirteen greedy picks in the first window; columns below epsilon later
    # every window breaks: the first, the middle ones and the remainder (three columns; the remainder has six picks)
    (300, 3, 36, 10, 10, WAVE8, "every window"),
    (512, 3, 54, 16, 11, WAVE8, "every window"),
    (800, 3, 36, 10, 12, WAVE16, "every window"),
    (1024, 3, 26, 10, 13, WAVE16, "every window"),
    (600, 3, 66, 20, 14, BLOCK, "every window"),
    (1100, 3, 36, 10, 15, BLOCK, "every window"),
    (300, 3, 40, 17, 16, BLOCK, "every window"),
    # topn > n over many windows: fills first, then windows with nothing left
    (70, 3, 90, 16, 17, WAVE8, "exhausted"),
    (520, 3, 540, 10, 18, WAVE16, "exhausted"),
    (520, 3, 540, 11, 19, BLOCK, "exhausted"),
]

#   n, h, the items that hold the maximum, topn, window, seed, kernel
TIE_CASES = [
    (512, 4, (70, 6, 454), 25, 10, 21, WAVE8),           # lane 6 of element slots 1, 0 and 7
    (200, 5, (), 30, 16, 22, WAVE8),                     # every live d2 equal: first occurrences in ascending order
    (199, 4, (198,), 12, 10, 23, WAVE8),                 # the maximum in the last valid lane only
    (600, 4, (70, 6, 518), 25, 10, 24, WAVE16),          # lane 6 of element slots 1, 0 and 8
    (1000, 4, (900, 580), 25, 10, 25, WAVE16),           # lane 4 of slots 14 and 9
    (777, 4, (776,), 12, 10, 26, WAVE16),
    (600, 4, (70, 6, 518), 25, 11, 27, BLOCK),
    (1100, 4, (1099, 1030), 25, 10, 28, BLOCK),          # beyond the 1024 threads: a thread's second item
    (300, 5, (), 40, 20, 29, BLOCK),
]


#   n, window, topn — topn of 1, window - 1, window, window + 1, n and n + 7 around; both sides of every boundary
EDGE_CASES = [
    (1, 10, 1), (1, 0, 8), (1, 17, 3),
    (2, 1, 2), (2, 16, 9),
    (63, 0, 63), (63, 11, 70),
    (64, 13, 64), (64, 16, 17), (64, 17, 71),
    (65, 16, 15), (65, 13, 72), (65, 17, 18),
    (512, 16, 48), (512, 16, 519), (512, 11, 11), (512, 17, 35),
    (513, 10, 31), (513, 0, 520), (513, 1, 3), (513, 11, 23),
    (1024, 10, 41), (1024, 0, 1), (1024, 11, 12),
    (1025, 10, 30), (1025, 1, 2),
]
# the dispatch rule, from both sides of each of its boundaries
BOUNDARIES = {(512, 16): WAVE8, (512, 17): BLOCK, (513, 10): WAVE16, (513, 11): BLOCK, (1024, 10): WAVE16, (1025, 10): BLOCK}


def hook_case(case):
    n, h, topn, window, seed = case[:5]
    hook, kinds, exps = exact_hooks(n, h, seed)
    return hook, kinds, exps, topn, window


def tie_case(case):
    n, h, top, topn, window, seed = case[:6]
    hook, kinds, exps = tie_hooks(n, h, top, seed)
    return hook, kinds, exps, topn, window


#   n, m distinct rows, dim, topn, window — candidates drawn with repetition from m table rows, m < window
DUP_CASES = [
    (300, 6, 128, 40, 10, WAVE8),
    (500, 9, 128, 48, 16, WAVE8),
    (800, 5, 64, 30, 10, WAVE16),
    (1100, 7, 128, 30, 10, BLOCK),
    (40, 3, 128, 40, 10, WAVE8),
]
DUP_TABLE_ROWS = 256


def dup_case(case, seed=40, hook_dim=0):
    """-> (table [256][d] fp32, cand [n] u32 over m of its rows, relevance, hook [n][hook_dim] or None): copies of one
    table row carry copies of one hook row"""
    n, m, d = case[:3]
    rng = np.random.default_rng(seed + n)
    tab = rng.standard_normal((DUP_TABLE_ROWS, d)).astype(np.float32)
    rows = rng.choice(DUP_TABLE_ROWS, m, replace=False).astype(np.uint32)
    cand = rows[rng.integers(0, m, n)]
    cand[:m] = rows                                       # every one of the m rows occurs
    rel = np.sort(rng.random(n))[::-1].copy()
    hook = None
    if hook_dim:
        per_row = rng.standard_normal((DUP_TABLE_ROWS, hook_dim))
        hook = per_row[cand]
    return tab, cand, rel, hook


def windows_of(n, topn, window):
    """DPPWithWindow's schedule: the topN of every DPP call (before the cut at N)"""
    if topn <= window:
        return [topn]
    return [window] * (topn // window) + ([topn % window] if topn % window else [])


def check_duplicates_fill_every_window(seq, cand, topn, window):
    """Conditions that keep a duplicate-rows case on the degenerate path, on the reference sequence: in every window the
    distinct rows among the items still unused are fewer than the window; the window picks each of them once, then one
    more item, and the rest is the ascending run of unused indices."""
    n = len(cand)
    pos = 0
    for t in windows_of(n, topn, window):
        unused = [i for i in range(n) if i not in set(seq[:pos])]
        distinct = len(set(cand[unused].tolist()))
        assert distinct < window, "precondition: %d distinct rows in a window of %d" % (distinct, window)
        t = min(t, n)
        g = min(distinct + 1, t)
        greedy = list(seq[pos:pos + g])
        assert len(set(cand[greedy[:distinct]].tolist())) == min(distinct, g), "the window's first picks are not the distinct rows"
        used = set(seq[:pos + g])
        want = [i for i in range(n) if i not in used][:t - g]
        assert t - g > 0 and list(seq[pos + g:pos + t]) == want, "the window does not end in the fill"
        pos += t
    assert pos == len(seq)
