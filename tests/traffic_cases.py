"""The calls the TrafficControlSort tests share (test_traffic_cpu.py against the host statement, test_gpu_traffic.py against the
kernels): each case is a dict of pg_traffic_sort_host's arguments — targets, ctx_size, page_no, gamma, beta, eta, nq, cap, score,
member, order, count, alpha — made from fixed seeds.  Lists are score-descending unless a case says otherwise, as ItemRankScore
leaves them."""
import numpy as np

import traffic_ref as ref

P, Q = ref.PERCENT, ref.QUANTITY
TARGETS8 = [(11, P), (12, Q), (13, P), (14, Q), (15, P), (16, Q), (17, P), (18, Q)]


def tables(pa):
    """the library's four tables as a traffic_ref.Tables"""
    return ref.Tables(*[pa.traffic_table(w) for w in range(4)])


def scores_desc(rng, nq, cap, lo=0.001, hi=1.0):
    return -np.sort(-rng.uniform(lo, hi, (nq, cap)), axis=1)


def members(rng, nq, cap, T, p=0.4):
    m = np.zeros((nq, cap), np.uint8)
    for t in range(T):
        m |= (rng.random((nq, cap)) < p).astype(np.uint8) << t
    return m


def case(targets, nq, cap, score, member, alpha, ctx_size=10, page_no=1, gamma=1.0, beta=1.0, eta=1.6, order=None, count=None):
    T = len(targets)
    return dict(targets=list(targets), ctx_size=ctx_size, page_no=page_no, gamma=gamma, beta=beta, eta=eta, nq=nq, cap=cap,
                score=None if score is None else np.ascontiguousarray(score, np.float64).reshape(nq, cap),
                member=None if member is None else np.ascontiguousarray(member, np.uint8).reshape(nq, cap),
                alpha=None if alpha is None else np.ascontiguousarray(alpha, np.float64).reshape(nq, T),
                order=None if order is None else np.ascontiguousarray(order, np.uint32).reshape(nq, cap),
                count=None if count is None else np.ascontiguousarray(count, np.uint32).reshape(nq))


ALPHA_MIXES = {
    # name → alphas of up to 8 targets (a call takes the first T)
    "zero": [0.0] * 8,
    "negative": [-3.0, -0.5, -40.0, -1.25, -7.0, -0.01, -2.0, -300.0],
    "positive": [2.5, 0.4, 30.0, 1.0, 0.75, 12.0, 0.05, 3.0],
    "mixed": [4.0, -6.0, 0.0, 0.9, -0.3, 25.0, 0.0, -15.0],
}


def alpha_rows(name, nq, T):
    return np.tile(np.asarray(ALPHA_MIXES[name][:T], np.float64), (nq, 1))


def lengths_case(lengths, T, mix, seed, cap=None, order=False, page_no=1, ctx_size=10, eta=1.6, zero_middle=False):
    """one call whose requests have the given list lengths (ragged counts); order: a permutation of every request's elements"""
    rng = np.random.default_rng(seed)
    nq = len(lengths)
    cap = cap or max(max(lengths), 1)
    sc = scores_desc(rng, nq, cap)
    mem = members(rng, nq, cap, T)
    al = alpha_rows(mix, nq, T)
    if zero_middle and nq >= 3:
        al[nq // 2] = 0.0
    ordr = None
    if order:
        ordr = np.stack([rng.permutation(cap) for _ in range(nq)]).astype(np.uint32)
        # the list is score-descending: element order[q][j] carries the j-th score
        s2, m2 = np.empty_like(sc), np.empty_like(mem)
        for q in range(nq):
            s2[q, ordr[q]] = sc[q]
            m2[q, ordr[q]] = mem[q]
        sc, mem = s2, m2
    return case(TARGETS8[:T], nq, cap, sc, mem, al, ctx_size=ctx_size, page_no=page_no, eta=eta, order=ordr,
                count=np.asarray(lengths, np.uint32))


def hostile_case(T=8, nq=4, cap=70, seed=99):
    """NaN and +-Inf scores and alphas, zero scores, negative scores, -0.0, a NaN and an infinite maxScore: pins goint, the wrapping
    arithmetic and the NaN-last order (zero_total_cases adds the +-Inf and NaN weights)"""
    rng = np.random.default_rng(seed)
    sc = scores_desc(rng, nq, cap)
    mem = members(rng, nq, cap, T, 0.6)
    al = np.tile(np.asarray(ALPHA_MIXES["mixed"][:T], np.float64), (nq, 1))
    specials = [np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 1e308, -1e308, 5e-324]
    for q in range(nq):
        for k, v in enumerate(specials):
            sc[q, (7 * k + 3 * q) % cap] = v
    sc[1, 0] = np.nan                       # maxScore NaN: every s / maxScore is NaN, goint gives INT64_MIN
    sc[2, 0] = np.inf
    sc[3, :] = 0.0                          # every s_i is 1e-8
    sc[3, 1] = -0.0
    al[0, 0], al[0, 1 % T] = np.nan, np.inf
    al[1, 0] = -np.inf
    if T > 2:
        al[2, 2] = 1e300
    c = case(TARGETS8[:T], nq, cap, sc, mem, al, ctx_size=5, page_no=2, eta=0.01)
    return c


def zero_total_cases(tabs):
    """scores that make `total` exactly 0.0: s_0 = positionWeight[1] (the library's), s_1 = -1.0, so w_0 + w_1 = 0; weight_t =
    sum_t / total is then +Inf (members {0}), NaN ({0, 1}) and -Inf ({1}) — step 4's division as written — and steps 2, 5, 6 and 8
    see goint(NaN), goint(+-Inf) and NaN positions"""
    sc = np.array([[tabs.pos[1], -1.0]])
    mem = np.array([[0b011, 0b110]], np.uint8)
    cases = []
    for alpha in ([2.0, -3.0, 1.5], [-2.0, 3.0, -1.5], [0.5, 0.0, 4.0]):
        for page_no in (1, 2):
            for types in ((P, Q, P), (Q, P, Q)):
                cases.append(case([(5, types[0]), (6, types[1]), (7, types[2])], 1, 2, sc, mem, [alpha], ctx_size=1, page_no=page_no))
    return cases


def random_cases(n_cases, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_cases):
        T = int(rng.integers(0, 9))
        nq = int(rng.integers(1, 4))
        cap = int(rng.integers(1, 48))
        sc = scores_desc(rng, nq, cap, -0.2 if rng.random() < 0.2 else 0.001, float(rng.choice([1.0, 50.0, 1e-3])))
        if rng.random() < 0.3:
            sc = np.round(sc, 1)            # equal runs and exact zeros
        if rng.random() < 0.2:
            sc[:, 0] = sc[:, 0] * 0.5       # a first score that is not the maximum
        mem = members(rng, nq, cap, max(T, 1), float(rng.choice([0.1, 0.5, 0.9])))
        al = rng.choice([0.0, 0.0, 1.0, -1.0, 3.5, -8.0, 0.3, 40.0, -0.02], (nq, T)) * rng.uniform(0.5, 1.5, (nq, T))
        if rng.random() < 0.1 and T:
            al[0, 0] = rng.choice([np.nan, np.inf, -np.inf])
        if rng.random() < 0.1:
            sc[0, int(rng.integers(0, cap))] = rng.choice([np.nan, np.inf, -np.inf, 0.0])
        order = count = None
        if rng.random() < 0.5:
            order = np.stack([rng.permutation(cap) for _ in range(nq)]).astype(np.uint32)
        if rng.random() < 0.5:
            count = rng.integers(0, cap + 3, nq).astype(np.uint32)
        targets = [(int(rng.integers(-50, 1000)), int(rng.choice([P, Q]))) for _ in range(T)]
        out.append(case(targets, nq, cap, sc if T else None, mem if T else None, al if T else None, ctx_size=int(rng.integers(1, 60)),
                        page_no=int(rng.integers(1, 4)), gamma=float(rng.choice([1.0, 0.0, 2.5, -1.0])), beta=float(rng.choice([1.0, 0.1, 7.0])),
                        eta=float(rng.choice([1.6, 0.01, 0.2])), order=order, count=count))
    return out


def expect(tabs, c):
    """traffic_ref's answer to a case"""
    return ref.traffic_sort(tabs, c["targets"], c["ctx_size"], c["nq"], c["cap"], score=c["score"], member=c["member"], order=c["order"],
                            count=c["count"], alpha=c["alpha"], page_no=c["page_no"], gamma=c["gamma"], beta=c["beta"], eta=c["eta"])


def same_bits(got, want, what=""):
    """order, count, control ids and new_pos (as uint64) are equal"""
    names = ("out_order", "out_count", "control_id", "new_pos")
    for name, g, w in zip(names, got, want):
        if g is None:
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        if name == "new_pos":
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            raise AssertionError("%s: %s differs at %s: got %r, expected %r" % (what, name, tuple(at), g[tuple(at)], w[tuple(at)]))
