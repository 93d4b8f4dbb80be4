"""CPU tests of TrafficControlSort's macro control (include/pairec_gpu.h: pg_traffic_*).  No GPU needed.

(a) pg_traffic_table against math.exp / math.tanh: every entry equal or within 1 ulp; the literal beyond 500 and math.e exact.
(b) pg_traffic_sort_host against tests/traffic_ref.py (written from the Go) by bits — order, count, control ids, new_pos as uint64 —
    with the library's tables handed to both, on the edge lengths, T in 0 / 1 / 8, every alpha mix, both control types on one
    entry in both target orders, both pages, ctx_size on both sides of n, irregular scores, a permuted order with ragged counts,
    hostile values, and a few hundred seeded random configurations.
(c) every refusal returns its code and names the cause."""
import math

import numpy as np
import pytest

import pairec_amd as pa
from pairec_amd import _lib

import traffic_cases as cases
import traffic_ref as ref

P, Q = ref.PERCENT, ref.QUANTITY
PG_ERR_INVALID, PG_ERR_UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def tabs():
    return cases.tables(pa)


def host(c, **kw):
    t = pa.traffic_compile(c["targets"])
    try:
        return t.sort_host(c["ctx_size"], c["nq"], c["cap"], score=c["score"], member=c["member"], order=c["order"], count=c["count"],
                           alpha=c["alpha"], page_no=c["page_no"], gamma=c["gamma"], beta=c["beta"], eta=c["eta"], **kw)
    finally:
        t.free()


def check(tabs, c, what):
    cases.same_bits(host(c), cases.expect(tabs, c), what)


# ---- (a) the tables -----------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    a, b = np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64)      # (all positive: the patterns are ordered)
    return np.abs(a - b)


def test_tables_against_libm():
    want = ref.make_tables()
    for which, w in enumerate(want):
        got = pa.traffic_table(which)
        assert got.shape == (len(w),)
        assert int(_ulps(got, w).max()) <= 1, "table %d is more than 1 ulp from libm" % which
    assert pa.traffic_table(0)[0] == 1.0 and pa.traffic_table(1)[0] == 1.0 and pa.traffic_table(2)[0] == 0.0
    L = _lib.load()
    part = np.empty(3, np.float64)
    _lib.check(L.pg_traffic_table(3, 9997, 3, part.ctypes.data))
    assert np.array_equal(part, pa.traffic_table(3)[9997:])


def test_literals_are_exact(tabs):
    # positions >= 500 weigh the literal 0.006737946999, entry 0's itemScore is math.e: one uplifted target over 502 entries of
    # equal score shows both in new_pos (delta_0 = alpha' * e, w_i beyond 500 = s * literal in the sums)
    n = 502
    c = cases.case([(3, P)], 1, n, np.full((1, n), 0.5), np.ones((1, n), np.uint8), [[0.25]], ctx_size=1000)
    out = host(c)
    cases.same_bits(out, cases.expect(tabs, c), "literals")
    total = 0.0
    for i in range(n):
        total += 0.5 * (tabs.pos[i] if i < 500 else 0.006737946999)
    alpha = 0.25 * (1.0 + 1.0 * tabs.tanh_(1.0 * (total / total)))
    assert out[3][0, 0] == 1.0 - alpha * math.e
    assert out[3][0, 501] == 502.0 - alpha * tabs.exp[999]


# ---- (b) the host statement against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0, 1, 8])
@pytest.mark.parametrize("mix", ["zero", "negative", "positive", "mixed"])
def test_edge_lengths(tabs, T, mix):
    # n in 0, 1, 2, 499, 500, 501 as ragged counts of one call
    c = cases.lengths_case([0, 1, 2, 499, 500, 501], T, mix, seed=100 + T)
    if T == 0:
        c["score"] = c["member"] = c["alpha"] = None
    check(tabs, c, "lengths T=%d %s" % (T, mix))
    if mix == "zero" or T == 0:                      # the identity
        out = host(c)
        for q, n in enumerate([0, 1, 2, 499, 500, 501]):
            assert np.array_equal(out[0][q, :n], np.arange(n)) and np.array_equal(out[2][q, :n], np.arange(1, n + 1))
            assert np.array_equal(out[3][q, :n], np.arange(1, n + 1, dtype=np.float64))


@pytest.mark.parametrize("eta", [0.01, 1.6])
def test_pull_down_sigmoid_range(tabs, eta):
    # eta = 0.01: rho * i * 1000 - 5000 stays inside the sigmoid table for hundreds of positions; eta = 1.6: it leaves at once
    c = cases.lengths_case([501, 300], 8, "negative", seed=7, eta=eta)
    check(tabs, c, "pull down eta=%g" % eta)
    pos = host(c)[3]
    inside = np.sum(np.abs(np.diff(pos[0])) != 1.0)
    assert inside > (200 if eta == 0.01 else 0)


@pytest.mark.parametrize("page_no", [1, 2])
@pytest.mark.parametrize("ctx_size", [3, 40, 900])
def test_pages_and_ctx_size(tabs, page_no, ctx_size):
    # ctx_size below and above n = 120; page 2 moves `start` by goint((weight - 0.3) * 10 * ctx_size): members cover a large share for
    # target 0 (weight > 0.3) and a small one for target 1 (weight < 0.3)
    rng = np.random.default_rng(5)
    n = 120
    sc = cases.scores_desc(rng, 2, n)
    mem = ((rng.random((2, n)) < 0.8).astype(np.uint8)) | ((rng.random((2, n)) < 0.08).astype(np.uint8) << 1)
    c = cases.case([(21, P), (22, Q)], 2, n, sc, mem, [[3.0, 5.0], [0.8, 2.0]], ctx_size=ctx_size, page_no=page_no)
    check(tabs, c, "page %d ctx_size %d" % (page_no, ctx_size))
    _, _, cid, _ = host(c)
    if ctx_size == 3:
        assert (cid[0] == -21).any() and (cid[0] == 0).any()


@pytest.mark.parametrize("types", [(P, Q), (Q, P), (P, P), (Q, Q)])
def test_both_control_types_on_one_entry(tabs, types):
    # every entry is a member of both targets and both uplift past `start`: the later target decides a Percent id, a Quantity
    # target leaves an id that is already negative
    n = 12
    sc = np.linspace(1.0, 0.6, n)[None, :]
    c = cases.case([(31, types[0]), (32, types[1])], 1, n, sc, np.full((1, n), 3, np.uint8), [[2.0, 3.0]], ctx_size=2)
    check(tabs, c, "types %r" % (types,))
    cid = host(c)[2][0]
    want = {(P, Q): -31, (Q, P): -32, (P, P): -32, (Q, Q): 0}[types]
    assert np.array_equal(cid[:3], [1, 2, 3]) and (cid[3:] == want).all()


def test_irregular_scores(tabs):
    # 0.0, negatives, equal runs, a first score that is not the maximum (s / maxScore > 1 clamps to entry 999)
    sc = np.array([[0.4, 0.9, 0.9, 0.9, 0.0, 0.0, -0.1, -0.1, 0.3, 2.0, 0.4, 0.4, -5.0, 0.0]])
    n = sc.shape[1]
    rng = np.random.default_rng(3)
    for mix in ("negative", "positive", "mixed"):
        for page_no in (1, 2):
            c = cases.case(cases.TARGETS8[:4], 1, n, sc, cases.members(rng, 1, n, 4, 0.6), cases.alpha_rows(mix, 1, 4), ctx_size=4, page_no=page_no)
            check(tabs, c, "irregular %s page %d" % (mix, page_no))


def test_permuted_order_with_ragged_counts(tabs):
    c = cases.lengths_case([37, 0, 64, 5, 63], 8, "mixed", seed=11, cap=64, order=True, zero_middle=True)
    check(tabs, c, "permuted")
    c = cases.lengths_case([37, 0, 64, 5, 63], 1, "positive", seed=12, cap=64, order=True, page_no=2)
    check(tabs, c, "permuted T=1")


def test_optional_outputs_absent(tabs):
    c = cases.lengths_case([20, 33], 8, "mixed", seed=13)
    full = host(c)
    part = host(c, want_control_id=False, want_new_pos=False)
    assert part[2] is None and part[3] is None
    assert np.array_equal(part[0], full[0]) and np.array_equal(part[1], full[1])


def test_hostile_values(tabs):
    for T in (1, 3, 8):
        check(tabs, cases.hostile_case(T), "hostile T=%d" % T)
    for k, c in enumerate(cases.zero_total_cases(tabs)):
        check(tabs, c, "zero total %d" % k)
    # a NaN alpha gives NaN positions, and they sort last, by origin among themselves
    c = cases.hostile_case(8)
    out = host(c)
    nan = np.isnan(out[3][0])
    k = int(nan.sum())
    assert 0 < k < c["cap"]
    assert np.array_equal(out[0][0, c["cap"] - k:], np.flatnonzero(nan)) and not nan[out[0][0, :c["cap"] - k]].any()
    # ... and `total` is exactly 0.0 in the zero-total requests
    c = cases.zero_total_cases(tabs)[0]
    assert c["score"][0, 0] * tabs.pos[0] + c["score"][0, 1] * tabs.pos[1] == 0.0
    assert ref.goint(float("nan")) == ref.INT64_MIN and ref.goint(1e19) == ref.INT64_MIN and ref.goint(-3.9) == -3
    assert ref.wrap(ref.INT64_MIN - 5000) > 0 and tabs.sigmoid(float("nan"), 1.0) == 1.0


def test_random_configurations(tabs):
    for k, c in enumerate(cases.random_cases(300, seed=20251)):
        check(tabs, c, "random %d" % k)


# ---- (c) refusals ---------------------------------------------------------------------------------------------------------------
def test_compile_refusals():
    L = _lib.load()
    h = _lib.C.c_void_p()

    def compile_rc(targets):
        arr = (_lib.PgTrafficTarget * max(len(targets), 1))()
        for i, (tid, ty) in enumerate(targets):
            arr[i].target_id, arr[i].control_type = tid, ty
        h.value = None
        rc = L.pg_traffic_compile(arr, len(targets), _lib.C.byref(h))
        return rc, L.pg_last_error().decode()

    rc, msg = compile_rc([(i, P) for i in range(9)])
    assert rc == PG_ERR_UNSUPPORTED and "9 targets" in msg and "pg_traffic_compile" in msg and not h.value
    rc, msg = compile_rc([(1, P), (2, 3)])
    assert rc == PG_ERR_UNSUPPORTED and "control type 3" in msg and not h.value
    rc, msg = compile_rc([(1, 0)])
    assert rc == PG_ERR_UNSUPPORTED and "control type 0" in msg
    rc, msg = compile_rc([(1, P), (-2147483648, Q)])
    assert rc == PG_ERR_INVALID and "negation" in msg and not h.value
    rc, msg = compile_rc([])
    assert rc == 0 and h.value and L.pg_traffic_num_targets(h) == 0
    L.pg_traffic_free(h)
    t = pa.traffic_compile([{"TrafficControlTargetId": "17", "ControlType": "Percent"}, {"TrafficControlTargetId": 4, "ControlType": "Quantity"}])
    assert t.n_targets == 2
    t.free()


def test_call_refusals():
    L = _lib.load()
    t = pa.traffic_compile([(1, P), (2, Q)])
    t0 = pa.traffic_compile([])
    cap = 4
    sc, mem, al = np.ones((1, cap)), np.ones((1, cap), np.uint8), np.ones((1, 2))
    out, oc = np.empty((256, cap), np.uint32), np.empty(256, np.uint32)
    v = lambda a: None if a is None else a.ctypes.data                                   # noqa: E731

    def call(tr=t, ctx_size=5, page_no=1, nq=1, cap_=cap, score=sc, member=mem, alpha=al, order=None):
        rc = L.pg_traffic_sort_host(tr.h, ctx_size, page_no, 1.0, 1.0, 1.6, nq, cap_, v(score), v(member), v(order), None, v(alpha), v(out), v(oc), None,
                                    None)
        return rc, L.pg_last_error().decode()

    for kw, code, word in (({"nq": 0}, PG_ERR_INVALID, "nq=0"), ({"nq": 257}, PG_ERR_UNSUPPORTED, "nq=257"),
                           ({"cap_": 0}, PG_ERR_UNSUPPORTED, "cap=0"), ({"cap_": 16385}, PG_ERR_UNSUPPORTED, "cap=16385"),
                           ({"ctx_size": 0}, PG_ERR_INVALID, "ctx_size"), ({"page_no": 0}, PG_ERR_INVALID, "page_no"),
                           ({"score": None}, PG_ERR_INVALID, "score"), ({"member": None}, PG_ERR_INVALID, "member"),
                           ({"alpha": None}, PG_ERR_INVALID, "alpha"),
                           ({"order": np.array([[0, 1, 4, 2]], np.uint32)}, PG_ERR_INVALID, "order[0][2] = 4")):
        rc, msg = call(**kw)
        assert rc == code and word in msg and "pg_traffic_sort_host" in msg, (kw, rc, msg)
    # without targets nothing but the outputs is needed, and the answer is the identity
    rc, msg = call(tr=t0, score=None, member=None, alpha=None)
    assert rc == 0 and np.array_equal(out[0], np.arange(cap)) and oc[0] == cap
    rc, msg = call()
    assert rc == 0
    t.free()
    t0.free()
