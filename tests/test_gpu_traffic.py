"""GPU tests of TrafficControlSort's macro control on the device (csrc/traffic.hip: pg_traffic_sort_dev,
pg_traffic_sort) against tests/traffic_ref.py, by bits: every element of out_order, out_count, the control ids and new_pos (as
uint64), with the library's own tables handed to the restatement.  List lengths sit on the kernel's edges (a wave of 64, the
position-weight table's 500, the chunk of 1 024, two chunks and one), several lengths travel in one call as ragged counts, every
output carries a pre-filled guard region behind it that must stay untouched, and the optional outputs are given in some calls and
absent in others."""
import numpy as np
import pytest

import pairec_amd as pa
from pairec_amd._lib import PgError

import traffic_cases as cases
from test_gpu_mixsort import Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tabs():
    return cases.tables(pa)


def run_dev(ctx, c, optional=True, traffic=None, d_member=None):
    """pg_traffic_sort_dev on a case → (out_order, out_count, control_id | None, new_pos | None)"""
    nq, cap = c["nq"], c["cap"]
    out, cnt = np.empty((nq, cap), np.uint32), np.empty(nq, np.uint32)
    cid = np.empty((nq, cap), np.int32) if optional else None
    pos = np.empty((nq, cap), np.float64) if optional else None
    t = traffic or pa.traffic_compile(c["targets"])
    g = Guarded(ctx)
    try:
        ctx.traffic_sort_dev(t, c["ctx_size"], nq, cap, g.put(c["score"]), d_member or g.put(c["member"]), g.put(c["order"]), g.put(c["count"]),
                             g.put(c["alpha"]), g.out(out), g.out(cnt), g.out(cid) if optional else 0, g.out(pos) if optional else 0,
                             page_no=c["page_no"], gamma=c["gamma"], beta=c["beta"], eta=c["eta"])
        g.fetch()
    finally:
        g.free()
        if traffic is None:
            t.free()
    return out, cnt, cid, pos


# lengths on the kernel's edges: 0, 1, 63, 64, 65, 499, 500, 501 in one call; 1023, 1024, 1025, 2049 and 501 in another of nq = 5 and
# cap = 2112
SMALL, LARGE = [0, 1, 63, 64, 65, 499, 500, 501], [2049, 1025, 1024, 1023, 501]
_WANT = {}


def want(tabs, key, make):
    """a case and the restatement's answer to it, computed once per session"""
    if key not in _WANT:
        c = make()
        _WANT[key] = (c, cases.expect(tabs, c))
    return _WANT[key]


@pytest.mark.parametrize("T,mix,order,optional", [(8, "negative", False, True), (8, "positive", True, False), (8, "mixed", False, False),
                                                  (8, "mixed", True, True), (1, "mixed", False, True), (1, "positive", True, True)])
def test_edge_lengths(ctx, tabs, T, mix, order, optional):
    for name, lengths, cap in (("small", SMALL, 512), ("large", LARGE, 2112)):
        # a request whose alphas are all 0 sits between two that are not; eta = 0.01 keeps the pull-downs inside the sigmoid table
        c, w = want(tabs, (name, T, mix, order), lambda: cases.lengths_case(lengths, T, mix, seed=31 + T, cap=cap, order=order, zero_middle=True,
                                                                            page_no=2 if order else 1, ctx_size=20,
                                                                            eta=0.01 if mix == "negative" else 1.6))
        cases.same_bits(run_dev(ctx, c, optional), w, "%s T=%d %s order=%s" % (name, T, mix, order))


def test_hostile_values(ctx, tabs):
    c = cases.hostile_case(8)
    cases.same_bits(run_dev(ctx, c), cases.expect(tabs, c), "hostile")
    for k, c in enumerate(cases.zero_total_cases(tabs)[:4]):
        cases.same_bits(run_dev(ctx, c), cases.expect(tabs, c), "zero total %d" % k)


def test_order_values_outside_the_arrays_are_padding(ctx, tabs):
    # on the device an order value >= cap leaves the list first: the entries behind it move up, the count shrinks
    c = cases.lengths_case([40, 70, 9], 8, "mixed", seed=5, cap=70, order=True)
    c["order"][0, [0, 17, 39]] = [70, 0xFFFFFFFF, 1 << 20]
    c["order"][1, 64:] = 0xFFFFFFFF
    got = run_dev(ctx, c)
    cases.same_bits(got, cases.expect(tabs, c), "padding")
    assert list(got[1]) == [37, 64, 9]


def test_masks_from_classcut(ctx, tabs):
    # the targets' item expressions as a classcut set over a three-column store: its masks go straight in as d_member
    rng = np.random.default_rng(77)
    rows_n, nq, cap = 300, 3, 130
    store = {"cat": rng.integers(0, 6, rows_n).astype(np.int32), "brand": rng.integers(0, 9, rows_n).astype(np.int32),
             "price": rng.uniform(0, 10, rows_n).astype(np.float32)}
    decl = [("cat", pa.F_I32), ("brand", pa.F_I32), ("price", pa.F_F32)]
    fs = pa.Features(ctx, rows_n)
    for (n, f) in decl:
        fs.set_column(n, f, store[n])
    exprs = ["cat == 3 || cat in (5, 0)", "brand < 4 && price * 2 > 5", "cat == cat"]      # (the last: a target without an item expression)
    cc = pa.classcut_compile([(e, pa.TRIM_FIX, 1) for e in exprs], decl, [])
    rows = rng.integers(0, rows_n, (nq, cap)).astype(np.uint64)
    sc = cases.scores_desc(rng, nq, cap)
    idx = rows.astype(np.int64)
    member = cc.masks_host(sc.reshape(-1), cols={n: store[n][idx].reshape(-1) for n in store}).reshape(nq, cap)
    assert (member & 4).all() and 0 < (member & 1).mean() < 1 and 0 < (member & 2).mean() < 1
    c = cases.case([(41, cases.P), (42, cases.Q), (43, cases.P)], nq, cap, sc, member, [[3.0, -4.0, 0.5], [0.0, 2.0, -1.0], [-2.0, 0.0, 0.0]], ctx_size=15,
                   page_no=2, count=[130, 64, 129])
    d_rows, d_score, d_count = ctx.to_device(rows), ctx.to_device(sc), ctx.to_device(c["count"])
    d_masks = ctx.malloc(nq * cap)
    try:
        ctx.classcut_masks_dev(cc, fs, nq, cap, d_rows, d_score, 0, d_count, d_masks)       # no sync: the sort follows on the stream
        got = run_dev(ctx, c, d_member=d_masks)
    finally:
        for p in (d_rows, d_score, d_count, d_masks):
            ctx.free(p)
        cc.free()
        fs.destroy()
    cases.same_bits(got, cases.expect(tabs, c), "classcut masks")


def test_two_calls_back_to_back(ctx, tabs):
    # two calls on one stream without a synchronisation in between: the second's scratch must not disturb the first's answer
    c1, w1 = want(tabs, ("b2b", 1), lambda: cases.lengths_case([300, 1100, 17], 8, "mixed", seed=61, cap=1100))
    c2, w2 = want(tabs, ("b2b", 2), lambda: cases.lengths_case([900, 2, 1030, 64], 1, "negative", seed=62, cap=1030, order=True, eta=0.01))
    t1, t2 = pa.traffic_compile(c1["targets"]), pa.traffic_compile(c2["targets"])
    g = Guarded(ctx)
    outs = []
    try:
        for c, t in ((c1, t1), (c2, t2)):
            nq, cap = c["nq"], c["cap"]
            o = (np.empty((nq, cap), np.uint32), np.empty(nq, np.uint32), np.empty((nq, cap), np.int32), np.empty((nq, cap), np.float64))
            outs.append(o)
            ctx.traffic_sort_dev(t, c["ctx_size"], nq, cap, g.put(c["score"]), g.put(c["member"]), g.put(c["order"]), g.put(c["count"]),
                                 g.put(c["alpha"]), *[g.out(a) for a in o], page_no=c["page_no"], gamma=c["gamma"], beta=c["beta"], eta=c["eta"])
        g.fetch()
    finally:
        g.free()
        t1.free()
        t2.free()
    cases.same_bits(outs[0], w1, "first of two")
    cases.same_bits(outs[1], w2, "second of two")


def test_one_request_call(ctx, tabs):
    for seed, n, T, order in ((71, 1, 8, False), (72, 777, 8, True), (73, 1025, 1, False)):
        c = cases.lengths_case([n], T, "mixed", seed=seed, order=order, page_no=2, ctx_size=30)
        t = pa.traffic_compile(c["targets"])
        try:
            out, cnt, cid, pos = ctx.traffic_sort_one(t, c["ctx_size"], c["score"][0], c["member"][0], c["alpha"][0],
                                                      order=None if c["order"] is None else c["order"][0], page_no=2)
        finally:
            t.free()
        cases.same_bits((out[None, :], np.array([cnt], np.uint32), cid[None, :], pos[None, :]), cases.expect(tabs, c), "one request n=%d" % n)
    # n = 0 is an empty answer; without targets the identity
    t0 = pa.traffic_compile([])
    out, cnt, _, _ = ctx.traffic_sort_one(t0, 5, np.zeros(0), np.zeros(0, np.uint8), np.zeros(0))
    assert cnt == 0
    out, cnt, cid, pos = ctx.traffic_sort_one(t0, 5, np.ones(9), np.zeros(9, np.uint8), np.zeros(0))
    assert cnt == 9 and np.array_equal(out, np.arange(9)) and np.array_equal(cid, np.arange(1, 10)) and np.array_equal(pos, np.arange(1.0, 10.0))
    t0.free()


def test_refusals_leave_the_context_usable(ctx, tabs):
    c = cases.lengths_case([20, 33], 2, "mixed", seed=81)
    t = pa.traffic_compile(c["targets"])
    nq, cap = c["nq"], c["cap"]
    g = Guarded(ctx)
    try:
        out, cnt = np.empty((nq, cap), np.uint32), np.empty(nq, np.uint32)
        d = dict(score=g.put(c["score"]), member=g.put(c["member"]), alpha=g.put(c["alpha"]), count=g.put(c["count"]), out=g.out(out), cnt=g.out(cnt))

        def call(ctx_size=10, page_no=1, nq_=nq, cap_=cap, **kw):
            a = dict(d, **kw)
            ctx.traffic_sort_dev(t, ctx_size, nq_, cap_, a["score"], a["member"], a.get("order", 0), a["count"], a["alpha"], a["out"], a["cnt"],
                                 a.get("cid", 0), a.get("pos", 0), page_no=page_no)
        for kw, word in (({"nq_": 0}, "nq=0"), ({"nq_": 257}, "nq=257"), ({"cap_": 0}, "cap=0"), ({"cap_": 16385}, "cap=16385"),
                         ({"ctx_size": 0}, "ctx_size"), ({"page_no": 0}, "page_no"), ({"score": 0}, "score"), ({"member": 0}, "member"),
                         ({"alpha": 0}, "alpha"), ({"out": 0}, "NULL"), ({"cid": d["score"]}, "overlaps"), ({"pos": d["out"]}, "overlaps"),
                         ({"order": d["out"]}, "overlaps")):
            with pytest.raises(PgError) as e:
                call(**kw)
            assert word in str(e.value) and "pg_traffic_sort_dev" in str(e.value), (kw, str(e.value))
        call()                                        # the context is still usable
        g.fetch()
    finally:
        g.free()
        t.free()
    w = cases.expect(tabs, c)
    assert np.array_equal(out, w[0]) and np.array_equal(cnt, w[1])
    with pytest.raises(PgError) as e:
        ctx.traffic_sort_one(pa.traffic_compile([]), 5, np.ones(4), np.zeros(4, np.uint8), np.zeros(0), order=np.array([0, 1, 9, 2], np.uint32))
    assert "order[2] = 9" in str(e.value)
