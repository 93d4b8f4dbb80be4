"""PG_MODEL_MIND (csrc/mind.hip, rank_model.hpp's parsing) through the public API: the interests against tests/mind_ref.py in fp64
within each case's bar (mind_ref.BARS: 4 x the float32 restatement's error, measured on the CPU), pg_mind_recall against
pg_recall_topk on the very interests, and the refusals."""
import struct

import numpy as np
import pytest

import pairec_amd as pa
from mind_ref import BARS, CASES, MAX_SEQ, ROWS, inputs, reference, table, weights
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def tabs(ctx):
    """the sequence table at a row scale, uploaded on first use"""
    made = {}

    def get(scale=1.0):
        if scale not in made:
            made[scale] = pa.Table(ctx, ROWS, 64)
            made[scale].upload(table(scale))
        return made[scale]
    yield get
    for t in made.values():
        t.destroy()


def model(ctx, name):
    K, n_iter, d_out, h1, d_user, normalize, _, _ = CASES[name]
    return pa.RankModel(ctx, pa.MODEL_MIND, pa.PREC_F32, pa.pack_mind(*weights(K, d_out, h1, d_user), n_iter, normalize))


def interests_dev(ctx, m, tab, users, seqs):
    so = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint32)
    sr = np.concatenate(list(seqs) + [np.zeros(1, np.uint32)]).astype(np.uint32)
    out = np.empty((len(seqs), m.n_out, m._mind_shape()[0]), dtype=np.float32)
    bufs = [ctx.to_device(users), ctx.to_device(sr), ctx.to_device(so), ctx.malloc(out.nbytes)]
    m.mind_interests_dev(tab, bufs[0], bufs[1], bufs[2], len(seqs), bufs[3])
    ctx.d2h(out, bufs[3])
    for b in bufs:
        ctx.free(b)
    return out


def check_case(ctx, tabs, name):
    users, seqs = inputs(name)
    m = model(ctx, name)
    try:
        assert m.n_out == CASES[name][0]
        got = interests_dev(ctx, m, tabs(CASES[name][6]), users, seqs)
        if name != "long":                                                   # the host form: the same kernel, the same bits
            assert np.array_equal(m.mind_interests(tabs(CASES[name][6]), users, seqs).view(np.uint32), got.view(np.uint32))
    finally:
        m.destroy()
    err = np.max(np.abs(got.astype(np.float64) - reference(name)))
    print("%s: max |interest - fp64| = %.3e (bar %.3e)" % (name, err, BARS[name]))
    assert err <= BARS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_interests_against_the_reference(ctx, tabs, name):
    check_case(ctx, tabs, name)


@pytest.mark.parametrize("name,n_req", [("edges", 5), ("neighbours", 40)], ids=["K3 one pass", "K8 40 requests two passes"])
def test_recall_is_the_recall_of_the_interests(ctx, tabs, name, n_req):
    K, k = CASES[name][0], 10
    rng = np.random.default_rng(5)
    users = rng.standard_normal((n_req, CASES[name][4])).astype(np.float32)
    seqs = [rng.integers(0, ROWS + 50, n).astype(np.uint32) for n in rng.integers(0, 60, n_req)]
    items = pa.Table(ctx, 3000, 64)
    items.upload((rng.standard_normal((3000, 64)) / 8).astype(np.float32))
    m = model(ctx, name)
    try:
        q = m.mind_interests(tabs(), users, seqs)
        rows, scores, counts = m.mind_recall(tabs(), items, users, seqs, k)
        want_rows, want_scores, _ = items.recall_topk(q.reshape(n_req * K, 64), k // K)
    finally:
        m.destroy()
        items.destroy()
    assert rows.shape == scores.shape == (n_req, K, k // K) and np.all(counts == k // K)
    assert np.array_equal(rows.reshape(-1, k // K), want_rows)
    assert np.array_equal(scores.reshape(-1, k // K).view(np.uint32), want_scores.view(np.uint32))


def hdr(b, **kw):
    """the blob with header fields replaced"""
    f = dict(zip(("d_user", "d_out", "K", "n_iter", "h1", "normalize"), struct.unpack("<6I", b[:24])))
    f.update(kw)
    return struct.pack("<6I", *f.values()) + b[24:]


@pytest.mark.parametrize("make,prec,code", [
    (lambda b: b[:-4], pa.PREC_F32, INVALID),
    (lambda b: b, pa.PREC_BF16, UNSUPPORTED),
    (lambda b: b, pa.PREC_BF16X3, UNSUPPORTED),
    (lambda b: hdr(b, d_user=0), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, d_user=1025), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, d_out=32), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, K=9), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, K=0), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, n_iter=5), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, h1=64), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, normalize=2), pa.PREC_F32, UNSUPPORTED),
    (lambda b: b[:24 + 4 * 4100] + struct.pack("<f", np.nan) + b[24 + 4 * 4101:], pa.PREC_F32, UNSUPPORTED),
], ids=["one float short", "bf16", "bf16x3", "d_user 0", "d_user 1025", "d_out 32", "K 9", "K 0", "5 iterations", "h1 64", "normalize 2", "NaN in b0"])
def test_load_refusals(ctx, tabs, make, prec, code):
    blob = pa.pack_mind(*weights(3, 64, 128, 7), 3, 0)
    with pytest.raises(PgError) as e:
        pa.RankModel(ctx, pa.MODEL_MIND, prec, make(blob))
    assert e.value.code == code
    check_case(ctx, tabs, "single-pass")                                     # the context is still usable


def interests_raw(ctx, m, tab, users, seq_rows, seq_off):
    """pg_mind_interests on offsets as given"""
    so, sr = np.asarray(seq_off, dtype=np.uint32), np.asarray(seq_rows, dtype=np.uint32)
    out = np.empty((len(so) - 1, 3, 64), dtype=np.float32)
    ptr = pa.engine._ptr
    pa._lib.check(ctx.L.pg_mind_interests(ctx.h, m.h, tab.h, ptr(users), ptr(sr), ptr(so), len(so) - 1, ptr(out)))


def test_call_refusals(ctx, tabs):
    users, seqs = inputs("edges")
    m = model(ctx, "edges")
    wide, items = pa.Table(ctx, 3000, 128), pa.Table(ctx, 300, 64)
    w = weights(3, 64, 128, 7)
    dnn = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_F32, pa.pack_dnn3(np.zeros((64 + 64, 128)), w[4], np.zeros((128, 128)), w[4], w[4], 0.0, 64))
    try:
        for call in (lambda: dnn.mind_interests(tabs(), users, seqs),                                     # a model of another kind
                     lambda: dnn.mind_recall(tabs(), items, users, seqs, 10),
                     lambda: m.mind_interests(wide, users, seqs),                                         # seq_table dim != 64
                     lambda: m.mind_recall(tabs(), wide, users, seqs, 10),                                # item_emb dim != d_out
                     lambda: interests_raw(ctx, m, tabs(), users, seqs[6], [0, 9, 4]),                    # offsets that descend
                     lambda: interests_raw(ctx, m, tabs(), users, seqs[6], [1, 4, 9]),                    # ... or do not start at 0
                     lambda: m.mind_interests(tabs(), users[:1], [np.zeros(MAX_SEQ + 1, np.uint32)]),     # a sequence too long
                     lambda: m.mind_recall(tabs(), items, users[:1], [np.zeros(MAX_SEQ + 1, np.uint32)], 10),
                     lambda: m.mind_interests(tabs(), np.zeros((257, 7), np.float32), [[]] * 257),        # n_req outside 1..256
                     lambda: m.mind_interests(tabs(), users[:0], []),
                     lambda: m.mind_recall(tabs(), items, users, seqs, 2),                                # k < K
                     lambda: m.mind_recall(tabs(), items, users[:1], seqs[:1], 3 * 16385),                # k / K > 16384
                     lambda: m.rank_dnn3(tabs(), users, np.zeros(4, np.uint32), [0, 4]),                  # existing entries refuse the kind
                     lambda: m.online_vector_recall(items, users, 10)):
            with pytest.raises(PgError) as e:
                call()
            assert e.value.code == INVALID
            got = m.mind_interests(tabs(), users, seqs)                                                   # ... and the context is usable
            assert np.max(np.abs(got - reference("edges"))) <= BARS["edges"]
        with pytest.raises(PgError) as e:                                                                 # the coalescer refuses the kind too
            pa.Coalescer(ctx, wide, 10, algos=[("mind", m)])
        assert e.value.code == INVALID and "PG_MODEL_MIND" in str(e.value)
    finally:
        for x in (dnn, m, wide, items):
            x.destroy()
