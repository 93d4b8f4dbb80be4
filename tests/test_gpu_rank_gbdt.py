"""PG_MODEL_GBDT (csrc/rank_gbdt.hip, rank_model.hpp's parsing and device packing, pa.pack_gbdt) through RankModel.rank_gbdt_dev,
against tests/gbdt_ref.py over the pointer trees.

Both bars are derived, not measured.  Objective 1: the walk is exact and the fp64 chain's order is the specification, so the scores
are BIT-EQUAL to the reference margins rounded to float32.  Objective 0: |score - fp64 sigmoid| <= 2^-25 + 1e-12 — one fp32
rounding of a value in (0, 1) costs at most 2^-25, and the kernel's fp64 exp (Go's, restated) differs from numpy's by a few 1e-16."""
import functools
import struct

import numpy as np
import pytest

import pairec_amd as pa
from gbdt_cases import BASE, PARITY, ROWS, blob, columns, forest, inputs
from gbdt_ref import gbdt_margins, gbdt_scores
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4
SMALL = PARITY[0]


@functools.lru_cache(maxsize=None)
def reference(case):
    return gbdt_scores(gbdt_margins(forest(case), BASE, inputs(case[0], case[1], case[7])[3], le=case[5]), case[4])


@pytest.fixture(scope="module")
def feats(ctx):
    f = pa.Features(ctx, ROWS)
    for k, (dt, v, default) in enumerate(columns(64)):          # (a case with fewer item features uses the first of them)
        f.set_column("c%d" % k, dt, v, default)
    yield f
    f.destroy()


def rank_dev(ctx, m, feats, n_item, users, cand, off):
    bufs = [ctx.to_device(a) if a.size else 0 for a in (users, cand, off)] + [ctx.malloc(len(cand) * 4)]
    out = np.empty(len(cand), dtype=np.float32)
    m.rank_gbdt_dev(feats, ["c%d" % k for k in range(n_item)], bufs[0], bufs[1], bufs[2], len(off) - 1, len(cand), bufs[3])
    ctx.d2h(out, bufs[3])
    for b in bufs:
        if b:
            ctx.free(b)
    return out


@pytest.mark.parametrize("case", PARITY, ids=lambda c: "-".join(map(str, c[:7])) + "-%d" % sum(c[7]))
def test_parity_with_the_reference(ctx, feats, case):
    users, cand, off, _ = inputs(case[0], case[1], case[7])
    m = pa.RankModel(ctx, pa.MODEL_GBDT, pa.PREC_F32, blob(case))
    try:
        assert m.n_out == 1
        got = rank_dev(ctx, m, feats, case[1], users, cand, off)
    finally:
        m.destroy()
    want = reference(case)
    if case[4] == 1:
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        print("case %s: %d of %d scores differ from the reference's bits" % (case[:7], len(bad), len(got)))
        assert len(bad) == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    else:
        err = np.max(np.abs(got.astype(np.float64) - want))
        print("case %s: max |score - fp64 sigmoid| = %.3e (bar %.3e)" % (case[:7], err, 2.0 ** -25 + 1e-12))
        assert err <= 2.0 ** -25 + 1e-12


def hdr(b, **kw):
    """the blob with header fields replaced"""
    f = dict(zip(("n_user", "n_item", "n_tree", "depth", "objective"), struct.unpack("<5I", b[:20])))
    f.update(kw)
    return struct.pack("<5I", *f.values()) + b[20:]


def word(b, at, value):
    """the blob with the 4 bytes at `at` past the header replaced"""
    return b[:24 + at] + value + b[28 + at:]


NODES = 255     # of SMALL's depth-8 tree: its thresholds start at 4 * NODES, its leaves at 8 * NODES


@pytest.mark.parametrize("make,prec,code", [
    (lambda b: b[:-4], pa.PREC_F32, INVALID),
    (lambda b: b, pa.PREC_BF16, UNSUPPORTED),
    (lambda b: b, pa.PREC_BF16X3, UNSUPPORTED),
    (lambda b: hdr(b, depth=9), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, depth=0), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, n_tree=0), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, n_tree=4097), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, n_user=65), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, n_user=0, n_item=0), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, objective=2), pa.PREC_F32, UNSUPPORTED),
    (lambda b: word(b, 4 * 9, struct.pack("<I", 8)), pa.PREC_F32, UNSUPPORTED),
    (lambda b: word(b, 4 * (NODES + 9), struct.pack("<f", np.nan)), pa.PREC_F32, UNSUPPORTED),
    (lambda b: word(b, 4 * (2 * NODES + 9), struct.pack("<f", np.inf)), pa.PREC_F32, UNSUPPORTED),
], ids=["one float short", "bf16", "bf16x3", "depth 9", "depth 0", "no trees", "4097 trees", "65 user features", "no features", "objective 2",
        "feature 8 of 8", "NaN threshold", "infinite leaf"])
def test_load_refusals(ctx, make, prec, code):
    with pytest.raises(PgError) as e:
        pa.RankModel(ctx, pa.MODEL_GBDT, prec, make(blob(SMALL)))
    assert e.value.code == code


def test_call_refusals(ctx, feats):
    from oracle import oracle as o
    users, cand, off, _ = inputs(SMALL[0], SMALL[1], SMALL[7])
    m = pa.RankModel(ctx, pa.MODEL_GBDT, pa.PREC_F32, blob(SMALL))
    w = o.Dnn3Weights()
    dnn = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_F32, pa.pack_dnn3(w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, 128))
    tab = pa.Table(ctx, ROWS, 128)
    cols = ["c0", "c1", "c2"]
    try:
        for call in (lambda: m.rank_gbdt(feats, [0, 1, 64], users, cand, off),          # a column outside the store
                     lambda: m.rank_gbdt(feats, [0, -1, 2], users, cand, off),
                     lambda: dnn.rank_gbdt(feats, cols, users, cand, off),              # a model of another kind
                     lambda: m.rank_dnn3(tab, np.zeros((len(off) - 1, 128), np.float32), np.minimum(cand, ROWS - 1), off),
                     lambda: m.rank_gbdt(feats, cols, users, cand, off[::-1].copy())):  # offsets that descend
            with pytest.raises(PgError) as e:
                call()
            assert e.value.code == INVALID
        with pytest.raises(PgError) as e:                                               # the coalescer refuses the kind as well
            pa.Coalescer(ctx, tab, 10, algos=[("forest", m)])
        assert e.value.code == INVALID and "PG_MODEL_GBDT" in str(e.value)
        got = m.rank_gbdt(feats, cols, users, cand, off)                                # the context and the model are still usable
        assert np.array_equal(got.view(np.uint32), reference(SMALL).view(np.uint32))
    finally:
        tab.destroy()
        dnn.destroy()
        m.destroy()
