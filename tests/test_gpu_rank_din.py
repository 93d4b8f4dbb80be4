"""PG_MODEL_DIN (csrc/rank_din.hip, rank_model.hpp's fold) through the public API, against tests/din_ref.py in fp64.

The bars are not device figures.  din_ref was evaluated on the CPU over exactly the parity inputs below, once in float32 with the
same naive formula and once more in float32 with e, s_l and the attention weights a_l rounded to bf16 before the trunk's first
layer; the largest |score - fp64 score| over all parity cases was
    float32:              7.986e-08  (bar 3.19e-07)
    float32, bf16 inputs: 2.513e-05  (bar 5.03e-05)
The F32 and BF16X3 bar is 4 x the first (the folded form and the MFMA summation order differ from numpy's: a small constant over a
same-precision evaluation), the BF16 bar 2 x the second (rounding dominates there, not order)."""
import functools
import struct

import numpy as np
import pytest

import pairec_amd as pa
from din_ref import din_scores
from oracle import oracle as o
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

F32_CPU_ERR, BF16_CPU_ERR = 7.986e-08, 2.513e-05        # measured on the CPU as the docstring says
BAR = {pa.PREC_F32: 4 * F32_CPU_ERR, pa.PREC_BF16X3: 4 * F32_CPU_ERR, pa.PREC_BF16: 2 * BF16_CPU_ERR}
INVALID, UNSUPPORTED = -1, -4
ROWS, D, D_USER = 3000, 64, 24
# (candidates, sequence length): every tile edge against both position chunks (Lc = 8 for att_h 32, 16 for att_h 16)
REQS = [(0, 64), (1, 1), (127, 7), (128, 8), (129, 9), (700, 63), (0, 0), (1, 15), (127, 16), (128, 17), (129, 0), (700, 64)]


def weights(att_h, h1, h2, n_out, mono=False):
    u = lambda k, n, fan: o.synth_uniform(o.SEED_WEIGHTS ^ (0xD100 + k), n, 1.0 / np.sqrt(fan))   # noqa: E731
    din = D_USER + 2 * D
    w = {"wa": u(1, 4 * D * att_h, 4 * D).reshape(4 * D, att_h), "ba": u(2, att_h, 4 * D), "wa2": u(3, att_h, att_h),
         "ba2": float(u(4, 1, att_h)[0]), "w1": u(5, din * h1, din).reshape(din, h1), "b1": u(6, h1, din),
         "w2": u(7, h1 * h2, h1).reshape(h1, h2), "b2": u(8, h2, h1), "w3": u(9, h2 * n_out, h2).reshape(h2, n_out), "b3": u(10, n_out, h2)}
    if mono:            # the score as a function of ONE pooled coordinate: a wrong pooling cannot hide under the trunk
        keep = 8 * w["w1"][D_USER + D + 5].copy()
        w["w1"][:] = 0
        w["w1"][D_USER + D + 5] = keep
    return w


@functools.lru_cache(maxsize=None)
def inputs():
    rng = np.random.default_rng(7)
    table = o.synth_rows(o.SEED_TABLE, 0, ROWS, D)
    users = o.synth_rows(o.SEED_QUERY, 0, len(REQS), D_USER)
    off = np.concatenate([[0], np.cumsum([c for c, _ in REQS])]).astype(np.uint32)
    cand = rng.integers(0, ROWS, int(off[-1])).astype(np.uint32)
    cand[[0, 200, 1500]] = ROWS - 1
    cand[[3, 300, 1600, 2100]] = [ROWS, ROWS + 5, 0xFFFFFFFF, ROWS]          # past the table: the last row
    seqs = [rng.integers(0, ROWS, n).astype(np.uint32) for _, n in REQS]
    seqs[2][3] = ROWS + 7                                                    # a history item the table no longer holds
    seqs[5][[10, 62]] = [ROWS, 0xFFFFFFFF]
    seqs[3][6] = seqs[3][1]                                                  # a repeated row
    return table, users, seqs, cand, off


@functools.lru_cache(maxsize=None)
def reference(att_h, h1, h2, n_out, mono):
    return din_scores(weights(att_h, h1, h2, n_out, mono), D_USER, *inputs())


@pytest.fixture(scope="module")
def tab(ctx):
    t = pa.Table(ctx, ROWS, D)
    t.upload(inputs()[0])
    yield t
    t.destroy()


def blob(w):
    return pa.pack_din(w["wa"], w["ba"], w["wa2"], w["ba2"], w["w1"], w["b1"], w["w2"], w["b2"], w["w3"], w["b3"], D_USER)


PARITY = [(a, h1, h2, 1, False) for a in (16, 32) for h1, h2 in ((128, 128), (512, 256))] + [(32, 128, 128, 2, False), (32, 128, 128, 1, True)]


@pytest.mark.parametrize("prec", [pa.PREC_F32, pa.PREC_BF16, pa.PREC_BF16X3])
@pytest.mark.parametrize("att_h,h1,h2,n_out,mono", PARITY)
def test_parity_with_the_reference(ctx, tab, prec, att_h, h1, h2, n_out, mono):
    _, users, seqs, cand, off = inputs()
    m = pa.RankModel(ctx, pa.MODEL_DIN, prec, blob(weights(att_h, h1, h2, n_out, mono)))
    try:
        got = m.rank_din(tab, users, seqs, cand, off).reshape(n_out, -1).astype(np.float64)
    finally:
        m.destroy()
    err = np.max(np.abs(got - reference(att_h, h1, h2, n_out, mono)))
    print("prec %d att_h %d trunk %d-%d heads %d mono %d: max |score - fp64| = %.3e (bar %.3e)" % (prec, att_h, h1, h2, n_out, mono, err, BAR[prec]))
    assert err <= BAR[prec]


def test_a_call_past_one_staging_run(ctx, tab):
    """more candidates than kDinRunItems (2^17): two runs, the second request cut by the boundary"""
    rng = np.random.default_rng(8)
    off = np.array([0, 100_000, 100_000, 131_072 + 700], dtype=np.uint32)
    cand = rng.integers(0, ROWS, int(off[-1])).astype(np.uint32)
    users = o.synth_rows(o.SEED_QUERY, 100, 3, D_USER)
    seqs = [rng.integers(0, ROWS, n).astype(np.uint32) for n in (2, 5, 3)]
    w = weights(16, 128, 128, 1)
    m = pa.RankModel(ctx, pa.MODEL_DIN, pa.PREC_F32, blob(w))
    try:
        got = m.rank_din(tab, users, seqs, cand, off).astype(np.float64)
    finally:
        m.destroy()
    err = np.max(np.abs(got - din_scores(w, D_USER, inputs()[0], users, seqs, cand, off)[0]))
    print("two runs: max |score - fp64| = %.3e (bar %.3e)" % (err, BAR[pa.PREC_F32]))
    assert err <= BAR[pa.PREC_F32]


@pytest.mark.parametrize("prec", [pa.PREC_F32, pa.PREC_BF16X3])
def test_empty_sequences_reduce_to_the_dnn3_trunk(ctx, tab, prec):
    _, users, _, cand, off = inputs()
    cand = np.minimum(cand, ROWS - 1)                                        # (pg_rank_dnn3 refuses rows past the table)
    w = weights(32, 128, 128, 1)
    din = pa.RankModel(ctx, pa.MODEL_DIN, prec, blob(w))
    dnn = pa.RankModel(ctx, pa.MODEL_DNN3, prec, pa.pack_dnn3(w["w1"][:D_USER + D], w["b1"], w["w2"], w["b2"], w["w3"], w["b3"][0], D_USER))
    try:
        got = din.rank_din(tab, users, [[] for _ in REQS], cand, off).astype(np.float64)
        want = dnn.rank_dnn3(tab, users, cand, off).astype(np.float64)
    finally:
        din.destroy()
        dnn.destroy()
    assert np.max(np.abs(got - want)) <= BAR[pa.PREC_F32]


def hdr(b, **kw):
    """the blob with header fields replaced (d_user, d_item, h1, h2, n_out, att_h)"""
    f = dict(zip(("d_user", "d_item", "h1", "h2", "n_out", "att_h"), struct.unpack("<6I", b[:24])))
    f.update(kw)
    return struct.pack("<6I", *f.values()) + b[24:]


@pytest.mark.parametrize("make,prec,code", [
    (lambda b: b[:-4], pa.PREC_F32, INVALID),
    (lambda b: hdr(b, att_h=24), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, d_item=128), pa.PREC_F32, UNSUPPORTED),
    (lambda b: b, pa.PREC_F16, UNSUPPORTED),
], ids=["one float short", "att_h 24", "d_item 128", "fp16"])
def test_load_refusals(ctx, make, prec, code):
    with pytest.raises(PgError) as e:
        pa.RankModel(ctx, pa.MODEL_DIN, prec, make(blob(weights(32, 128, 128, 1))))
    assert e.value.code == code


def test_call_refusals(ctx, tab):
    _, users, seqs, cand, off = inputs()
    m = pa.RankModel(ctx, pa.MODEL_DIN, pa.PREC_F32, blob(weights(32, 128, 128, 1)))
    wide = pa.Table(ctx, 64, 128)
    try:
        for table, s, call in ((tab, [np.zeros(65, np.uint32)] + seqs[1:], m.rank_din), (wide, seqs, m.rank_din),
                               (tab, None, m.rank_dnn3)):
            with pytest.raises(PgError) as e:
                call(table, users, s, cand, off) if s is not None else call(table, users, cand, off)
            assert e.value.code == INVALID
        assert m.rank_din(tab, users, seqs, cand, off).shape == cand.shape   # the context and the model are still usable
    finally:
        wide.destroy()
        m.destroy()
