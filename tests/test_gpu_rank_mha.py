"""PG_MODEL_MHA (csrc/rank_mha.hip, rank_model.hpp's packing) through the public API, against tests/mha_ref.py in fp64.

The bars are not device figures.  mha_ref was evaluated on the CPU over exactly the inputs below, once in float32 with the same
naive formula and once more in float32 with the BF16 form's rounding points (the attention's and the bf16 trunk's); the largest
|score - fp64 score| over all cases of each kind was
    parity, float32:                 7.519e-08  (F32 and BF16X3 bar 3.01e-07; per case 6.8e-08 .. 7.5e-08)
    parity, float32, bf16 rounding:  9.723e-05  (BF16 bar 1.94e-04; per case 3.7e-05 .. 9.7e-05)
    steep logits, float32:           7.133e-08  (bar 2.85e-07; the float32 evaluation stays finite, logits -54.0 .. +51.5)
    steep logits, bf16 rounding:     3.744e-04  (bar 7.49e-04: q's rounding error is multiplied by the logits' size)
The F32 and BF16X3 bar is 4 x the float32 figure (the kernel's permuted and blocked
summation order and v_exp_f32 differ from numpy's by a small constant over a same-precision evaluation), the BF16 bar 2 x the
bf16 figure (rounding dominates there, not order)."""
import functools
import struct

import numpy as np
import pytest

import pairec_amd as pa
from mha_ref import mha_scores
from oracle import oracle as o
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

F32_CPU_ERR, BF16_CPU_ERR = 7.519e-08, 9.723e-05              # measured on the CPU as the docstring says
STEEP_F32_CPU_ERR, STEEP_BF16_CPU_ERR = 7.133e-08, 3.744e-04
STEEP_GAIN = 3.7           # on Wq and Wk, on top of the parity gains: logits of -54 .. +52 instead of -5 .. +5
INVALID, UNSUPPORTED = -1, -4
ROWS, D, D_USER = 3000, 64, 24
# (candidates, sequence length): every edge of the 128-candidate tile and of the 32-position block, both ends of the sequence
REQS = [(0, 64), (1, 1), (127, 31), (128, 32), (129, 33), (700, 511), (1, 512), (127, 0), (128, 65), (129, 64), (700, 33), (1, 40)]


def bars(f32_err, bf16_err):
    return {pa.PREC_F32: 4 * f32_err, pa.PREC_BF16X3: 4 * f32_err, pa.PREC_BF16: 2 * bf16_err}


def weights(d_att, n_head, h1, h2, n_out, mono=False, steep=1.0):
    u = lambda k, shape, fan, g=1.0: o.synth_uniform(o.SEED_WEIGHTS ^ (0xA700 + k), int(np.prod(shape)), g / np.sqrt(fan)).reshape(shape)   # noqa: E731
    din = D_USER + 2 * D
    # (gains: logits of a few units, |pooled| of 0.85 .. 1.2 beside |e| = 1 — an attention left uniform or lost under the trunk
    # would pass anything; a larger pooled would test the trunk on rows three times the norm of any table's)
    w = {"wq": u(1, (D, d_att), D, 12 * steep), "bq": u(2, (d_att,), D, 8), "wk": u(3, (D, d_att), D, 12 * steep), "wv": u(4, (D, d_att), D, 8),
         "bv": u(5, (d_att,), D), "wo": u(6, (d_att, D), d_att, 1.5), "w1": u(7, (din, h1), din), "b1": u(8, (h1,), din),
         "w2": u(9, (h1, h2), h1), "b2": u(10, (h2,), h1), "w3": u(11, (h2, n_out), h2), "b3": u(12, (n_out,), h2)}
    if mono:            # the score as a function of ONE pooled coordinate: a wrong attention cannot hide under the trunk
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
    seqs[2][0] = ROWS + 7                                                    # entries the table no longer holds: at the start,
    seqs[5][[100, 300]] = [ROWS, 0xFFFFFFFF]                                 # in the middle,
    seqs[8][32:64] = ROWS + 1                                                # a whole block of them (the last valid entry moves up),
    seqs[10][1:] = 0xFFFFFFFF                                                # all but one,
    seqs[11][:] = ROWS                                                       # and a request with nothing else
    seqs[3][6] = seqs[3][1]                                                  # a repeated row
    return table, users, seqs, cand, off


@functools.lru_cache(maxsize=None)
def steep_inputs(d_att, n_head):
    """Logits of about +-60 (STEEP_GAIN).  Request 0's sequence is ordered so that head 0's running max rises in every 32-position
    block for its first 64 candidates (one row), request 1's so that it never moves after the first block for its first."""
    rng = np.random.default_rng(9)
    table, users = inputs()[0], inputs()[1][:2]
    off = np.array([0, 129, 258], dtype=np.uint32)
    cand = rng.integers(0, ROWS, 258).astype(np.uint32)
    cand[:64] = cand[0]
    w = weights(d_att, n_head, 128, 128, 1, steep=STEEP_GAIN)
    seqs = []
    for r, n in enumerate((200, 512)):
        s = rng.integers(0, ROWS, n).astype(np.uint32)
        d_h = d_att // n_head
        a = (table[s].astype(np.float64) @ w["wk"][:, :d_h]) @ (table[cand[off[r]]].astype(np.float64) @ w["wq"][:, :d_h] + w["bq"][:d_h])
        seqs.append(s[np.argsort(a if r == 0 else -a)])
    return table, users, seqs, cand, off


@functools.lru_cache(maxsize=None)
def reference(case):
    d_att, n_head, h1, h2, n_out, mono = case
    return mha_scores(weights(d_att, n_head, h1, h2, n_out, mono), D_USER, n_head, *inputs())


@pytest.fixture(scope="module")
def tab(ctx):
    t = pa.Table(ctx, ROWS, D)
    t.upload(inputs()[0])
    yield t
    t.destroy()


def blob(w, n_head):
    return pa.pack_mha(w["wq"], w["bq"], w["wk"], w["wv"], w["bv"], w["wo"], w["w1"], w["b1"], w["w2"], w["b2"], w["w3"], w["b3"], D_USER, n_head)


def run(ctx, tab, prec, w, n_head, users, seqs, cand, off):
    m = pa.RankModel(ctx, pa.MODEL_MHA, prec, blob(w, n_head))
    try:
        return m.rank_mha(tab, users, seqs, cand, off).reshape(w["b3"].shape[0], -1).astype(np.float64)
    finally:
        m.destroy()


# (d_att, n_head, h1, h2, n_out, mono): all four attention shapes on 128-128, one on 512-256, two heads, the mono model
PARITY = [(64, 1, 128, 128, 1, False), (64, 2, 128, 128, 1, False), (128, 2, 128, 128, 1, False), (128, 4, 128, 128, 1, False),
          (128, 4, 512, 256, 1, False), (64, 2, 128, 128, 2, False), (128, 4, 128, 128, 1, True), (64, 1, 128, 128, 1, True)]


@pytest.mark.parametrize("prec", [pa.PREC_F32, pa.PREC_BF16, pa.PREC_BF16X3])
@pytest.mark.parametrize("case", PARITY)
def test_parity_with_the_reference(ctx, tab, prec, case):
    d_att, n_head, h1, h2, n_out, mono = case
    got = run(ctx, tab, prec, weights(d_att, n_head, h1, h2, n_out, mono), n_head, *inputs()[1:])
    err, bar = np.max(np.abs(got - reference(case))), bars(F32_CPU_ERR, BF16_CPU_ERR)[prec]
    print("prec %d case %s: max |score - fp64| = %.3e (bar %.3e)" % (prec, case, err, bar))
    assert err <= bar


@pytest.mark.parametrize("prec", [pa.PREC_F32, pa.PREC_BF16, pa.PREC_BF16X3])
@pytest.mark.parametrize("d_att,n_head", [(64, 1), (128, 4)])
def test_steep_logits(ctx, tab, prec, d_att, n_head):
    """a wrong rescale when the max moves, or an exponent taken without the max, shows here"""
    _, users, seqs, cand, off = steep_inputs(d_att, n_head)
    w = weights(d_att, n_head, 128, 128, 1, steep=STEEP_GAIN)
    got = run(ctx, tab, prec, w, n_head, users, seqs, cand, off)
    err, bar = np.max(np.abs(got - mha_scores(w, D_USER, n_head, *steep_inputs(d_att, n_head)))), bars(STEEP_F32_CPU_ERR, STEEP_BF16_CPU_ERR)[prec]
    print("steep, prec %d d_att %d heads %d: max |score - fp64| = %.3e (bar %.3e)" % (prec, d_att, n_head, err, bar))
    assert err <= bar


def test_a_call_past_one_run(ctx, tab):
    """more candidates than a run stages (2^17) and more requests than a run keeps keys for (256): the runs are cut by both, one
    request cut by the candidate boundary"""
    rng = np.random.default_rng(8)
    counts = np.concatenate([[100_000, 0, 31_072 + 700], np.full(297, 3)])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    cand = rng.integers(0, ROWS, int(off[-1])).astype(np.uint32)
    users = o.synth_rows(o.SEED_QUERY, 100, len(counts), D_USER)
    seqs = [rng.integers(0, ROWS, n).astype(np.uint32) for n in rng.integers(0, 40, len(counts))]
    w = weights(64, 2, 128, 128, 1)
    got = run(ctx, tab, pa.PREC_F32, w, 2, users, seqs, cand, off)
    err, bar = np.max(np.abs(got - mha_scores(w, D_USER, 2, inputs()[0], users, seqs, cand, off))), bars(F32_CPU_ERR, BF16_CPU_ERR)[pa.PREC_F32]
    print("past one run: max |score - fp64| = %.3e (bar %.3e)" % (err, bar))
    assert err <= bar


@pytest.mark.parametrize("prec", [pa.PREC_F32, pa.PREC_BF16X3])
def test_empty_sequences_reduce_to_the_dnn3_trunk(ctx, tab, prec):
    _, users, _, cand, off = inputs()
    cand = np.minimum(cand, ROWS - 1)                                        # (pg_rank_dnn3 refuses rows past the table)
    w = weights(128, 4, 128, 128, 1)
    dnn = pa.RankModel(ctx, pa.MODEL_DNN3, prec, pa.pack_dnn3(w["w1"][:D_USER + D], w["b1"], w["w2"], w["b2"], w["w3"], w["b3"][0], D_USER))
    try:
        want = dnn.rank_dnn3(tab, users, cand, off).astype(np.float64)
    finally:
        dnn.destroy()
    got = run(ctx, tab, prec, w, 4, users, [[] for _ in REQS], cand, off)[0]
    assert np.max(np.abs(got - want)) <= bars(F32_CPU_ERR, BF16_CPU_ERR)[pa.PREC_F32]


def hdr(b, **kw):
    """the blob with header fields replaced"""
    f = dict(zip(("d_user", "d_item", "h1", "h2", "n_out", "d_att", "n_head"), struct.unpack("<7I", b[:28])))
    f.update(kw)
    return struct.pack("<7I", *f.values()) + b[28:]


@pytest.mark.parametrize("make,prec,code", [
    (lambda b: b[:-4], pa.PREC_F32, INVALID),
    (lambda b: hdr(b, n_head=8), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, d_item=128), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, h1=192), pa.PREC_F32, UNSUPPORTED),
    (lambda b: hdr(b, n_out=9), pa.PREC_F32, UNSUPPORTED),
    (lambda b: b, pa.PREC_F16, UNSUPPORTED),
], ids=["one float short", "d_h 16", "d_item 128", "h1 192", "n_out 9", "fp16"])
def test_load_refusals(ctx, make, prec, code):
    with pytest.raises(PgError) as e:
        pa.RankModel(ctx, pa.MODEL_MHA, prec, make(blob(weights(128, 4, 128, 128, 1), 4)))
    assert e.value.code == code


def test_call_refusals(ctx, tab):
    _, users, seqs, cand, off = inputs()
    m = pa.RankModel(ctx, pa.MODEL_MHA, pa.PREC_F32, blob(weights(64, 2, 128, 128, 1), 2))
    wide = pa.Table(ctx, 64, 128)
    try:
        for table, s, call in ((tab, [np.zeros(513, np.uint32)] + seqs[1:], m.rank_mha), (wide, seqs, m.rank_mha), (tab, seqs, m.rank_din),
                               (tab, None, m.rank_dnn3), (tab, None, m.rank_mmoe), (tab, None, m.rank_dcn)):
            with pytest.raises(PgError) as e:
                call(table, users, s, cand, off) if s is not None else call(table, users, cand, off)
            assert e.value.code == INVALID
        assert m.rank_mha(tab, users, seqs, cand, off).shape == cand.shape   # the context and the model are still usable
    finally:
        wide.destroy()
        m.destroy()
