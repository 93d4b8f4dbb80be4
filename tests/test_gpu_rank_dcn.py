"""PG_MODEL_DCN (csrc/rank_dcn.hip, rank_model.hpp's packing) through the public API, against tests/dcn_ref.py in fp64.

The bars are not device figures.  dcn_ref was evaluated on the CPU over exactly the parity inputs below, once in float32 with the
same naive formula and once more in float32 with the BF16 form's rounding points; the largest |score - fp64 score| over all parity
cases was
    float32:                 7.603e-08  (BF16X3 bar 3.04e-07; per case 6.5e-08 .. 7.6e-08)
    float32, bf16 rounding:  4.868e-05  (BF16 bar 9.74e-05; per case 3.5e-05 .. 4.9e-05) outside the d_user = 1 case, which has its
                             own entry: 1.171e-04 (bar 2.34e-04), 2.4 x the rest
The BF16X3 bar is 4 x the first (the kernel's summation order and expf differ from numpy's by a small constant over a
same-precision evaluation), the BF16 bar 2 x the second (rounding dominates there, not order).  The "strong" variant scales the
cross weights and biases x 8: swapping two output columns of the last cross matrix then moves a score by 1.1e-3 .. 2.1e-3 (8e-5 ..
2.7e-4 in the two plain cases).  Observed on an MI355X: BF16X3 <= 1.446e-07; BF16 <= 4.868e-05, 1.171e-04 in the d_user = 1 case."""
import functools
import struct

import numpy as np
import pytest

import pairec_amd as pa
from dcn_ref import dcn_scores
from oracle import oracle as o
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

F32_CPU_ERR, BF16_CPU_ERR, BF16_CPU_ERR_USER1 = 7.603e-08, 4.868e-05, 1.171e-04        # measured on the CPU as the docstring says
BAR = {pa.PREC_BF16X3: 4 * F32_CPU_ERR, pa.PREC_BF16: 2 * BF16_CPU_ERR}
INVALID, UNSUPPORTED = -1, -4
ROWS = 3000
REQS = (0, 1, 127, 128, 129, 700)           # candidates per request: every edge of the 128-candidate tile and an empty request
# (d_user, d_item, L, h1, h2, n_out, variant): D = 256; 128 (no padding) and 129 (one past it, padded to 192) on both d_item; a
# padded 256; d_user 1; every L; both heads; n_out 1, 2, 4
PARITY = [(128, 128, 3, 256, 128, 4, "strong"), (64, 64, 2, 128, 128, 1, "strong"), (65, 64, 1, 256, 128, 4, "strong"),
          (1, 128, 3, 128, 128, 1, "strong"), (24, 128, 3, 256, 128, 2, ""), (150, 64, 2, 128, 128, 4, "")]


def weights(d_user, d_item, L, h1, h2, n_out, variant=""):
    u = lambda k, shape, fan: o.synth_uniform(o.SEED_WEIGHTS ^ (0xDC00 + k), int(np.prod(shape)), 1.0 / np.sqrt(fan)).reshape(shape)   # noqa: E731
    D = d_user + d_item
    w = {"wc": u(1, (L, D, D), D), "bc": u(2, (L, D), D), "w1": u(3, (D, h1), D), "b1": u(4, (h1,), D), "w2": u(5, (h1, h2), h1),
         "b2": u(6, (h2,), h1), "w3": u(7, (h2, n_out), h2), "b3": u(8, (n_out,), h2)}
    if variant == "strong":
        w["wc"], w["bc"] = w["wc"] * np.float32(8), w["bc"] * np.float32(8)
    return w


@functools.lru_cache(maxsize=None)
def inputs(d_user, d_item):
    rng = np.random.default_rng(11)
    table = o.synth_rows(o.SEED_TABLE, 0, ROWS, d_item)
    users = o.synth_rows(o.SEED_QUERY, 0, len(REQS), d_user)
    off = np.concatenate([[0], np.cumsum(REQS)]).astype(np.uint32)
    cand = rng.integers(0, ROWS, int(off[-1])).astype(np.uint32)
    cand[[0, 200, 900]] = ROWS - 1
    cand[[1, 300, 1000, 1084]] = [ROWS, ROWS + 5, 0xFFFFFFFF, ROWS]          # past the table: the last row
    return table, users, cand, off


@functools.lru_cache(maxsize=None)
def reference(case):
    return dcn_scores(weights(*case), case[0], *inputs(case[0], case[1]))


@pytest.fixture(scope="module")
def tabs(ctx):
    t = {d: pa.Table(ctx, ROWS, d) for d in (64, 128)}
    for d in t:
        t[d].upload(inputs(1, d)[0])
    yield t
    for d in t:
        t[d].destroy()


def blob(w, d_user):
    return pa.pack_dcn(w["wc"], w["bc"], w["w1"], w["b1"], w["w2"], w["b2"], w["w3"], w["b3"], d_user)


def rank_dev(ctx, m, tab, users, cand, off):
    """pg_rank_dcn_dev over device copies (the host call refuses rows past the table)"""
    bufs = [ctx.to_device(a) for a in (users, cand, off)] + [ctx.malloc(m.n_out * len(cand) * 4)]
    out = np.empty((m.n_out, len(cand)), dtype=np.float32)
    m.rank_dcn_dev(tab, bufs[0], bufs[1], bufs[2], len(off) - 1, len(cand), bufs[3])
    ctx.d2h(out, bufs[3])
    for b in bufs:
        ctx.free(b)
    return out


@pytest.mark.parametrize("prec", [pa.PREC_BF16, pa.PREC_BF16X3])
@pytest.mark.parametrize("case", PARITY, ids=lambda c: "-".join(map(str, c)))
def test_parity_with_the_reference(ctx, tabs, prec, case):
    _, users, cand, off = inputs(case[0], case[1])
    m = pa.RankModel(ctx, pa.MODEL_DCN, prec, blob(weights(*case), case[0]))
    try:
        assert m.n_out == case[5]
        got = rank_dev(ctx, m, tabs[case[1]], users, cand, off).astype(np.float64)
    finally:
        m.destroy()
    bar = 2 * BF16_CPU_ERR_USER1 if prec == pa.PREC_BF16 and case[0] == 1 else BAR[prec]
    err = np.max(np.abs(got - reference(case)))
    print("prec %d case %s: max |score - fp64| = %.3e (bar %.3e)" % (prec, case, err, bar))
    assert err <= bar


@pytest.mark.parametrize("prec", [pa.PREC_BF16, pa.PREC_BF16X3])
@pytest.mark.parametrize("beta", [0, 1])
def test_zero_cross_weights_reduce_to_the_dnn3(ctx, tabs, prec, beta):
    """Wc = 0 and bc = beta: x_L = (1 + L beta) x_0 exactly (x_0 for beta 0, 4 x_0 for beta 1 and L = 3), so every head is the
    two-head DNN3 [24 + 128]-256-128 whose w1 is scaled by 1 + L beta.  The users are bf16 values: the DNN3's BF16 form rounds the
    user vector, the DCN's does not."""
    _, users, cand, off = inputs(24, 128)
    users, cand = o.f32_to_bf16_round(users), np.minimum(cand, ROWS - 1)     # (the host calls refuse rows past the table)
    w = weights(24, 128, 3, 256, 128, 2)
    w["wc"][:], w["bc"][:] = 0, beta
    m = pa.RankModel(ctx, pa.MODEL_DCN, prec, blob(w, 24))
    dnn = pa.RankModel(ctx, pa.MODEL_DNN3_MULTI, prec, pa.pack_dnn3_multi(w["w1"] * np.float32(1 + 3 * beta), w["b1"], w["w2"], w["b2"], w["w3"],
                                                                          w["b3"], 24))
    try:
        got = m.rank_dcn(tabs[128], users, cand, off).astype(np.float64)
        want = dnn.rank_dnn3(tabs[128], users, cand, off).astype(np.float64)
    finally:
        dnn.destroy()
        m.destroy()
    assert got.shape == want.shape == (2, len(cand))
    assert np.max(np.abs(got - want)) <= 2 * BAR[prec]


def hdr(b, **kw):
    """the blob with header fields replaced"""
    f = dict(zip(("d_user", "d_item", "n_cross", "h1", "h2", "n_out"), struct.unpack("<6I", b[:24])))
    f.update(kw)
    return struct.pack("<6I", *f.values()) + b[24:]


@pytest.mark.parametrize("make,prec,code", [
    (lambda b: b[:-4], pa.PREC_BF16, INVALID),
    (lambda b: hdr(b, n_cross=0), pa.PREC_BF16, UNSUPPORTED),
    (lambda b: hdr(b, n_cross=4), pa.PREC_BF16, UNSUPPORTED),
    (lambda b: hdr(b, h1=512, h2=256), pa.PREC_BF16, UNSUPPORTED),
    (lambda b: hdr(b, d_item=96), pa.PREC_BF16, UNSUPPORTED),
    (lambda b: hdr(b, d_user=193), pa.PREC_BF16, UNSUPPORTED),
    (lambda b: hdr(b, n_out=5), pa.PREC_BF16, UNSUPPORTED),
    (lambda b: b, pa.PREC_F32, UNSUPPORTED),
    (lambda b: b, pa.PREC_F16, UNSUPPORTED),
], ids=["one float short", "L 0", "L 4", "512-256", "d_item 96", "D 257", "n_out 5", "fp32", "fp16"])
def test_load_refusals(ctx, make, prec, code):
    with pytest.raises(PgError) as e:
        pa.RankModel(ctx, pa.MODEL_DCN, prec, make(blob(weights(24, 64, 1, 128, 128, 2), 24)))
    assert e.value.code == code


def test_call_refusals(ctx, tabs):
    _, users, cand, off = inputs(24, 64)
    cand = np.minimum(cand, ROWS - 1)
    w = weights(24, 64, 1, 128, 128, 2)
    m = pa.RankModel(ctx, pa.MODEL_DCN, pa.PREC_BF16, blob(w, 24))
    dnn = pa.RankModel(ctx, pa.MODEL_DNN3_MULTI, pa.PREC_BF16, pa.pack_dnn3_multi(w["w1"], w["b1"], w["w2"], w["b2"], w["w3"], w["b3"], 24))
    try:
        for call, table in ((m.rank_dcn, tabs[128]), (m.rank_dnn3, tabs[64]), (m.rank_mmoe, tabs[64]), (dnn.rank_dcn, tabs[64])):
            with pytest.raises(PgError) as e:
                call(table, users, cand, off)
            assert e.value.code == INVALID
        assert m.rank_dcn(tabs[64], users, cand, off).shape == (2, len(cand))   # the context and the model are still usable
    finally:
        dnn.destroy()
        m.destroy()
