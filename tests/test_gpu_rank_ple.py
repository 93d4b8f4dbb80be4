"""PG_MODEL_PLE (csrc/rank_ple.hip, rank_model.hpp's packing) through the public API, against tests/ple_ref.py in fp64.

The bars are not device figures.  ple_ref was evaluated on the CPU over exactly the parity inputs below, once in float32 with the
same naive formula and once more in float32 with the BF16 form's rounding points (candidate row, weight matrices, x1_g, the towers'
inputs); the largest |score - fp64 score| over all parity cases was
    float32:                 7.068e-08  (BF16X3 bar 2.83e-07)
    float32, bf16 rounding:  2.821e-05  (BF16 bar 5.64e-05) outside the saturated-gate case, which alone reaches 8.254e-04 and has
                             its own entry (bar 1.65e-03), as MMoE's saturated case would have needed
The BF16X3 bar is 4 x the first (the kernel's summation order and expf differ from numpy's by a small constant over a
same-precision evaluation), the BF16 bar 2 x the second (rounding dominates there, not order).  No instantiation of the kernel is
single-buffered, so no case is there for one.  Observed on an MI355X: BF16 <= 2.821e-05 (saturated 8.254e-04); BF16X3 <= 9.02e-08
(the saturated case; it gave 2.939e-07 while level 1's experts of a two-level model took three products per term, which is why
they take six: DESIGN.md section 5 item 13)."""
import functools
import struct

import numpy as np
import pytest

import pairec_amd as pa
from oracle import oracle as o
from pairec_amd._lib import PgError
from ple_ref import ple_scores

pytestmark = pytest.mark.gpu

F32_CPU_ERR, BF16_CPU_ERR, BF16_SAT_CPU_ERR = 7.068e-08, 2.821e-05, 8.254e-04        # measured on the CPU as the docstring says
INVALID, UNSUPPORTED = -1, -4
ROWS, D_USER = 3000, 24
REQS = (0, 1, 127, 128, 129, 700)           # candidates per request: every tile edge and an empty request
# (d_item, T, E_t, E_s, h_e, levels, h_t, variant): both d_item and h_t, T 1 and 3, E_t != E_s both ways, h_e 128 with one level,
# the largest two-level shape
PARITY = [(128, 3, 2, 2, 64, 2, 64, ""), (64, 1, 1, 2, 64, 2, 32, ""), (128, 3, 2, 1, 64, 1, 32, ""), (64, 1, 2, 2, 128, 1, 64, ""),
          (64, 2, 2, 1, 64, 2, 64, "coordinate"), (128, 2, 1, 2, 64, 2, 32, "saturated")]
SAT_L2_GAIN = 650.0                             # the saturated case's factor on level 2's gate weights (checked in test_rank_ple_cpu.py)


def bar(prec, case):
    if prec == pa.PREC_BF16X3:
        return 4 * F32_CPU_ERR
    return 2 * (BF16_SAT_CPU_ERR if case[7] == "saturated" else BF16_CPU_ERR)


def weights(d_item, T, e_t, e_s, h_e, n_level, h_t, variant=""):
    k = iter(range(1, 100))
    u = lambda shape, fan: o.synth_uniform(o.SEED_WEIGHTS ^ (0x91E0 + next(k)), int(np.prod(shape)), 1.0 / np.sqrt(fan)).reshape(shape)   # noqa: E731
    levels = []
    for lv in range(n_level):
        n_in = h_e if lv else D_USER + d_item
        w = {"we_t": u((T, e_t, n_in, h_e), n_in), "we_s": u((e_s, n_in, h_e), n_in), "be_t": u((T, e_t, h_e), n_in), "be_s": u((e_s, h_e), n_in),
             "wg_t": u((T, n_in, e_t + e_s), n_in), "bg_t": u((T, e_t + e_s), n_in)}
        if lv + 1 < n_level:
            w.update({"wg_s": u((n_in, T * e_t + e_s), n_in), "bg_s": u((T * e_t + e_s,), n_in)})
        if variant == "coordinate":     # unequal gates at both levels
            w["bg_t"] = (0.5 * np.arange(e_t + e_s)[None, :] - 0.3 * np.arange(T)[:, None] + 0.2 * lv).astype(np.float32)
            if "bg_s" in w:
                w["bg_s"] = (0.4 * np.arange(T * e_t + e_s) - 0.7).astype(np.float32)
        if variant == "saturated":      # logits to about +-80: exp overflows fp32 without the max subtraction
            gain = np.float32(SAT_L2_GAIN if lv else 30 * np.sqrt(n_in))
            w["wg_t"] = w["wg_t"] * gain
            if "wg_s" in w:
                w["wg_s"] = w["wg_s"] * gain
        levels.append(w)
    w = {"levels": levels, "wt": u((T, h_e, h_t), h_e), "bt": u((T, h_t), h_e), "wo": u((T, h_t), h_t), "bo": u((T,), h_t)}
    if variant == "coordinate":         # the score as a function of ONE coordinate of x_t per task
        keep = 8 * w["wt"][:, 37].copy()
        w["wt"][:] = 0
        w["wt"][:, 37] = keep
    return w


@functools.lru_cache(maxsize=None)
def inputs(d_item):
    rng = np.random.default_rng(11)
    table = o.synth_rows(o.SEED_TABLE, 0, ROWS, d_item)
    users = o.synth_rows(o.SEED_QUERY, 0, len(REQS), D_USER)
    off = np.concatenate([[0], np.cumsum(REQS)]).astype(np.uint32)
    cand = rng.integers(0, ROWS, int(off[-1])).astype(np.uint32)
    cand[[0, 200, 900]] = ROWS - 1
    cand[[1, 300, 1000, 1084]] = [ROWS, ROWS + 5, 0xFFFFFFFF, ROWS]          # past the table: the last row
    return table, users, cand, off


@functools.lru_cache(maxsize=None)
def reference(case):
    return ple_scores(weights(*case), D_USER, *inputs(case[0]))


@pytest.fixture(scope="module")
def tabs(ctx):
    t = {d: pa.Table(ctx, ROWS, d) for d in (64, 128)}
    for d in t:
        t[d].upload(inputs(d)[0])
    yield t
    for d in t:
        t[d].destroy()


def blob(w):
    return pa.pack_ple(w["levels"], w["wt"], w["bt"], w["wo"], w["bo"], D_USER)


def rank_dev(ctx, m, tab, users, cand, off):
    """pg_rank_ple_dev over device copies (the host call refuses rows past the table)"""
    bufs = [ctx.to_device(a) for a in (users, cand, off)] + [ctx.malloc(m.n_out * len(cand) * 4)]
    out = np.empty((m.n_out, len(cand)), dtype=np.float32)
    m.rank_ple_dev(tab, bufs[0], bufs[1], bufs[2], len(off) - 1, len(cand), bufs[3])
    ctx.d2h(out, bufs[3])
    for b in bufs:
        ctx.free(b)
    return out


@pytest.mark.parametrize("prec", [pa.PREC_BF16, pa.PREC_BF16X3])
@pytest.mark.parametrize("case", PARITY, ids=lambda c: "-".join(map(str, c)))
def test_parity_with_the_reference(ctx, tabs, prec, case):
    _, users, cand, off = inputs(case[0])
    m = pa.RankModel(ctx, pa.MODEL_PLE, prec, blob(weights(*case)))
    try:
        assert m.n_out == case[1]
        got = rank_dev(ctx, m, tabs[case[0]], users, cand, off).astype(np.float64)
    finally:
        m.destroy()
    err = np.max(np.abs(got - reference(case)))
    print("prec %d case %s: max |score - fp64| = %.3e (bar %.3e)" % (prec, case, err, bar(prec, case)))
    assert err <= bar(prec, case)


@pytest.mark.parametrize("prec", [pa.PREC_BF16, pa.PREC_BF16X3])
@pytest.mark.parametrize("h_e", [64, 128])
def test_one_task_one_level_is_the_mmoe(ctx, tabs, prec, h_e):
    """T = 1, one level, E_t = E_s = 2: the task gate covers all four experts, so the model is the MMoE (4, h_e) with one task on
    the same weights."""
    _, users, cand, off = inputs(64)
    cand = np.minimum(cand, ROWS - 1)       # (the host calls refuse rows past the table)
    w = weights(64, 1, 2, 2, h_e, 1, 32)
    lv = w["levels"][0]
    m = pa.RankModel(ctx, pa.MODEL_PLE, prec, blob(w))
    mm = pa.RankModel(ctx, pa.MODEL_MMOE, prec, pa.pack_mmoe(np.concatenate([lv["we_t"][0], lv["we_s"]]), np.concatenate([lv["be_t"][0], lv["be_s"]]),
                                                              lv["wg_t"], lv["bg_t"], w["wt"], w["bt"], w["wo"], w["bo"], D_USER))
    try:
        got = m.rank_ple(tabs[64], users, cand, off).astype(np.float64)
        want = mm.rank_mmoe(tabs[64], users, cand, off).astype(np.float64)
    finally:
        mm.destroy()
        m.destroy()
    assert np.max(np.abs(got - want)) <= 2 * bar(prec, PARITY[0])


def hdr(b, **kw):
    """the blob with header fields replaced"""
    f = dict(zip(("d_user", "d_item", "n_task", "e_task", "e_shared", "h_e", "n_level", "h_t"), struct.unpack("<8I", b[:32])))
    f.update(kw)
    return struct.pack("<8I", *f.values()) + b[32:]


@pytest.mark.parametrize("make,prec,code", [
    (lambda b: b[:-4], pa.PREC_BF16, INVALID),
    (lambda b: hdr(b, n_task=4), pa.PREC_BF16, UNSUPPORTED),
    (lambda b: hdr(b, n_level=3), pa.PREC_BF16, UNSUPPORTED),
    (lambda b: hdr(b, h_e=128), pa.PREC_BF16, UNSUPPORTED),
    (lambda b: hdr(b, d_item=96), pa.PREC_BF16, UNSUPPORTED),
    (lambda b: b, pa.PREC_F32, UNSUPPORTED),
    (lambda b: b, pa.PREC_F16, UNSUPPORTED),
], ids=["one float short", "T 4", "3 levels", "h_e 128 in two levels", "d_item 96", "fp32", "fp16"])
def test_load_refusals(ctx, make, prec, code):
    with pytest.raises(PgError) as e:
        pa.RankModel(ctx, pa.MODEL_PLE, prec, make(blob(weights(64, 2, 1, 1, 64, 2, 32))))
    assert e.value.code == code


def test_call_refusals(ctx, tabs):
    _, users, cand, off = inputs(64)
    cand = np.minimum(cand, ROWS - 1)
    w = weights(64, 2, 1, 1, 64, 2, 32)
    lv = w["levels"][0]
    m = pa.RankModel(ctx, pa.MODEL_PLE, pa.PREC_BF16, blob(w))
    mm = pa.RankModel(ctx, pa.MODEL_MMOE, pa.PREC_BF16, pa.pack_mmoe(np.concatenate([lv["we_t"][0], lv["we_t"][1], lv["we_s"], lv["we_s"]]), np.zeros((4, 64)),
                                                                     np.zeros((1, D_USER + 64, 4)), np.zeros((1, 4)), w["wt"][:1], w["bt"][:1],
                                                                     w["wo"][:1], w["bo"][:1], D_USER))
    try:
        for call, table in ((m.rank_ple, tabs[128]), (m.rank_dnn3, tabs[64]), (m.rank_mmoe, tabs[64]), (mm.rank_ple, tabs[64])):
            with pytest.raises(PgError) as e:
                call(table, users, cand, off)
            assert e.value.code == INVALID
        assert m.rank_ple(tabs[64], users, cand, off).shape == (2, len(cand))   # the context and the model are still usable
    finally:
        mm.destroy()
        m.destroy()
