"""The four host-buffer rank entries (pg_rank_dnn3, pg_rank_fm2t, pg_rank_fm2t_rows, pg_rank_fm2t_irows) and pg_model_load
(csrc/rank_entry.hip) through the public API: the same bits as the matching *_dev entry on the same inputs, the empty calls that
return PG_OK before any data pointer is looked at, and every refusal with its status and exact text — each leaves the context
usable, the next good call scoring the same bits as before.  Every refusal happens on the host, before any launch.

Shapes, the smallest the kernels accept: a table of 64 rows x 64; DNN3 [1 + 64] -> 128 -> 128 -> 1; FM + two-tower with 1 user
field, 16 item fields x 8, d_user 1, towers 128-64, vocab 1, over a feature store of 2 rows and its item records.  Requests of
0, 1 and 33 candidates."""
import ctypes as C
import struct

import numpy as np
import pytest

import pairec_amd as pa
from oracle import oracle as o
from pairec_amd._lib import PgError, check

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4
OFFSETS = np.array([0, 0, 1, 34], dtype=np.uint32)
N_REQ, N_ITEMS = 3, 34
FIELDS = ["if%d" % f for f in range(16)]


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Entry:
    """one host-buffer entry and its *_dev form: (handles..., inputs in argument order..., offsets, n_req[, n_items], scores)"""

    def __init__(self, ctx, name, handles, inputs, n_out=1):
        self.ctx, self.name, self.handles, self.inputs, self.n_out = ctx, name, handles, inputs, n_out

    def host_rc(self, inputs=None, offsets=OFFSETS, n_req=N_REQ, handles=None, with_out=True):
        inputs = self.inputs if inputs is None else inputs
        out = np.full(self.n_out * int(offsets[-1]), np.nan, dtype=np.float32) if with_out else None
        rc = getattr(self.ctx.L, self.name)(self.ctx.h, *(self.handles if handles is None else handles), *[ptr(a) for a in inputs],
                                           ptr(offsets), n_req, ptr(out))
        return rc, out

    def host(self, **kw):
        rc, out = self.host_rc(**kw)
        check(rc)
        return out

    def dev(self):
        ctx = self.ctx
        bufs = [ctx.to_device(a) for a in self.inputs] + [ctx.to_device(OFFSETS), ctx.malloc(self.n_out * N_ITEMS * 4)]
        try:
            check(getattr(ctx.L, self.name + "_dev")(ctx.h, *self.handles, *[C.c_void_p(b) for b in bufs[:-1]], N_REQ, N_ITEMS,
                                                     C.c_void_p(bufs[-1])))
            out = np.zeros(self.n_out * N_ITEMS, dtype=np.float32)
            ctx.d2h(out, bufs[-1])
        finally:
            for b in bufs:
                ctx.free(b)
        return out

    def refused(self, code, text, **kw):
        rc, _ = self.host_rc(**kw)
        assert rc == code
        assert self.ctx.L.pg_last_error().decode() == text


def fm2t_weights():
    return o.Fm2tWeights(n_user_fields=1, n_item_fields=16, k=8, d_user=1, t_h1=128, t_out=64, vocab=1)


def dnn3_weights():
    return o.Dnn3Weights(d_user=1, d_item=64, h1=128, h2=128)


def dnn3_blob(w=None):
    w = w or dnn3_weights()
    return pa.pack_dnn3(w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, 1)


@pytest.fixture(scope="module")
def world(ctx):
    rng = np.random.default_rng(20)
    t = pa.Table(ctx, 64, 64)
    t.upload(rng.standard_normal((64, 64)).astype(np.float32))
    t128 = pa.Table(ctx, 64, 128)
    dnn = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_BF16, dnn3_blob())
    fm_blob = pa.pack_fm2t(fm2t_weights())
    fm = pa.RankModel(ctx, pa.MODEL_FM_TWOTOWER, pa.PREC_BF16, fm_blob)
    fm_other = pa.RankModel(ctx, pa.MODEL_FM_TWOTOWER, pa.PREC_BF16, fm_blob)
    fs = pa.Features(ctx, 2)
    for name in FIELDS:
        fs.set_column(name, pa.F_I32, np.zeros(2, dtype=np.int32))
    cols = fs._cols(FIELDS)
    ir = pa.ItemRows(fm, fs, FIELDS)
    ir_other = pa.ItemRows(fm_other, fs, FIELDS)
    u = rng.standard_normal((N_REQ, 1)).astype(np.float32)
    uf = np.zeros((N_REQ, 1), dtype=np.int32)
    cand = rng.integers(0, 64, N_ITEMS).astype(np.uint32)
    itf = np.zeros((N_ITEMS, 16), dtype=np.int32)
    rows = rng.integers(0, 2, N_ITEMS).astype(np.uint32)
    entries = {
        "pg_rank_dnn3": Entry(ctx, "pg_rank_dnn3", [dnn.h, t.h], [u, cand]),
        "pg_rank_fm2t": Entry(ctx, "pg_rank_fm2t", [fm.h], [u, uf, itf]),
        "pg_rank_fm2t_rows": Entry(ctx, "pg_rank_fm2t_rows", [fm.h, fs.h, ptr(cols)], [u, uf, rows]),
        "pg_rank_fm2t_irows": Entry(ctx, "pg_rank_fm2t_irows", [fm.h, ir.h], [u, uf, rows]),
    }
    good = {name: e.host() for name, e in entries.items()}         # computed once, never changed
    yield {"ctx": ctx, "entries": entries, "good": good, "t": t, "t128": t128, "dnn": dnn, "fm": fm, "ir_other": ir_other, "cols": cols}
    for x in (ir, ir_other, fs, dnn, fm, fm_other, t, t128):
        x.destroy()


NAMES = ["pg_rank_dnn3", "pg_rank_fm2t", "pg_rank_fm2t_rows", "pg_rank_fm2t_irows"]


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def still_good(world, name):
    assert np.array_equal(bits(world["entries"][name].host()), bits(world["good"][name]))


@pytest.mark.parametrize("name", NAMES)
def test_same_bits_as_the_dev_entry(world, name):
    got = world["good"][name]
    assert got.shape == (N_ITEMS,) and np.all(np.isfinite(got)) and np.all((got > 0) & (got < 1))
    assert np.array_equal(bits(got), bits(world["entries"][name].dev()))


@pytest.mark.parametrize("name", NAMES)
def test_empty_calls_return_ok_without_data(world, name):
    e = world["entries"][name]
    none = [None] * len(e.inputs)
    assert e.host_rc(inputs=none, offsets=np.zeros(1, dtype=np.uint32), n_req=0, with_out=False)[0] == 0
    assert e.host_rc(inputs=none, offsets=np.zeros(4, dtype=np.uint32), n_req=3, with_out=False)[0] == 0
    still_good(world, name)


@pytest.mark.parametrize("name", NAMES)
def test_offsets_refused(world, name):
    e = world["entries"][name]
    e.refused(INVALID, name + ": req_offsets[0] must be 0", offsets=np.array([1, 1, 2, 34], dtype=np.uint32))
    e.refused(INVALID, name + ": req_offsets not monotone at 1", offsets=np.array([0, 5, 3, 34], dtype=np.uint32))
    still_good(world, name)


@pytest.mark.parametrize("name", NAMES[1:])
def test_user_field_id_refused(world, name):
    e = world["entries"][name]
    for bad in (-1, 1):                               # below zero; equal to vocab
        uf = e.inputs[1].copy()
        uf[2, 0] = bad
        e.refused(INVALID, "%s: user field id %d outside vocab 1" % (name, bad), inputs=[e.inputs[0], uf, e.inputs[2]])
        still_good(world, name)


def test_dnn3_candidate_row_and_table_dim_refused(world):
    e = world["entries"]["pg_rank_dnn3"]
    cand = e.inputs[1].copy()
    cand[33] = 64
    e.refused(INVALID, "pg_rank_dnn3: candidate 33 row 64 outside table of 64 rows", inputs=[e.inputs[0], cand])
    still_good(world, "pg_rank_dnn3")
    e.refused(INVALID, "pg_rank_dnn3: table dim 128 != model d_item 64", handles=[world["dnn"].h, world["t128"].h])
    still_good(world, "pg_rank_dnn3")


def test_fm2t_item_field_id_refused(world):
    e = world["entries"]["pg_rank_fm2t"]
    for bad in (-1, 1):
        itf = e.inputs[2].copy()
        itf[33, 15] = bad
        e.refused(INVALID, "pg_rank_fm2t: item field id %d outside vocab 1" % bad, inputs=[e.inputs[0], e.inputs[1], itf])
        still_good(world, "pg_rank_fm2t")


def test_irows_of_another_model_refused(world):
    e = world["entries"]["pg_rank_fm2t_irows"]
    e.refused(INVALID, "pg_rank_fm2t_irows: the item records belong to another model", handles=[world["fm"].h, world["ir_other"].h])
    still_good(world, "pg_rank_fm2t_irows")


def test_model_load_refusals(world):
    ctx = world["ctx"]
    w = dnn3_weights()
    multi = pa.pack_dnn3_multi(w.w1, w.b1, w.w2, w.b2, np.stack([w.w3, w.w3], axis=1), [w.b3, w.b3], 1)
    fm = pa.pack_fm2t(fm2t_weights())
    nan = dnn3_weights()
    nan.w1[0, 0] = np.nan
    fm_hdr = struct.pack("<7If", 17, 16, 8, 1, 128, 64, 1, 0.0)
    dnn3_shape = "->1 unsupported (d_item 64 or 128; hidden widths 128-128, 256-128, 256-256, 512-256, 1024-512)"
    cases = [
        (pa.MODEL_DNN3, pa.PREC_BF16, dnn3_blob()[:-4], INVALID, "pg_model_load: DNN3 blob is 100368 bytes, expected 100372"),
        (pa.MODEL_DNN3_MULTI, pa.PREC_BF16, multi[:-4], INVALID, "pg_model_load: DNN3 blob is 100888 bytes, expected 100892"),
        (pa.MODEL_FM_TWOTOWER, pa.PREC_BF16, fm[:-4], INVALID, "pg_model_load: two-tower blob is 133760 bytes, expected 133764"),
        (pa.MODEL_DNN3, pa.PREC_BF16, struct.pack("<4I", 1, 64, 128, 256), UNSUPPORTED, "pg_model_load: DNN3 shape [1+64]->128->256" + dnn3_shape),
        (pa.MODEL_DNN3_MULTI, pa.PREC_BF16, struct.pack("<5I", 1, 64, 128, 128, 9), UNSUPPORTED,
         "pg_model_load: a multi-output DNN3 has 1..8 outputs, the blob says 9"),
        (pa.MODEL_FM_TWOTOWER, pa.PREC_BF16, fm_hdr, UNSUPPORTED,
         "pg_model_load: two-tower shape unsupported (1..16 user fields; item fields x k = 128 with k = 8, 16 or 32; towers 256-64 "
         "(k 16 / 32), 128-64 (k 8), 512-128 (k 16))"),
        (pa.MODEL_DNN3, pa.PREC_F16X2, dnn3_blob(nan), UNSUPPORTED,
         "pg_model_load: the blob holds a non-finite weight (float 0): not representable in an fp16 mode"),
    ]
    e = world["entries"]["pg_rank_dnn3"]
    for kind, prec, blob, code, text in cases:
        with pytest.raises(PgError) as ei:
            pa.RankModel(ctx, kind, prec, blob)
        assert ei.value.code == code and str(ei.value) == "pairec_gpu error %d: %s" % (code, text)
        m = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_BF16, dnn3_blob())        # a load that succeeds after a refused one
        try:
            assert np.array_equal(bits(e.host(handles=[m.h, world["t"].h])), bits(world["good"]["pg_rank_dnn3"]))
        finally:
            m.destroy()
