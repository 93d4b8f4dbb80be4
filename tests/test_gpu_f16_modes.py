"""GPU tests of PG_PREC_F16X2 / PG_PREC_F16 (pairec_amd/csrc/rank_2r.hip): the DNN3 matrix layers on the fp16 MFMA with
operands scaled by exact powers of two, against the FP32 oracle (prec = 0, nothing mirrored).

Bars: |score - fp32 oracle| <= 1e-5 (north_star), and, as a regression bar, <= 2 x the mode's emulated error
(tests/test_f16_modes_cpu.py: EMULATED; the factor 2 is for the fp32 accumulation order, which the emulation does not
model).  Data the fp16 range cannot carry — an activation past 65504 once scaled, inf, NaN — must come back exactly as a
PG_PREC_BF16X3 model scores it, tile by tile, and be counted (pg_model_f16_stats); calls outside the kernel's shapes are
served whole by the BF16X3 path, bit for bit."""
import os
import sys

import numpy as np
import pytest

import pairec_amd as pa
from oracle import oracle as o

pytestmark = pytest.mark.gpu

KERNEL_SHAPES = [(128, 128), (256, 128), (256, 256), (512, 256)]
TOL = 1e-5
EMULATED = {"f16x2": 3.0e-6, "f16": 3.7e-6}          # tests/test_f16_modes_cpu.py
MODES = ["f16x2", "f16"]
SIZES = [5000, 1, 0, 333, 128, 129, 64, 65, 127, 257]


def _prec(mode):
    return {"f16x2": pa.PREC_F16X2, "f16": pa.PREC_F16}[mode]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _blob(w):
    return pa.pack_dnn3(w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, 128)


def _requests(n, seed, sizes):
    rng = np.random.default_rng(seed)
    users = o.synth_rows(o.SEED_QUERY, 3, len(sizes), 128)
    cands = [rng.integers(0, n, s_).astype(np.uint32) for s_ in sizes]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    return users, cands, off


def _n_tiles(sizes):
    return sum((s_ + 127) // 128 for s_ in sizes)


@pytest.fixture(scope="module")
def world(ctx):
    """one 40 000-row table and, per kernel shape, the requests and the fp32 oracle's scores (1 head and several)"""
    n = 40_000
    t = pa.Table(ctx, n, 128)
    t.fill_synthetic(o.SEED_TABLE)
    tab = o.synth_rows(o.SEED_TABLE, 0, n, 128)
    cases = {}
    for h1, h2 in KERNEL_SHAPES:
        users, cands, off = _requests(n, h1 + h2, SIZES)
        w = o.Dnn3Weights(128, 128, h1, h2, seed=o.SEED_WEIGHTS ^ (h1 + h2))
        ref = np.concatenate([o.dnn3_forward(w, 0, users[r], tab[cands[r]]) for r in range(len(SIZES))])
        multi = []
        for n_out in (3, 2, 8) if (h1, h2) == (512, 256) else (3,):
            wm = o.Dnn3MultiWeights(n_out, 128, 128, h1, h2, seed=o.SEED_WEIGHTS ^ (h1 * 3 + n_out))
            rm = np.concatenate([o.dnn3_multi_forward(wm, 0, users[r], tab[cands[r]]) for r in range(len(SIZES))], axis=1)
            multi.append((wm, rm))
        cases[(h1, h2)] = (users, cands, off, w, ref, multi)
    yield t, tab, cases
    t.destroy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("h1,h2", KERNEL_SHAPES)
def test_fp16_modes_match_the_fp32_oracle(ctx, world, h1, h2, mode):
    t, tab, cases = world
    users, cands, off, w, ref, multi = cases[(h1, h2)]
    m = pa.RankModel(ctx, pa.MODEL_DNN3, _prec(mode), _blob(w))
    got = m.rank_dnn3(t, users, np.concatenate(cands), off)
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    st = m.f16_stats()
    print("%s %d-%d: max |d| vs the fp32 oracle %.3g (emulated %.3g)  %s" % (mode, h1, h2, err, EMULATED[mode], st))
    assert got.shape == ref.shape and err <= TOL, (mode, h1, h2, err)
    assert err <= 2 * EMULATED[mode], (mode, h1, h2, err)
    assert st == {"calls": 1, "tiles": _n_tiles(SIZES), "tiles_served_bf16x3": 0, "calls_served_bf16x3_whole": 0}
    m.destroy()
    for wm, rm in multi:
        mm = pa.RankModel(ctx, pa.MODEL_DNN3_MULTI, _prec(mode),
                          pa.pack_dnn3_multi(wm.w1, wm.b1, wm.w2, wm.b2, wm.w3m, wm.b3m, wm.d_user))
        gm = mm.rank_dnn3(t, users, np.concatenate(cands), off)
        assert gm.shape == (wm.n_out, int(off[-1]))
        errm = float(np.max(np.abs(gm.astype(np.float64) - rm)))
        print("%s %d-%d, %d heads: %.3g" % (mode, h1, h2, wm.n_out, errm))
        assert errm <= TOL and errm <= 2 * EMULATED[mode], (mode, h1, h2, wm.n_out, errm)
        assert mm.f16_stats()["tiles_served_bf16x3"] == 0
        mm.destroy()


@pytest.mark.parametrize("mode", MODES)
def test_fp16_modes_on_inputs_of_a_wide_dynamic_range(ctx, mode):
    """tests/test_gpu_bf16x3.py's construction — columns scaled by 2^-20 .. 2^12, layer 1 undoing it: the per-column
    factor carries it, no tile goes back to BF16X3."""
    n, d = 20_000, 128
    tab = o.synth_rows(o.SEED_TABLE, 0, n, d)
    scale = np.exp2(np.random.default_rng(11).integers(-20, 13, d)).astype(np.float32)
    tab_s = (tab * scale[None, :]).astype(np.float32)
    t = pa.Table(ctx, n, d)
    t.upload(tab_s)
    w = o.Dnn3Weights()
    w1 = w.w1.copy()
    w1[128:] = (w1[128:] / scale[:, None]).astype(np.float32)
    w.w1 = w1
    users, cands, off = _requests(n, 5, [3000, 500])
    m = pa.RankModel(ctx, pa.MODEL_DNN3, _prec(mode), _blob(w))
    got = m.rank_dnn3(t, users, np.concatenate(cands), off)
    ref = np.concatenate([o.dnn3_forward(w, 0, users[r], tab_s[cands[r]]) for r in range(2)])
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print("%s wide range: %.3g" % (mode, err))
    assert err <= TOL and err <= 2 * EMULATED[mode]
    assert m.f16_stats()["tiles_served_bf16x3"] == 0
    m.destroy()
    t.destroy()


@pytest.fixture(scope="module")
def hostile(ctx):
    """20 000 rows: 50 carry 1e9 in one column, six +-inf / NaN, the rest ordinary; a BF16X3 model beside the oracle"""
    n = 20_000
    tab = o.synth_rows(o.SEED_TABLE, 0, n, 128).copy()
    big = np.arange(100, 150)
    tab[big, 17] = 1e9
    odd = np.array([200, 201, 202, 203, 204, 205])
    tab[odd[0], 3] = np.inf
    tab[odd[1], 90] = -np.inf
    tab[odd[2], 0] = np.nan
    tab[odd[3], 127] = np.nan
    tab[odd[4], 64] = np.inf
    tab[odd[5], 64] = -np.inf
    bad = np.concatenate([big, odd])
    t = pa.Table(ctx, n, 128)
    t.upload(tab)
    w = o.Dnn3Weights()
    mx3 = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_BF16X3, _blob(w))
    yield t, tab, w, mx3, bad
    mx3.destroy()
    t.destroy()


def _check_hostile(ctx, hostile, mode, cands, sizes):
    """tiles holding a hostile row: a BF16X3 model's bits; every other item: the fp32 oracle to 1e-5; the count"""
    t, tab, w, mx3, bad = hostile
    users = o.synth_rows(o.SEED_QUERY, 3, len(sizes), 128)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    flat = np.concatenate(cands)
    is_bad = np.isin(flat, bad)
    in_bad_tile = np.zeros(flat.size, bool)
    n_bad_tiles = 0
    for r in range(len(sizes)):
        for b in range(int(off[r]), int(off[r + 1]), 128):
            e = min(b + 128, int(off[r + 1]))
            if is_bad[b:e].any():
                in_bad_tile[b:e] = True
                n_bad_tiles += 1
    m = pa.RankModel(ctx, pa.MODEL_DNN3, _prec(mode), _blob(w))
    got = m.rank_dnn3(t, users, flat, off)
    x3 = mx3.rank_dnn3(t, users, flat, off)
    st = m.f16_stats()
    m.destroy()
    assert np.array_equal(_bits(got[in_bad_tile]), _bits(x3[in_bad_tile]))
    with np.errstate(all="ignore"):
        ref = np.concatenate([o.dnn3_forward(w, 0, users[r], tab[cands[r]]) for r in range(len(sizes))])
    err = float(np.max(np.abs(got[~in_bad_tile].astype(np.float64) - ref[~in_bad_tile])))
    print("%s: %d of %d tiles re-served, other items within %.3g" % (mode, n_bad_tiles, _n_tiles(sizes), err))
    assert err <= TOL
    assert st["tiles"] == _n_tiles(sizes) and st["tiles_served_bf16x3"] == n_bad_tiles and st["calls_served_bf16x3_whole"] == 0
    return n_bad_tiles


@pytest.mark.parametrize("mode", MODES)
def test_out_of_range_and_non_finite_rows_are_served_in_bf16x3_tile_by_tile(ctx, hostile, mode):
    bad = hostile[4]
    rng = np.random.default_rng(8)
    sizes = [6000, 1500, 700]
    cands = [rng.integers(1000, 20_000, s_).astype(np.uint32) for s_ in sizes]      # ordinary rows only ...
    cands[0][128 * 3 + rng.permutation(128)[:30]] = bad[:30]                         # ... then the hostile ones, bunched
    cands[0][128 * 20 + 5] = bad[30]
    cands[0][128 * 41:128 * 41 + 10] = bad[31:41]
    cands[1][128 * 2 + 64:128 * 2 + 64 + 9] = bad[41:50]
    cands[1][128 * 11 + 91] = bad[50]                                                # (the short last tile)
    cands[2][np.array([0, 130, 300, 301, 699])] = bad[51:56]
    n_bad = _check_hostile(ctx, hostile, mode, cands, sizes)
    assert 0 < n_bad < _n_tiles(sizes) / 4


@pytest.mark.parametrize("mode", MODES)
def test_fallback_list_at_tile_boundaries(ctx, hostile, mode):
    """a hostile row as the first item of a tile, the last, the only one, and in a request's short last tile"""
    bad = hostile[4]
    rng = np.random.default_rng(9)
    sizes = [389, 129, 1, 256]
    cands = [rng.integers(1000, 20_000, s_).astype(np.uint32) for s_ in sizes]
    cands[0][0] = bad[0]          # first item of tile 0
    cands[0][255] = bad[50]       # last item of tile 1 (+inf)
    cands[0][386] = bad[1]        # the 5-item last tile
    cands[1][128] = bad[52]       # the only item of its tile (NaN)
    cands[2][0] = bad[2]          # a one-item request
    assert _check_hostile(ctx, hostile, mode, cands, sizes) == 5


@pytest.mark.parametrize("mode", MODES)
def test_calls_outside_the_kernel_are_served_whole_by_the_bf16x3_path(ctx, world, mode):
    t, tab, cases = world
    n = 40_000
    users, cands, off = _requests(n, 21, [700, 129, 1])
    flat = np.concatenate(cands)

    def pair(w):
        return pa.RankModel(ctx, pa.MODEL_DNN3, _prec(mode), _blob(w)), pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_BF16X3, _blob(w))
    # 1024-512
    m, mx3 = pair(o.Dnn3Weights(128, 128, 1024, 512))
    assert np.array_equal(_bits(m.rank_dnn3(t, users, flat, off)), _bits(mx3.rank_dnn3(t, users, flat, off)))
    assert m.f16_stats() == {"calls": 1, "tiles": 0, "tiles_served_bf16x3": 0, "calls_served_bf16x3_whole": 1}
    m.destroy(), mx3.destroy()
    # a 64-wide table
    t64 = pa.Table(ctx, n, 64)
    t64.fill_synthetic(o.SEED_TABLE)
    m, mx3 = pair(o.Dnn3Weights(128, 64, 512, 256))
    assert np.array_equal(_bits(m.rank_dnn3(t64, users, flat, off)), _bits(mx3.rank_dnn3(t64, users, flat, off)))
    assert m.f16_stats()["calls_served_bf16x3_whole"] == 1 and m.f16_stats()["tiles"] == 0
    m.destroy(), mx3.destroy()
    t64.destroy()
    # rank_no_ws
    m, mx3 = pair(o.Dnn3Weights())
    fast = m.rank_dnn3(t, users, flat, off)
    ctx.set_option("rank_no_ws", 1)
    try:
        general = m.rank_dnn3(t, users, flat, off)
        want = mx3.rank_dnn3(t, users, flat, off)
    finally:
        ctx.set_option("rank_no_ws", 0)
    assert np.array_equal(_bits(general), _bits(want))
    assert not np.array_equal(_bits(fast), _bits(general))             # (the first call did run the fp16 kernel)
    assert m.f16_stats() == {"calls": 2, "tiles": _n_tiles([700, 129, 1]), "tiles_served_bf16x3": 0, "calls_served_bf16x3_whole": 1}
    m.destroy(), mx3.destroy()


def test_recommend_step_and_coalescer_inherit_the_mode(ctx):
    """pg_recommend_dnn3 and a coalescer rank call reach rank_2r.hip through the same entry: the direct call's bits"""
    n, R, K = 300_000, 3, 200
    t = pa.Table(ctx, n, 128)
    t.fill_synthetic(o.SEED_TABLE)
    w = o.Dnn3Weights()
    m = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_F16X2, _blob(w))
    ex = pa.Expr("${gpu_dnn}*(1+${current_score})^0.1")
    q = o.synth_rows(o.SEED_QUERY, 0, R, 128)
    rows, rec, rnk, fus, order, cnt = pa.recommend_dnn3(ctx, t, m, ex, "gpu_dnn", q, K)
    assert list(cnt) == [K] * R
    off = (np.arange(R + 1) * K).astype(np.uint32)
    direct = m.rank_dnn3(t, q, rows.reshape(-1).astype(np.uint32), off).reshape(R, K)
    assert np.array_equal(_bits(rnk), _bits(direct))
    co = pa.Coalescer(ctx, t, K, m, max_rank_items=K, max_wait_us=200)
    one = co.rank_dnn3(q[1], rows[1].astype(np.uint32))
    co.destroy()
    assert np.array_equal(_bits(one), _bits(direct[1]))
    st = m.f16_stats()
    assert st["calls"] == 3 and st["tiles"] == 2 * R + 2 * R + 2 and st["tiles_served_bf16x3"] == 0 and st["calls_served_bf16x3_whole"] == 0
    m.destroy()
    t.destroy()


@pytest.mark.parametrize("mode", MODES)
def test_what_an_fp16_mode_refuses(ctx, mode):
    fw = o.Fm2tWeights(vocab=300)
    with pytest.raises(pa._lib.PgError) as e:
        pa.RankModel(ctx, pa.MODEL_FM_TWOTOWER, _prec(mode), pa.pack_fm2t(fw))
    assert e.value.code == -4 and "PG_MODEL_FM_TWOTOWER" in str(e.value)
    for where in ("w1", "w2", "b2"):
        w = o.Dnn3Weights(128, 128, 128, 128)
        getattr(w, where).reshape(-1)[5] = np.inf if where != "w2" else np.nan
        with pytest.raises(pa._lib.PgError) as e:
            pa.RankModel(ctx, pa.MODEL_DNN3, _prec(mode), _blob(w))
        assert e.value.code == -4 and "non-finite" in str(e.value)
    # a zero row in either matrix is fine (scale exponent 0)
    w = o.Dnn3Weights(128, 128, 128, 128)
    w.w1[128 + 9, :] = 0.0
    w.w2[77, :] = 0.0
    tab = o.synth_rows(o.SEED_TABLE, 0, 2000, 128)
    t = pa.Table(ctx, 2000, 128)
    t.fill_synthetic(o.SEED_TABLE)
    users, cands, off = _requests(2000, 1, [300])
    m = pa.RankModel(ctx, pa.MODEL_DNN3, _prec(mode), _blob(w))
    got = m.rank_dnn3(t, users, cands[0], off)
    assert np.max(np.abs(got.astype(np.float64) - o.dnn3_forward(w, 0, users[0], tab[cands[0]]))) <= TOL
    assert m.f16_stats()["tiles_served_bf16x3"] == 0
    m.destroy()
    t.destroy()


@pytest.mark.parametrize("mode", MODES)
def test_fp16_page_order_against_the_f32_mode(ctx, mode):
    """bench.precision_figures on a small table.  fp16's ~3e-6 reorders near-ties that BF16X3's 1e-7 does not: the order
    fractions are printed (DESIGN.md §4.2 records them), only the page SET is held for F16X2."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    n, d, R, K = 300_000, 128, 48, 2000
    t = pa.Table(ctx, n, d)
    t.fill_synthetic(o.SEED_TABLE)
    w = o.Dnn3Weights()
    mh, m32 = pa.RankModel(ctx, pa.MODEL_DNN3, _prec(mode), _blob(w)), pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_F32, _blob(w))
    ex = pa.Expr(bench.RANK_EXPR)
    q = o.synth_rows(o.SEED_QUERY, 0, R, d)
    f = bench.precision_figures(pa, ctx, t, ex, mh, m32, q, K, page=100, tau_requests=12)
    print("%s vs f32:" % mode, {k_: v for k_, v in f.items() if k_ != "note"})
    assert f["items"] == R * K
    assert f["max_abs_dscore"] <= TOL
    if mode == "f16x2":
        assert f["frac_requests_page_set_unchanged"] >= 0.9
    assert mh.f16_stats()["tiles_served_bf16x3"] == 0
    for m in (mh, m32):
        m.destroy()
    t.destroy()
