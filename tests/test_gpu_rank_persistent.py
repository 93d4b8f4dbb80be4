"""GPU tests of the persistent rank kernels past one tile per workgroup.  Every fast rank kernel launches one workgroup per
CU (two for the small register-stationary shapes) and lets workgroup b walk the tiles [n_tiles * b / G, n_tiles * (b + 1) / G):
descriptors prefetched three tiles ahead, row ids two, table rows one; the request's layer-1 partial reloaded when the
request changes inside the range; a partial tile followed by a full one; the head of a tile finished under the next one's
first layer (rank_2r.hip); waves striding by eight (rank_is.hip); the fp16 modes' fallback list appended by every workgroup.
The other rank tests give a workgroup zero tiles or one.  Here:

    kernel  model / precision                                   tile items  workgroups G     items (14 x G tiles and more)
    ws      DNN3 512-256, BF16                                   64          CUs              ~233 K
    rs      128-128, 256-128 (two per CU), 256-256 (one), BF16   64          CUs x 2 / CUs    ~460 K / ~233 K
    ls      1024-512, BF16                                       128         CUs              ~459 K
    x3      128-128, 256-128, 256-256, 512-256, BF16X3           128         CUs              ~459 K
    h2      the same four, F16X2 and F16                         128         CUs              ~459 K
    isw     FM2T 256-64, k 16, 8 item fields, BF16, ItemRows     32          CUs (8 waves)    ~197 K (24 x G tiles and more)

(figures for 256 CUs; G comes from the device).  14 tiles per workgroup rather than the 5 a steady-state loop needs: the run
of twelve 1-item requests has to fit inside one workgroup's range.  The batches and the conditions they meet — at least 5
tiles in every range (3 per wave for isw), a request change in a quarter of the ranges, a partial tile before a full one in
16, the 1-item run inside one range, ranges that start and end with a partial tile — are tests/rank_tiles_ref.py's, shown
on the CPU for G = 256 / 512 by tests/test_rank_tiles_cpu.py and asserted here for the device's G.

Every case:
  a  the kernel's rank_*_calls counter of pg_stats, and no other, moves by the number of calls made
  b  the oracle on a stratified sample (rank_tiles_ref.sample_items: first / last tiles of 16 ranges, the 1-item run, the
     tiles around the empty run, partial-then-full tiles of 16 ranges, 2 000 random items), at the project's tolerances:
     BF16 1e-5 against the mirrored oracle, BF16X3 test_gpu_bf16x3.OBSERVED, fp16 min(1e-5, 2 x test_gpu_f16_modes.EMULATED)
     against the fp32 oracle, FM2T BF16 1e-5
  c  every item and head, bit for bit, against the same requests ranked in calls of at most G tiles (zero tiles or one per
     workgroup: the regime the other files hold to the oracle in full; for isw that is one tile for a workgroup's first wave).
     An item's arithmetic does not depend on the tile slot or loop trip it lands in, so any difference is a kernel bug; the
     failure names workgroup and position in its range
  d  once per family, a multi-output model (3 heads; 8 for ws, whose head partials live in per-workgroup scratch) through b, c
  e  fp16 modes: on a table whose first 1 % of rows leave the fp16 range (1e9, inf, NaN), tiles holding such a row equal a
     BF16X3 model's bits, the sample elsewhere meets b, and pg_model_f16_stats counts exactly numpy's tiles

and once: the tile table at 8192 requests (build_tiles_wide_kernel's last) and 8193 (build_tiles_kernel's first), and the
general mlp_kernel's counter."""
import subprocess
import sys
import time
from collections import namedtuple

import numpy as np
import pytest

import pairec_amd as pa
from oracle import oracle as o

import rank_tiles_ref as rt
from test_gpu_bf16x3 import OBSERVED
from test_gpu_f16_modes import EMULATED

pytestmark = pytest.mark.gpu

N_ROWS = 40_000
N_BAD = N_ROWS // 100         # table `hostile`: rows [0, N_BAD) leave the fp16 range
KINDS = ("rank_ws_calls", "rank_rs_calls", "rank_ls_calls", "rank_x3_calls", "rank_h2_calls", "rank_isw_calls", "rank_mlp_calls")
TILE_ITEMS = {"ws": 64, "rs": 64, "ls": 128, "x3": 128, "h2": 128, "isw": 32}
PREC = {"bf16": pa.PREC_BF16, "bf16x3": pa.PREC_BF16X3, "f16x2": pa.PREC_F16X2, "f16": pa.PREC_F16}
TOL = {"bf16": 1e-5, "bf16x3": OBSERVED, "f16x2": min(1e-5, 2 * EMULATED["f16x2"]), "f16": min(1e-5, 2 * EMULATED["f16"])}

Case = namedtuple("Case", "kernel h1 h2 mode heads")
X3_SHAPES = [(128, 128), (256, 128), (256, 256), (512, 256)]
CASES = ([Case("ws", 512, 256, "bf16", 1), Case("ws", 512, 256, "bf16", 8),
          Case("rs", 128, 128, "bf16", 1), Case("rs", 256, 128, "bf16", 1), Case("rs", 256, 256, "bf16", 1),
          Case("rs", 256, 128, "bf16", 3),
          Case("ls", 1024, 512, "bf16", 1), Case("ls", 1024, 512, "bf16", 3)]
         + [Case("x3", h1, h2, "bf16x3", 1) for h1, h2 in X3_SHAPES] + [Case("x3", 512, 256, "bf16x3", 3)]
         + [Case("h2", h1, h2, mode, 1) for h1, h2 in X3_SHAPES for mode in ("f16x2", "f16")]
         + [Case("h2", 256, 256, "f16x2", 3)])


def _id(c):
    return "%s-%d-%d-%s%s" % (c.kernel, c.h1, c.h2, c.mode, "-%dheads" % c.heads if c.heads > 1 else "")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def counters(ctx):
    s = ctx.stats()
    return {k: getattr(s, k) for k in KINDS + ("rank_calls",)}


def counted(ctx, kind, by, call):
    """call() with the assertion that `by` launch sequences of `kind`, and no other rank kernel, served it"""
    before = counters(ctx)
    got = call()
    after = counters(ctx)
    moved = {k: after[k] - before[k] for k in KINDS}
    assert moved == {k: (by if k == kind else 0) for k in KINDS}, moved
    assert after["rank_calls"] - before["rank_calls"] == by
    assert sum(after[k] for k in KINDS) == after["rank_calls"]
    return got


def workgroups(case, cus):
    return cus * (2 if case.kernel == "rs" and case.h2 == 128 else 1)      # rank_rs.hip: launch_dnn3_rs


def device_cus():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked of a short-lived child: torch brings a HIP runtime
    of its own, which finds no device in a process where the library's has already opened it"""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout.split()[-1])


@pytest.fixture(scope="module")
def world(ctx):
    cus = device_cus()
    t = pa.Table(ctx, N_ROWS, 128)
    t.fill_synthetic(o.SEED_TABLE)
    tab = o.synth_rows(o.SEED_TABLE, 0, N_ROWS, 128)
    bad = tab.copy()                                       # test_gpu_f16_modes.py's hostile rows, on 1 % of the table
    bad[:N_BAD, 17] = 1e9
    bad[3, 3], bad[5, 90], bad[7, 0], bad[11, 127], bad[13, 64], bad[17, 64] = np.inf, -np.inf, np.nan, np.nan, np.inf, -np.inf
    hostile = pa.Table(ctx, N_ROWS, 128)
    hostile.upload(bad)
    batches = {}

    def batch(tile_items, G, waves=1, n_rows=N_ROWS):
        """the (tile_items, G) batch with its candidates, users, chunks and sample: built once, shared, left unchanged"""
        key = (tile_items, G, waves)
        if key not in batches:
            seed, b, tt = rt.batch_for(tile_items, G, waves)
            if seed is None:
                pytest.skip("no seed below %d gives a batch that meets the coverage conditions for %d workgroups of this "
                            "device (%d-item tiles): %s" % (rt.MAX_SEED, G, tile_items, "; ".join(tt)))
            assert rt.check_coverage(b, tt, G, waves) == []
            rng = np.random.default_rng(1000 + seed)
            n = int(b.offsets[-1])
            batches[key] = {"batch": b, "tt": tt, "off": b.offsets, "n": n, "G": G, "waves": waves,
                            "cand": rng.integers(0, n_rows, n).astype(np.uint32),
                            "users": o.synth_rows(o.SEED_QUERY, 3, b.sizes.size, 128),
                            "chunks": [c for c in rt.chunks(b.sizes, tile_items, G) if b.offsets[c[1]] > b.offsets[c[0]]],
                            "sample": rt.sample_items(b, tt, G, seed=seed), "ref": {}}
            for v in batches[key].values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        return batches[key]
    yield {"t": t, "tab": tab, "hostile": hostile, "cus": cus, "batch": batch}
    hostile.destroy()
    t.destroy()


def by_request(off, sample):
    """[(request, positions in `sample` of its items)]"""
    req = np.searchsorted(off, sample, side="right") - 1
    cut = np.nonzero(np.diff(req))[0] + 1
    return [(int(req[p[0]]), p) for p in np.split(np.arange(sample.size), cut)]


def same_bits(big, small, d, what):
    """check c: every item and head of the big call against the chunked calls"""
    big, small = np.atleast_2d(big), np.atleast_2d(small)
    assert big.shape == small.shape
    diff = np.nonzero(np.any(bits(big) != bits(small), axis=0))[0]
    if diff.size:
        where = [rt.locate(d["tt"], d["G"], i, d["waves"]) for i in diff[:8]]
        tiles = np.unique(np.searchsorted(d["tt"].tile_item0, diff, side="right") - 1)
        pytest.fail("%s: %d of %d items (in %d tiles) differ between one call and calls of at most one tile per workgroup; "
                    "first: %s; big %s small %s" % (what, diff.size, big.shape[1], tiles.size, where,
                                                    big[:, diff[:4]].tolist(), small[:, diff[:4]].tolist()))


def rank_chunks(d, call):
    off = d["off"].astype(np.int64)
    return np.concatenate([np.atleast_2d(call(r0, r1, int(off[r0]), int(off[r1]), (off[r0:r1 + 1] - off[r0]).astype(np.uint32)))
                           for r0, r1 in d["chunks"]], axis=1)


def weights(case):
    if case.heads > 1:
        w = o.Dnn3MultiWeights(case.heads, 128, 128, case.h1, case.h2, seed=o.SEED_WEIGHTS ^ (case.h1 * 3 + case.heads))
        return w, pa.pack_dnn3_multi(w.w1, w.b1, w.w2, w.b2, w.w3m, w.b3m, w.d_user), pa.MODEL_DNN3_MULTI
    w = o.Dnn3Weights(128, 128, case.h1, case.h2, seed=o.SEED_WEIGHTS ^ (case.h1 + case.h2))
    return w, pa.pack_dnn3(w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, 128), pa.MODEL_DNN3


def oracle_on_sample(d, w, prec, tab, heads):
    """[heads][sample]: computed once per (shape, oracle precision, heads) and shared (h2's two modes, x3)"""
    key = (w.h1, w.h2, prec, heads)
    if key not in d["ref"]:
        ref = np.empty((heads, d["sample"].size), np.float32)
        fwd = o.dnn3_multi_forward if heads > 1 else o.dnn3_forward
        for r, pos in by_request(d["off"], d["sample"]):
            ref[:, pos] = fwd(w, prec, d["users"][r], tab[d["cand"][d["sample"][pos]]])
        ref.setflags(write=False)
        d["ref"][key] = ref
    return d["ref"][key]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_dnn3_kernel_over_many_tiles_per_workgroup(ctx, world, case):
    t_start = time.perf_counter()
    t, tab = world["t"], world["tab"]
    G = workgroups(case, world["cus"])
    d = world["batch"](TILE_ITEMS[case.kernel], G)
    kind = "rank_%s_calls" % case.kernel
    users, cand, off, sample = d["users"], d["cand"], d["off"], d["sample"]
    w, blob, model_kind = weights(case)
    m = pa.RankModel(ctx, model_kind, PREC[case.mode], blob)
    # a + the big call
    big = np.atleast_2d(counted(ctx, kind, 1, lambda: m.rank_dnn3(t, users, cand, off)))
    assert big.shape == (case.heads, d["n"])
    # b
    ref = oracle_on_sample(d, w, 1 if case.mode == "bf16" else 0, tab, case.heads)
    err = float(np.max(np.abs(big[:, sample].astype(np.float64) - ref)))
    print("%s: %d items, %d tiles over %d workgroups; max |d| vs the oracle on %d sampled items %.3g (tolerance %.3g)"
          % (_id(case), d["n"], d["tt"].tile_req.size, G, sample.size, err, TOL[case.mode]))
    # c (before b's verdict: a difference is located by workgroup and position, which says more than an error figure)
    small = counted(ctx, kind, len(d["chunks"]), lambda: rank_chunks(
        d, lambda r0, r1, i0, i1, o_: m.rank_dnn3(t, users[r0:r1], cand[i0:i1], o_)))
    same_bits(big, small, d, _id(case))
    assert err <= TOL[case.mode], (_id(case), err)
    if case.kernel == "h2":
        st = m.f16_stats()
        n_tiles = int(d["tt"].tile_req.size)
        assert st == {"calls": 1 + len(d["chunks"]), "tiles": 2 * n_tiles, "tiles_served_bf16x3": 0, "calls_served_bf16x3_whole": 0}
        if case.heads == 1:
            # e
            hostile = world["hostile"]
            mx3 = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_BF16X3, blob)
            got = counted(ctx, kind, 1, lambda: m.rank_dnn3(hostile, users, cand, off))
            x3 = counted(ctx, "rank_x3_calls", 1, lambda: mx3.rank_dnn3(hostile, users, cand, off))
            mx3.destroy()
            tt = d["tt"]
            bad_tile = np.add.reduceat((cand < N_BAD).astype(np.int64), tt.tile_item0) > 0
            in_bad_tile = np.repeat(bad_tile, tt.tile_cnt)
            tb, te = rt.ranges(n_tiles, G)
            marked = np.add.reduceat(bad_tile.astype(np.int64), tb)
            assert np.sum((marked > 0) & (marked < te - tb)) >= G // 2      # marked and unmarked tiles within most ranges
            assert np.array_equal(bits(got[in_bad_tile]), bits(x3[in_bad_tile]))
            clean = ~in_bad_tile[sample]
            err_h = float(np.max(np.abs(got[sample][clean].astype(np.float64) - ref[0][clean])))
            print("%s, hostile rows: %d of %d tiles served in bf16x3, %d sampled items elsewhere within %.3g"
                  % (_id(case), int(bad_tile.sum()), n_tiles, int(clean.sum()), err_h))
            assert clean.sum() >= 500 and err_h <= TOL[case.mode]
            st2 = m.f16_stats()
            assert st2["tiles"] - st["tiles"] == n_tiles and st2["tiles_served_bf16x3"] == int(bad_tile.sum())
            assert st2["calls_served_bf16x3_whole"] == 0
    m.destroy()
    print("%s: %.2f s" % (_id(case), time.perf_counter() - t_start))


def test_fm2t_per_wave_kernel_over_many_tiles_per_wave(ctx, world):
    """isw: FM + two-tower 256-64, k = 16, 8 item fields, BF16, over materialised item records — every wave of every
    workgroup three tiles and more; the chunked calls give a workgroup's first wave one tile."""
    t_start = time.perf_counter()
    G, vocab, n_store = world["cus"], 3000, 20_000
    d = world["batch"](TILE_ITEMS["isw"], G, rt.IS_WAVES, n_store)
    users, cand, off, sample = d["users"], d["cand"], d["off"], d["sample"]
    fw = o.Fm2tWeights(vocab=vocab)
    m = pa.RankModel(ctx, pa.MODEL_FM_TWOTOWER, pa.PREC_BF16, pa.pack_fm2t(fw))
    rng = np.random.default_rng(4)
    ufids = rng.integers(0, vocab, (users.shape[0], 8)).astype(np.int32)
    cols = rng.integers(0, vocab, (n_store, 8)).astype(np.int32)
    fs = pa.Features(ctx, n_store)
    names = ["f%d" % f for f in range(8)]
    for f in range(8):
        fs.set_column(names[f], pa.F_I32, cols[:, f].copy(), default=0)
    ir = pa.ItemRows(m, fs, names)
    big = counted(ctx, "rank_isw_calls", 1, lambda: ir.rank(users, ufids, cand, off))
    ref = np.empty(sample.size, np.float32)
    for r, pos in by_request(off, sample):
        ref[pos] = o.fm2t_forward(fw, 1, users[r], ufids[r], cols[cand[sample[pos]]])
    err = float(np.max(np.abs(big[sample].astype(np.float64) - ref)))
    print("isw: %d items, %d tiles over %d workgroups x %d waves; max |d| vs the oracle on %d sampled items %.3g (tolerance 1e-5)"
          % (d["n"], d["tt"].tile_req.size, G, rt.IS_WAVES, sample.size, err))
    small = counted(ctx, "rank_isw_calls", len(d["chunks"]), lambda: rank_chunks(
        d, lambda r0, r1, i0, i1, o_: ir.rank(users[r0:r1], ufids[r0:r1], cand[i0:i1], o_)))
    same_bits(big, small, d, "isw")
    assert err <= 1e-5
    # the per-field path is the general kernel's
    r0, r1 = d["chunks"][0]
    i1 = int(off[r1])
    per_field = counted(ctx, "rank_mlp_calls", 1, lambda: m.rank_fm2t(users[:r1], ufids[:r1], cols[cand[:i1]], off[:r1 + 1]))
    assert np.array_equal(bits(per_field), bits(big[:i1]))
    ir.destroy()
    fs.destroy()
    m.destroy()
    print("isw: %.2f s" % (time.perf_counter() - t_start))


def test_general_kernel_is_counted(ctx, world):
    """rank_no_ws and a 64-wide table take mlp_kernel, whatever fast kernel the shape has"""
    t, tab = world["t"], world["tab"]
    rng = np.random.default_rng(6)
    sizes = [700, 129, 0, 1]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    users = o.synth_rows(o.SEED_QUERY, 3, len(sizes), 128)
    cand = rng.integers(0, 20_000, int(off[-1])).astype(np.uint32)
    w = o.Dnn3Weights()
    blob = pa.pack_dnn3(w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, 128)
    ref = np.concatenate([o.dnn3_forward(w, 1, users[r], tab[cand[off[r]:off[r + 1]]]) for r in range(len(sizes))])
    m = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_BF16, blob)
    fast = counted(ctx, "rank_ws_calls", 1, lambda: m.rank_dnn3(t, users, cand, off))
    ctx.set_option("rank_no_ws", 1)
    try:
        general = counted(ctx, "rank_mlp_calls", 1, lambda: m.rank_dnn3(t, users, cand, off))
    finally:
        ctx.set_option("rank_no_ws", 0)
    assert np.max(np.abs(fast.astype(np.float64) - ref)) <= 1e-5 and np.max(np.abs(general.astype(np.float64) - ref)) <= 1e-5
    m.destroy()
    t64 = pa.Table(ctx, 20_000, 64)
    t64.fill_synthetic(o.SEED_TABLE)
    tab64 = o.synth_rows(o.SEED_TABLE, 0, 20_000, 64)
    w64 = o.Dnn3Weights(128, 64, 512, 256)
    m = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_BF16, pa.pack_dnn3(w64.w1, w64.b1, w64.w2, w64.b2, w64.w3, w64.b3, 128))
    got = counted(ctx, "rank_mlp_calls", 1, lambda: m.rank_dnn3(t64, users, cand, off))
    ref = np.concatenate([o.dnn3_forward(w64, 1, users[r], tab64[cand[off[r]:off[r + 1]]]) for r in range(len(sizes))])
    assert np.max(np.abs(got.astype(np.float64) - ref)) <= 1e-5
    before = counters(ctx)
    assert m.rank_dnn3(t64, users[:2], cand[:0], [0, 0, 0]).size == 0            # nothing to rank: nothing launched, nothing counted
    assert counters(ctx) == before
    m.destroy()
    t64.destroy()


def test_tile_table_beyond_8192_requests(ctx, world):
    """8192 requests: the many-workgroup tile table's last (prefix searched in LDS); 8193: the one-workgroup table's first
    (prefix searched in global memory).  0 … 3 items a request, runs of empty ones, an empty first and last request; DNN3
    128-128 through the general kernel (F32, 128-item tiles) and the register-stationary one (BF16, 64-item tiles), every
    item against the oracle."""
    t, tab = world["t"], world["tab"]
    rng = np.random.default_rng(8192)
    sizes = rng.integers(0, 4, 8193)
    for r0 in rng.integers(1, 8000, 12):
        sizes[r0:r0 + int(rng.integers(2, 40))] = 0                             # runs of empty requests
    sizes[0], sizes[1], sizes[8190], sizes[8191], sizes[8192] = 0, 2, 0, 3, 0
    at_limit = sizes[:8192].copy()
    at_limit[8191] = 0                                                          # (8192 requests, the last one empty too)
    users = o.synth_rows(o.SEED_QUERY, 3, 8193, 128)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(off[-1])
    n_limit = int(at_limit.sum())
    assert n_limit == n - 3 and 10_000 <= n <= 14_000
    cand = rng.integers(0, N_ROWS, n).astype(np.uint32)
    off_limit = np.concatenate([[0], np.cumsum(at_limit)]).astype(np.uint32)
    w = o.Dnn3Weights(128, 128, 128, 128, seed=o.SEED_WEIGHTS ^ 256)
    blob = pa.pack_dnn3(w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, 128)
    for prec, tol, kind in ((pa.PREC_F32, 2e-7, "rank_mlp_calls"), (pa.PREC_BF16, 1e-5, "rank_rs_calls")):
        # (the 8192-request call ranks the first n - 3 of the same candidates for the same users: one reference serves both)
        ref = np.zeros(n, np.float32)
        for r in np.nonzero(sizes)[0]:
            ref[off[r]:off[r + 1]] = o.dnn3_forward(w, prec, users[r], tab[cand[off[r]:off[r + 1]]], 1)
        m = pa.RankModel(ctx, pa.MODEL_DNN3, prec, blob)
        got_limit = counted(ctx, kind, 1, lambda: m.rank_dnn3(t, users[:8192], cand[:n_limit], off_limit))
        got = counted(ctx, kind, 1, lambda: m.rank_dnn3(t, users, cand, off))
        m.destroy()
        e_limit = float(np.max(np.abs(got_limit.astype(np.float64) - ref[:n_limit])))
        e = float(np.max(np.abs(got.astype(np.float64) - ref)))
        print("prec %d: 8192 requests %.3g, 8193 requests %.3g (tolerance %.3g), %d items" % (prec, e_limit, e, tol, n))
        assert got_limit.shape == (n_limit,) and got.shape == (n,)
        assert e_limit <= tol and e <= tol
