"""Cost of pg_rank_gbdt_dev (csrc/rank_gbdt.hip) at a serving shape: 500 trees of depth 6 over 32 user + 32 item features, the
feature store at 1 M rows, for 256 requests x 5000 candidates (the wide tile) and for 1 request x 5000 (the one-wave tile).

Each shape is first checked against tests/gbdt_ref.py on a seeded sample of its candidates (objective 1: bit-equal), then warmed
up and timed with device events around windows of back-to-back calls, each window sized from a trial to last about a second.

Reported per shape: ms per call (median window), node visits per second (items x trees x depth over the time) and that rate beside
the LDS ISSUE BOUND of the design: a visit is one ds_read_b64 (64 lanes x 8 B) and one ds_read_b32 (64 x 4 B), a tree one more
ds_read_b32 for its leaf; at 128 bytes per clock and CU that is 6 clocks per visit and 2 per tree for a wave of 64 candidates, with
CUS compute units at CLOCK_HZ.  The bound counts no bank conflict among the node reads, no chunk store and no feature gather.
Prints one JSON document, and writes it to the path given as the first argument, if any."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pairec_amd as pa  # noqa: E402
from gbdt_ref import gbdt_margins  # noqa: E402

STORE, N_USER, N_ITEM, TREES, DEPTH, CAND = 1_000_000, 32, 32, 500, 6, 5000
CUS, CLOCK_HZ, LDS_BYTES_PER_CLK = 256, 2.4e9, 128
DTYPES = (pa.F_F32, pa.F_F64, pa.F_I64, pa.F_I32)
NP = {pa.F_F32: np.float32, pa.F_F64: np.float64, pa.F_I64: np.int64, pa.F_I32: np.int32}


def full_tree(rng):
    """a complete pointer tree of DEPTH in heap order"""
    nn = 2 ** DEPTH - 1
    idx = np.arange(2 * nn + 1)
    return {"feature": np.r_[rng.integers(0, N_USER + N_ITEM, nn), np.zeros(nn + 1, int)], "threshold": rng.standard_normal(2 * nn + 1).astype(np.float32),
            "left": np.where(idx < nn, 2 * idx + 1, -1), "right": np.where(idx < nn, 2 * idx + 2, -1), "missing_left": rng.integers(0, 2, 2 * nn + 1),
            "value": (0.05 * rng.standard_normal(2 * nn + 1)).astype(np.float32)}


def lds_bound_visits_per_s():
    clocks_per_wave_tree = DEPTH * (64 * 8 + 64 * 4) / LDS_BYTES_PER_CLK + 64 * 4 / LDS_BYTES_PER_CLK
    return CUS * CLOCK_HZ * 64 * DEPTH / clocks_per_wave_tree


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rng = np.random.default_rng(5)
    trees = [full_tree(rng) for _ in range(TREES)]
    blob = pa.pack_gbdt(trees, N_USER, N_ITEM, 0.1, 1)
    cols = [rng.standard_normal(STORE).astype(NP[DTYPES[k % 4]]) if k % 4 < 2 else rng.integers(-3, 4, STORE).astype(NP[DTYPES[k % 4]]) for k in range(N_ITEM)]
    out = {"store_rows": STORE, "features": [N_USER, N_ITEM], "trees": TREES, "depth": DEPTH, "lds_bound_visits_per_s": lds_bound_visits_per_s(),
           "bound": "LDS issue: 6 clocks per visit + 2 per tree and wave at %d B/clk/CU, %d CUs, %.1f GHz" % (LDS_BYTES_PER_CLK, CUS, CLOCK_HZ / 1e9), "shapes": {}}
    stream = torch.cuda.Stream()
    with pa.Context(0, stream=stream.cuda_stream) as ctx:
        fs = pa.Features(ctx, STORE)
        for k, v in enumerate(cols):
            fs.set_column("c%d" % k, DTYPES[k % 4], v)
        names = ["c%d" % k for k in range(N_ITEM)]
        m = pa.RankModel(ctx, pa.MODEL_GBDT, pa.PREC_F32, blob)
        for n_req in (256, 1):
            n = n_req * CAND
            users = rng.standard_normal((n_req, N_USER)).astype(np.float32)
            cand = rng.integers(0, STORE, n).astype(np.uint32)
            off = (np.arange(n_req + 1) * CAND).astype(np.uint32)
            d_u, d_c, d_o, d_s = ctx.to_device(users), ctx.to_device(cand), ctx.to_device(off), ctx.malloc(n * 4)
            call = lambda: m.rank_gbdt_dev(fs, names, d_u, d_c, d_o, n_req, n, d_s)   # noqa: E731
            call()
            got = np.empty(n, dtype=np.float32)
            ctx.d2h(got, d_s)
            pick = rng.choice(n, 4096, replace=False)
            x = np.concatenate([users[pick // CAND], np.stack([c[cand[pick]].astype(np.float32) for c in cols], axis=1)], axis=1)
            want = gbdt_margins(trees, 0.1, x).astype(np.float32)
            assert np.array_equal(got[pick].view(np.uint32), want.view(np.uint32)), "scores differ from gbdt_ref at %d x %d" % (n_req, CAND)

            def window(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(reps):
                    call()
                e1.record(stream)
                ctx.synchronize()
                return e0.elapsed_time(e1) / reps
            window(20)                                                                  # warm-up
            reps = max(20, int(1000.0 / window(20)))
            ms = [window(reps) for _ in range(5)]
            med = statistics.median(ms)
            rate = n * TREES * DEPTH / (med * 1e-3)
            out["shapes"]["%dx%d" % (n_req, CAND)] = {"ms_per_call": med, "ms_windows": ms, "calls_per_window": reps, "node_visits_per_s": rate,
                                                      "share_of_lds_bound": rate / out["lds_bound_visits_per_s"], "checked_bit_equal": len(pick)}
            print(n_req, out["shapes"]["%dx%d" % (n_req, CAND)], flush=True)
            for p in (d_u, d_c, d_o, d_s):
                ctx.free(p)
        m.destroy()
        fs.destroy()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
