"""Developer aid (GPU box): the exact IVF index (pg_index_*) against the table's own pass, one JSON line.
   python scripts/dev/index_sweep.py [rows] [reps] [n_lists]
   python scripts/dev/index_sweep.py [rows] [reps] breakeven
Tables: mixtures of 1 000 centres at sigma 0.3 / 0.1 / 0.03 and the uniform synthetic table, dim 128.  Per table: build ms,
radii, and for R in {1, 8, 32, 64, 256} queries at K = 5 000 the index recall's median ms beside pg_recall_topk_dev's in the same
process, the (row, query) pairs the index scored per (R x rows) and its fallbacks.  `breakeven`: the mixture at sigma 0.3 through
indexes of few, wide lists (100 and 1 000) with the dense rule lifted — the index's cost where it scores 0.5-10 % of the table per
query, beside the pass: what the default of index_dense_fraction is set from.  Spot-checks exactness against the table's
pass on every R (ids and score bits)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

import pairec_amd as pa  # noqa: E402
from oracle import oracle as o  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
breakeven = len(sys.argv) > 3 and sys.argv[3] == "breakeven"
n_lists = int(sys.argv[3]) if len(sys.argv) > 3 and not breakeven else 0
D, K, CENTRES, SEED = 128, 5000, 1000, 0x5EED0007
RS = (1, 8, 32, 64, 256)

ctx = pa.Context(0)
d_rows = ctx.malloc(256 * K * 8)
d_sc = ctx.malloc(256 * K * 4)
d_rows2 = ctx.malloc(256 * K * 8)
d_sc2 = ctx.malloc(256 * K * 4)


def timed(fn):
    ms = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


out = {"rows": rows, "dim": D, "k": K, "reps": reps, "tables": []}
legs = [("mixture_s0.3", 0.3, n_lists), ("mixture_s0.1", 0.1, n_lists), ("mixture_s0.03", 0.03, n_lists), ("uniform", None, n_lists)]
if breakeven:
    out["breakeven"] = True
    ctx.set_option("index_dense_fraction", 1e9)
    legs = [("mixture_s0.3", 0.3, 100), ("mixture_s0.3", 0.3, 1000)]
last = None
for name, sigma, nl in legs:
    if last is None or last[0] != name:
        if last is not None:
            last[1].destroy()
        t = pa.Table(ctx, rows, D)
        if sigma is None:
            t.fill_synthetic(o.SEED_TABLE)
        else:
            t.fill_mixture(SEED, CENTRES, sigma)
        ctx.synchronize()
        last = (name, t)
    ix = pa.Index(ctx, t, n_lists=nl)
    st = ix.stats()
    rec = {"table": name, "build_ms": round(st["build_ms"], 1), "n_lists": st["n_lists"], "max_radius": st["max_radius"],
           "mean_radius": st["mean_radius"], "largest_list": st["largest_list"], "runs": []}
    for R in RS:
        if sigma is None:
            q = o.synth_rows(o.SEED_QUERY, 1000 * R, R, D)
        else:
            q = o.synth_mixture_rows(SEED, 1000 * R, R, D, CENTRES, sigma, stream=1)
        d_q = ctx.to_device(q)
        t.recall_topk_dev(d_q, R, K, d_rows, d_sc)            # warm: the table's statistics / shadows, the index's scratch
        ix.recall_topk_dev(d_q, R, K, d_rows2, d_sc2)
        a_r, a_s = np.empty((R, K), np.uint64), np.empty((R, K), np.float32)
        b_r, b_s = np.empty((R, K), np.uint64), np.empty((R, K), np.float32)
        ctx.d2h(a_r, d_rows), ctx.d2h(a_s, d_sc), ctx.d2h(b_r, d_rows2), ctx.d2h(b_s, d_sc2)
        exact = bool(np.array_equal(a_r, b_r) and np.array_equal(a_s.view(np.uint32), b_s.view(np.uint32)))
        table_ms = timed(lambda: t.recall_topk_dev(d_q, R, K, d_rows, d_sc))
        s0 = ix.stats()
        index_ms = timed(lambda: ix.recall_topk_dev(d_q, R, K, d_rows2, d_sc2))
        s1 = ix.stats()
        calls = max(s1["calls"] - s0["calls"], 1)
        run = {"R": R, "table_ms": round(table_ms, 3), "index_ms": round(index_ms, 3), "ratio": round(index_ms / table_ms, 3),
               "pairs_per_R_rows": round((s1["pairs_scored"] - s0["pairs_scored"]) / calls / (R * rows), 5),
               "live_rows_per_rows": round((s1["rows_live"] - s0["rows_live"]) / calls / rows, 5), "exact": exact}
        for f in ("dense", "stale", "nonfinite", "overflow"):
            run["fallback_" + f] = s1["fallback_" + f] - s0["fallback_" + f]
        rec["runs"].append(run)
        print(name, run, flush=True, file=sys.stderr)
        ctx.free(d_q)
    out["tables"].append(rec)
    ix.destroy()
last[1].destroy()
print(json.dumps(out))
