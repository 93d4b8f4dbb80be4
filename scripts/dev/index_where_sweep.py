"""Developer aid (GPU box): filtered recalls through the exact IVF index (pg_index_recall_topk_where) against
pg_recall_topk_where in the same process, one JSON file.
   python scripts/dev/index_where_sweep.py [out.json] [rows] [reps]
Table: pg_table_fill_mixture, 1 000 centres at sigma 0.1, dim 128 (100 M rows by default), the default lists, K = 5 000.
Filters on int32 columns: random admitting 50 / 10 / 1 / 0.1 %, correlated with the clusters (the row's list id mod 10 == 3) and
anti-correlated (the rows of the 256 queries' unfiltered top K rejected).  Per filter and R in {1, 8, 32, 256}: the first call
(a cache of 0 entries: every call builds the filtered lists), the steady-state call (cached lists) under the default dense rule
and with the rule lifted, pg_recall_topk_where — medians of `reps` — with the pairs scored per (admitted x R) and the fallbacks.
Every batch is checked equal to pg_recall_topk_where (ids, score bits, counts)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

import pairec_amd as pa  # noqa: E402
from oracle import oracle as o  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/index_where.json"
rows = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
D, K, CENTRES, SIGMA, SEED = 128, 5000, 1000, 0.1, 0x5EED0007
RS = (1, 8, 32, 256)
FALLBACKS = ("fallback_dense", "fallback_stale", "fallback_nonfinite", "fallback_overflow")


def log(*a):
    print(*a, flush=True)


ctx = pa.Context(0)
t = pa.Table(ctx, rows, D)
t.fill_mixture(SEED, CENTRES, SIGMA)
q_all = o.synth_mixture_rows(SEED, 4242, 256, D, CENTRES, SIGMA, stream=1)
t0 = time.perf_counter()
ix = pa.Index(ctx, t)
ctx.synchronize()
st = ix.stats()
log("index built: %.0f ms, %d lists" % ((time.perf_counter() - t0) * 1e3, st["n_lists"]))

# the columns
rng = np.random.default_rng(SEED)
feats = pa.Features(ctx, rows)
feats.set_column("u", pa.F_I32, rng.integers(0, 1000, rows, dtype=np.int32))
r = ix.read()
cl = np.empty(rows, np.int32)
cl[r["perm"]] = np.repeat(np.arange(st["n_lists"], dtype=np.int32), np.diff(r["offsets"].astype(np.int64)))
feats.set_column("cl10", pa.F_I32, cl % 10)
del cl, r
near, _, _ = t.recall_topk(q_all, K)
anti = np.zeros(rows, np.int32)
anti[np.unique(near.astype(np.int64) - t.row_offset)] = 1
feats.set_column("anti", pa.F_I32, anti)
del anti, near
log("columns set")

FILTERS = [("random_50", "u", "<", 500), ("random_10", "u", "<", 100), ("random_1", "u", "<", 10), ("random_0.1", "u", "==", 7),
           ("correlated", "cl10", "==", 3), ("anti_correlated", "anti", "==", 0)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2]))


def timed(fn, ref, checks):
    ms = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        got = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
        if ref is not None:
            checks.append(same(got, ref))
    return float(np.median(ms)), got


out = {"rows": rows, "dim": D, "k": K, "centres": CENTRES, "sigma": SIGMA, "reps": reps, "n_lists": st["n_lists"], "filters": []}
for name, col, op, val in FILTERS:
    wr = ix.where_read(feats, col, op, val)
    adm = wr["admitted"]
    del wr
    f = {"filter": name, "where": "%s %s %d" % (col, op, val), "admitted": adm, "admitted_fraction": adm / rows, "R": []}
    for R in RS:
        q = q_all[:R]
        checks = []
        where_ms, ref = timed(lambda: t.recall_topk_where(feats, col, op, val, q, K), None, checks)
        ctx.set_option("index_where_cache", 0)
        first_ms, _ = timed(lambda: ix.recall_topk_where(feats, col, op, val, q, K), ref, checks)
        ctx.set_option("index_where_cache", 4)
        ix.recall_topk_where(feats, col, op, val, q, K)                # (the lists into the cache)
        legs = {}
        for leg, frac in (("default", 0.01), ("lifted", 1e9)):
            ctx.set_option("index_dense_fraction", frac)
            b = ix.stats()
            ms, _ = timed(lambda: ix.recall_topk_where(feats, col, op, val, q, K), ref, checks)
            a = ix.stats()
            pairs = (a["pairs_scored"] - b["pairs_scored"]) / reps
            legs[leg] = {"ms": round(ms, 3), "pairs_per_admitted_R": pairs / max(adm * R, 1), "pairs_per_rows_R": pairs / (rows * R),
                         "fallbacks": {k: a[k] - b[k] for k in FALLBACKS if a[k] - b[k]}}
        ctx.set_option("index_dense_fraction", 0.01)
        e = {"R": R, "where_ms": round(where_ms, 3), "first_ms": round(first_ms, 3), "steady_ms": legs["default"]["ms"],
             "speedup": round(where_ms / legs["default"]["ms"], 2), "default": legs["default"], "lifted": legs["lifted"],
             "exact_batches": "%d/%d" % (sum(checks), len(checks)), "exact": all(checks)}
        f["R"].append(e)
        log(json.dumps({"filter": name, **e}))
    out["filters"].append(f)
out["where_stats"] = ix.where_stats()
out["all_exact"] = all(e["exact"] for f in out["filters"] for e in f["R"])
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(out, fh, indent=1)
log("wrote %s, all exact: %s" % (out_path, out["all_exact"]))
feats.destroy()
ix.destroy()
t.destroy()
ctx.close()
