"""Developer aid (GPU box): what the per-request exclusion lists cost, in one process, one JSON file.
   python scripts/dev/exclude_sweep.py [out.json] [rows] [reps]
Table: pg_table_fill_synthetic, dim 128 (100 M rows by default; fewer when the card has no room — the rows used are recorded),
K = 5 000.  Per R in {1, 32, 256} and list length n in {0, 64, 512, 4096} (every request a list of n ids drawn from its own plain
top-(K + n)), medians of `reps` of:
   plain_k_ms     pg_recall_topk_dev at K
   plain_kx_ms    pg_recall_topk_dev at K' = K + n
   exclude_ms     pg_recall_topk_exclude_dev (lists resident on the device)
   compact_ms     pg_exclude_compact_dev alone on the K' answer (enqueue to synchronised)
Every exclude answer is checked against the host-side restatement of the K' answer (listed ids dropped, cut to K)."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

import pairec_amd as pa  # noqa: E402
from oracle import oracle as o  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/exclude_sweep.json"
rows = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
D, K = 128, 5000
RS, NS = (1, 32, 256), (0, 64, 512, 4096)
U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def log(*a):
    print(*a, flush=True)


def timed(fn):
    ms = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 4)


ctx = pa.Context(0)
t = None
while t is None:
    try:
        t = pa.Table(ctx, rows, D)
    except pa._lib.PgError:
        rows //= 2
        log("no room: trying %d rows" % rows)
t.fill_synthetic(o.SEED_TABLE)
q_all = o.synth_rows(o.SEED_QUERY, 0, 256, D)
L, vp = ctx.L, C.c_void_p
KX = K + max(NS)
d_q = ctx.to_device(q_all)
d_rows, d_sc = ctx.malloc(256 * KX * 8), ctx.malloc(256 * KX * 4)
d_orows, d_osc, d_cnt = ctx.malloc(256 * K * 8), ctx.malloc(256 * K * 4), ctx.malloc(256 * 4)
cnt = np.zeros(256, np.uint32)
out = {"rows": rows, "dim": D, "k": K, "reps": reps, "cases": []}
rng = np.random.default_rng(7)
for R in RS:
    for n in NS:
        kx = K + n

        def plain(k):
            pa._lib.check(L.pg_recall_topk_dev(ctx.h, t.h, vp(d_q), R, k, vp(d_rows), vp(d_sc), cnt.ctypes.data))

        plain(K)
        plain_k = timed(lambda: plain(K))
        plain(kx)
        plain_kx = timed(lambda: plain(kx))
        top, top_sc = np.empty((R, kx), np.uint64), np.empty((R, kx), np.float32)
        ctx.d2h(top, d_rows)
        ctx.d2h(top_sc, d_sc)
        lists = [rng.choice(top[r], n, replace=False) if n else np.zeros(0, np.uint64) for r in range(R)]
        ids, off = pa.engine._pack_lists(lists, R)
        d_ids, d_off = ctx.to_device(ids), ctx.to_device(off)

        def exclude():
            pa._lib.check(L.pg_recall_topk_exclude_dev(ctx.h, t.h, vp(d_q), R, K, vp(d_ids), off.ctypes.data, None, vp(d_orows), vp(d_osc),
                                                       cnt.ctypes.data))

        def compact():
            pa._lib.check(L.pg_exclude_compact_dev(ctx.h, vp(d_rows), vp(d_sc), R, kx, vp(d_ids), vp(d_off), K, float("-inf"), vp(d_orows),
                                                   vp(d_osc), vp(d_cnt)))

        exclude()
        got, got_sc = np.empty((R, K), np.uint64), np.empty((R, K), np.float32)
        ctx.d2h(got, d_orows)
        ctx.d2h(got_sc, d_osc)
        exact = True
        for r in range(R):
            keep = ~np.isin(top[r], lists[r])
            exact = exact and np.array_equal(got[r], top[r][keep][:K]) and np.array_equal(got_sc[r].view(np.uint32), top_sc[r][keep][:K].view(np.uint32))
        e = {"R": R, "n": n, "k_inner": kx, "plain_k_ms": plain_k, "plain_kx_ms": plain_kx, "exclude_ms": timed(exclude),
             "compact_ms": timed(compact), "exact": bool(exact)}
        out["cases"].append(e)
        log(json.dumps(e))
        ctx.free(d_ids)
        ctx.free(d_off)
out["all_exact"] = all(e["exact"] for e in out["cases"])
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(out, fh, indent=1)
log("wrote %s, all exact: %s" % (out_path, out["all_exact"]))
for p in (d_q, d_rows, d_sc, d_orows, d_osc, d_cnt):
    ctx.free(p)
t.destroy()
ctx.close()
