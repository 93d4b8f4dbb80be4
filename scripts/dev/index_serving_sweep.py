"""Developer aid (GPU box): serving through an attached index (pg_index_attach), one JSON line.
   python scripts/dev/index_serving_sweep.py [rows] [requests per caller] > profiles/index_serving.json
Tables: mixtures of 1 000 centres at sigma 0.1 and 0.3 and the uniform synthetic table, dim 128, K = 5 000.  Per table:
  callers   1 / 8 / 32 / 128 threads, each issuing single requests through one coalescer (pg_coalescer_recall) back to back,
            without and with the index attached: p50 / p99 request latency (ms) and requests per second; the attached leg's
            serving counters (plans held, re-plans, skipped batches)
  direct    pg_recall_topk_dev at R = 1 / 8 / 32 / 64 / 256 with the index attached, beside pg_index_recall_topk_dev (the
            synchronous index path) and the table's own pass (detached): median ms; every attached answer is compared with the
            pass's (ids and score bits)."""
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

import pairec_amd as pa  # noqa: E402
from oracle import oracle as o  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
per_caller = int(sys.argv[2]) if len(sys.argv) > 2 else 60
D, K, CENTRES, SEED = 128, 5000, 1000, 0x5EED0007
RS = (1, 8, 32, 64, 256)
CALLERS = (1, 8, 32, 128)
REPS = 7

ctx = pa.Context(0)
d_rows, d_sc = ctx.malloc(256 * K * 8), ctx.malloc(256 * K * 4)
d_rows2, d_sc2 = ctx.malloc(256 * K * 8), ctx.malloc(256 * K * 4)


def timed(fn):
    ms = []
    for _ in range(REPS):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def callers_leg(t, q, n):
    """n threads, per_caller requests each (after two warm-up requests): latencies and throughput"""
    co = pa.Coalescer(ctx, t, K, max_wait_us=200)
    lat = [[] for _ in range(n)]
    gate = threading.Barrier(n + 1)

    def run(i):
        for j in range(2):
            co.recall(q[(i * 7 + j) % q.shape[0]])
        gate.wait()
        for j in range(per_caller):
            t0 = time.perf_counter()
            co.recall(q[(i * 131 + j) % q.shape[0]])
            lat[i].append((time.perf_counter() - t0) * 1e3)
    th = [threading.Thread(target=run, args=(i,)) for i in range(n)]
    for x in th:
        x.start()
    gate.wait()
    t0 = time.perf_counter()
    for x in th:
        x.join()
    wall = time.perf_counter() - t0
    co.destroy()
    a = np.concatenate([np.asarray(v) for v in lat])
    return {"p50_ms": round(float(np.percentile(a, 50)), 3), "p99_ms": round(float(np.percentile(a, 99)), 3),
            "req_per_s": round(a.size / wall, 1)}


def same(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


def fetch(R):
    r, s = np.empty((R, K), np.uint64), np.empty((R, K), np.float32)
    ctx.d2h(r, d_rows)
    ctx.d2h(s, d_sc)
    return r, s


out = {"rows": rows, "dim": D, "k": K, "reps": REPS, "requests_per_caller": per_caller, "tables": []}
for name, sigma in (("mixture_s0.1", 0.1), ("mixture_s0.3", 0.3), ("uniform", None)):
    t = pa.Table(ctx, rows, D)
    if sigma is None:
        t.fill_synthetic(o.SEED_TABLE)
        q = o.synth_rows(o.SEED_QUERY, 0, 512, D)
    else:
        t.fill_mixture(SEED, CENTRES, sigma)
        q = o.synth_mixture_rows(SEED, 0, 512, D, CENTRES, sigma, stream=1)
    ix = pa.Index(ctx, t)
    rec = {"table": name, "build_ms": round(ix.stats()["build_ms"], 1), "n_lists": ix.stats()["n_lists"], "callers": [], "direct": []}
    for n in CALLERS:
        plain = callers_leg(t, q, n)
        ix.attach()
        s0 = ix.serving_stats()
        att = callers_leg(t, q, n)
        s1 = ix.serving_stats()
        ix.detach()
        att["serving"] = {k: s1[k] - s0[k] for k in s1}
        rec["callers"].append({"callers": n, "plain": plain, "attached": att})
        print(name, n, plain, att, flush=True, file=sys.stderr)
    for R in RS:
        d_q = ctx.to_device(np.ascontiguousarray(q[:R]))
        t.recall_topk_dev(d_q, R, K, d_rows, d_sc)
        ref = fetch(R)
        pass_ms = timed(lambda: t.recall_topk_dev(d_q, R, K, d_rows, d_sc))
        ix.recall_topk_dev(d_q, R, K, d_rows, d_sc)
        sync_ok = same(fetch(R), ref)
        sync_ms = timed(lambda: ix.recall_topk_dev(d_q, R, K, d_rows, d_sc))
        ix.attach()
        s0 = ix.serving_stats()
        t.recall_topk_dev(d_q, R, K, d_rows, d_sc)
        att_ok = same(fetch(R), ref)
        att_ms = timed(lambda: t.recall_topk_dev(d_q, R, K, d_rows, d_sc))
        s1 = ix.serving_stats()
        ix.detach()
        run = {"R": R, "pass_ms": round(pass_ms, 3), "index_sync_ms": round(sync_ms, 3), "attached_ms": round(att_ms, 3),
               "exact": sync_ok and att_ok, "serving": {k: s1[k] - s0[k] for k in s1}}
        rec["direct"].append(run)
        print(name, run, flush=True, file=sys.stderr)
        ctx.free(d_q)
    out["tables"].append(rec)
    ix.destroy()
    t.destroy()
print(json.dumps(out))
