"""Developer aid (GPU box): what the U2I2X2I recall costs, in one process, one JSON file.
   python scripts/dev/x2i_sweep.py [out.json] [rows] [n_x]
X table: `rows` item rows (200 000 by default) that each name `xpi` X out of n_x (20 000), whose lists hold `xlen` distinct items.  The
sweep is nq x triggers x X per item x X list length, K = 1 000, HIP-event time around pg_x2i_recall_dev (triggers resident on the
device), medians of 3.  A request's distinct X are about triggers x xpi (X are drawn at random from n_x), its (X, item) pairs
about that times xlen; shapes beyond 1 024 X or 65 536 pairs are skipped.  For scale, pg_cf_recall_dev over a similarity table of the
same rows is timed in the same run at the same pair count per request (its triggers' lists `xlen` long, distinct X of them).
The event pair brackets the whole call — the staged offsets, the kernel, the status read-back — not the kernel alone."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pairec_amd as pa  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/x2i_sweep.json"
rows = int(sys.argv[2]) if len(sys.argv) > 2 else 200_000
n_x = int(sys.argv[3]) if len(sys.argv) > 3 else 20_000
K, REPS, STEP = 1000, 3, 7919
NQS, TRIGGERS, XPIS, XLENS = (1, 32, 256), (20, 200), (1, 4), (50, 300)


def log(*a):
    print(*a, flush=True)


stream = torch.cuda.Stream()
ctx = pa.Context(0, stream.cuda_stream)
t = pa.Table(ctx, rows, 64)
rng = np.random.default_rng(5)
vp = C.c_void_p
out = {"rows": rows, "n_x": n_x, "k": K, "reps": REPS, "cases": []}
d_rows, d_sc = ctx.malloc(256 * K * 8), ctx.malloc(256 * K * 8)


def timed(call):
    call()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def lists_of(n, length):
    """n lists of `length` distinct rows: (base + j * STEP) mod rows"""
    base = rng.integers(0, rows, n, dtype=np.int64)
    return ((base[:, None] + STEP * np.arange(length, dtype=np.int64)[None, :]) % rows).astype(np.uint32).reshape(-1)


for xpi in XPIS:
    for xlen in XLENS:
        xt = pa.XTable(ctx, t, n_x)
        sim = pa.SimTable(ctx, t)
        chunk = 100_000
        for r0 in range(0, rows, chunk):
            n = min(chunk, rows - r0)
            # xpi distinct X per row: a random start and a stride coprime to n_x
            xs = ((rng.integers(0, n_x, n, dtype=np.int64)[:, None] + 7 * np.arange(xpi, dtype=np.int64)[None, :]) % n_x).astype(np.uint32)
            xt.upload_item2x(np.arange(n + 1, dtype=np.uint64) * xpi, xs.reshape(-1), r0)
            sim.upload(np.arange(n + 1, dtype=np.uint64) * xlen, lists_of(n, xlen), rng.random(n * xlen, dtype=np.float32), r0)
        xt.upload_x2item(np.arange(n_x + 1, dtype=np.uint64) * xlen, lists_of(n_x, xlen), rng.random(n_x * xlen, dtype=np.float32), 0)
        log("uploaded", xt.info())
        for nt in TRIGGERS:
            nxq = nt * xpi                                   # about: a few X repeat
            pairs = nxq * xlen
            if nxq > 1024 or pairs > 65536:
                log("skipped: %d triggers x %d X x %d items is beyond a limit" % (nt, xpi, xlen))
                continue
            for R in NQS:
                trig = rng.integers(0, rows, R * nt).astype(np.uint32)
                pref = rng.uniform(0.5, 5.0, R * nt)
                off = (np.arange(R + 1) * nt).astype(np.uint32)
                # the scale: the same pair count per request through pg_cf_recall (nxq triggers with lists of xlen)
                ctrig = rng.integers(0, rows, R * nxq).astype(np.uint32)
                cpref = rng.uniform(0.5, 5.0, R * nxq)
                coff = (np.arange(R + 1) * nxq).astype(np.uint32)
                bufs = [ctx.to_device(a) for a in (trig, pref, ctrig, cpref)]
                cnt = np.zeros(R, np.uint32)

                def x2i():
                    pa._lib.check(ctx.L.pg_x2i_recall_dev(ctx.h, xt.h, vp(bufs[0]), vp(bufs[1]), off.ctypes.data, R, K, None, vp(d_rows), vp(d_sc),
                                                          cnt.ctypes.data))

                def cf():
                    pa._lib.check(ctx.L.pg_cf_recall_dev(ctx.h, sim.h, vp(bufs[2]), vp(bufs[3]), coff.ctypes.data, R, K, None, vp(d_rows), vp(d_sc),
                                                         cnt.ctypes.data))

                m = timed(x2i)
                min_count = int(cnt.min())
                e = {"R": R, "triggers": nt, "x_per_item": xpi, "x_list": xlen, "pairs_about": pairs,
                     "tier": "lds" if pairs <= 5120 else "global", "x2i_call_ms": round(m, 4), "x2i_requests_per_s": round(R / m * 1e3, 1),
                     "min_count": min_count}
                if nxq <= 256:
                    mc = timed(cf)
                    e["cf_same_pairs_call_ms"] = round(mc, 4)
                    e["cf_tier"] = "lds" if pairs <= 6144 else "global"
                out["cases"].append(e)
                log(json.dumps(e))
                for b in bufs:
                    ctx.free(b)
        xt.destroy()
        sim.destroy()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(out, fh, indent=1)
log("wrote", out_path)
ctx.free(d_rows)
ctx.free(d_sc)
t.destroy()
ctx.close()
