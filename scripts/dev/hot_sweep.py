"""Developer aid (GPU box): what the list recall (UserGroupHot / UserGlobalHot / UserTopic) costs, in one
process, one JSON file.
   python scripts/dev/hot_sweep.py [out.json]
A hot table of 64 triggers over an item table of 1 M rows.  Per R in {1, 32, 256} requests, K = 1 000, HIP-event time around
pg_hot_recall_dev, medians of 3:
   one_500     one list of 500 entries per request                      (LDS tier, one wave gathers)
   8x1000      8 lists of 1 000 = 8 000 entries, padded to 8 192        (the LDS tier's edge)
   32x2000     32 lists of 2 000 = 64 000 entries, padded to 65 536     (the scratch tier)
each in PG_HOT_GROUP (always sorted) and, for the first two, in PG_HOT_TOPIC (never sorted: the gather alone).
The event pair brackets the whole call — the staged triggers' copy and the kernel — not the kernel alone."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pairec_amd as pa  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/hot_sweep.json"
ROWS, N_TRIG, K, RS, REPS = 1_000_000, 64, 1000, (1, 32, 256), 3


def log(*a):
    print(*a, flush=True)


stream = torch.cuda.Stream()
ctx = pa.Context(0, stream.cuda_stream)
t = pa.Table(ctx, ROWS, 64)
hot = ctx.hottable_create(t, N_TRIG)
rng = np.random.default_rng(5)
# trigger 0: 500 entries; 1 .. 8: 1 000 each; 9 .. 40: 2 000 each
lens = np.array([500] + [1000] * 8 + [2000] * 32 + [0] * (N_TRIG - 41), np.uint64)
off = np.zeros(N_TRIG + 1, np.uint64)
off[1:] = np.cumsum(lens)
n = int(off[-1])
hot.upload(off, rng.integers(0, ROWS, n, dtype=np.uint32), np.floor(rng.random(n) * 1e6), rng.integers(0, 4, n).astype(np.uint8))
log("uploaded", hot.info())

out = {"rows": ROWS, "k": K, "reps": REPS, "cases": []}
d_rows, d_sc, d_src, d_cnt = ctx.malloc(256 * K * 8), ctx.malloc(256 * K * 8), ctx.malloc(256 * K), ctx.malloc(256 * 4)
shapes = (("one_500", [0], 500), ("8x1000", list(range(1, 9)), 8000), ("32x2000", list(range(9, 41)), 64000))
for name, trig, entries in shapes:
    for mode, mname in ((pa.HOT_GROUP, "group"), (pa.HOT_TOPIC, "topic")):
        if mode == pa.HOT_TOPIC and entries > 8000:
            continue
        for R in RS:
            trigs = [trig] * R
            values = [[1.0] * len(trig)] * R if mode == pa.HOT_TOPIC else None

            def call():
                ctx.hot_recall_dev(hot, mode, trigs, K, d_rows, d_sc, d_src, d_cnt, values=values)

            call()
            ms = []
            for _ in range(REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            m = float(np.median(ms))
            cnt = np.empty(R, np.uint32)
            ctx.d2h(cnt, d_cnt)
            gathered = min(entries, K) if mode == pa.HOT_TOPIC else entries      # (TOPIC: the quotas share K among the lists)
            e = {"shape": name, "mode": mname, "entries": gathered, "R": R, "tier": "none" if mode == pa.HOT_TOPIC else "lds" if entries <= 8192 else "scratch",
                 "call_ms": round(m, 4), "requests_per_s": round(R / m * 1e3, 1), "entries_per_us": round(R * gathered / m / 1e3, 2),
                 "min_count": int(cnt.min())}
            out["cases"].append(e)
            log(json.dumps(e))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(out, fh, indent=1)
log("wrote", out_path)
for p in (d_rows, d_sc, d_src, d_cnt):
    ctx.free(p)
hot.destroy()
t.destroy()
ctx.close()
