"""Developer aid (GPU box): what ColdStartRecall on the device costs, in one process, one JSON file.
   python scripts/dev/coldstart_sweep.py [out.json] [rows]
A table of `rows` rows (100 M by default), a store with an int32 `bucket` column (uniform in 0 .. 999) and an int64 `create_time`
column; pools of 10 % (`bucket < 100 AND one = 1`) and 0.1 % (`bucket < 1 AND one = 1`) of the rows.  HIP-event time around each
call with everything resident on the device, median of 7 after a warm-up:
   prefix   the first pg_cold_recall_dev of a fresh pg_cold over a current bitmap: block counts + scan (synchronises, as documented)
   sample   pg_cold_recall_dev, random order         nq 1 / 32 / 256, k 200 / 5 000
   select   pg_cold_recall_dev, create_time DESC      the same shapes (one list per call: nq only widens the last write)
The bitmap's own build is pg_where's (its stats' last_build_ms is recorded beside)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pairec_amd as pa  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/coldstart.json"
rows = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
REPS = 7


def log(*a):
    print(*a, flush=True)


stream = torch.cuda.Stream()
ctx = pa.Context(0, stream.cuda_stream)
t = pa.Table(ctx, rows, 64)
fs = pa.Features(ctx, rows)
rng = np.random.default_rng(7)
fs.set_column("bucket", pa.F_I32, rng.integers(0, 1000, rows, dtype=np.int32))
fs.set_column("one", pa.F_I32, np.ones(rows, np.int32))
fs.set_column("create_time", pa.F_I64, rng.integers(1_600_000_000, 1_760_000_000, rows, dtype=np.int64))
log("uploaded", rows, "rows")


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


d_rows, d_sc, d_cnt = ctx.malloc(256 * 5000 * 8), ctx.malloc(256 * 5000 * 4), ctx.malloc(256 * 4)
d_seed = ctx.to_device(rng.integers(0, 1 << 63, 256).astype(np.uint64))
out = {"rows": rows, "reps": REPS, "cases": []}
for share, clause in (("10%", "bucket < 100 AND one = 1"), ("0.1%", "bucket < 1 AND one = 1")):
    w = pa.Where(clause)
    ms = []
    for _ in range(REPS + 1):                          # a fresh pg_cold builds its prefix; the first one the bitmap too (dropped)
        c = pa.ColdStart(w, None)
        ms.append(timed(lambda: c.recall_dev(ctx, t, fs, d_seed, 1, 1, d_rows, d_sc, d_cnt)))
        st = c.stats()
        c.free()
    e = {"call": "prefix", "pool": share, "admitted": st["admitted"], "call_ms": round(float(np.median(ms[1:])), 4),
         "bitmap_build_ms": round(w.stats()["last_build_ms"], 4), "prefix_bytes": st["bytes"]}
    out["cases"].append(e)
    log(json.dumps(e))
    for name, order_by in (("sample", None), ("select", "create_time DESC")):
        c = pa.ColdStart(w, order_by)
        for nq in (1, 32, 256):
            for k in (200, 5000):
                call = lambda: c.recall_dev(ctx, t, fs, d_seed, nq, k, d_rows, d_sc, d_cnt)      # noqa: E731
                call()
                m = float(np.median([timed(call) for _ in range(REPS)]))
                e = {"call": name, "pool": share, "nq": nq, "k": k, "call_ms": round(m, 4)}
                out["cases"].append(e)
                log(json.dumps(e))
        c.free()
    w.free()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(out, fh, indent=1)
log("wrote", out_path)
for p in (d_rows, d_sc, d_cnt, d_seed):
    ctx.free(p)
fs.destroy()
t.destroy()
ctx.close()
