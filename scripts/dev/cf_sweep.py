"""Developer aid (GPU box): what the collaborative-filter recall costs, in one process, one JSON file.
   python scripts/dev/cf_sweep.py [out.json] [rows] [neighbours]
Similarity table: `rows` item rows (10 M by default) with `neighbours` (50) distinct neighbours each.  Per R in {1, 32, 256}
requests, K = 1 000, HIP-event time around pg_cf_recall_dev (triggers resident on the device), medians of 3:
   t200     200 triggers per request = 10 000 pairs: above what the LDS tier holds (6 144 pairs), so the global tier either way
   t120     120 triggers per request = 6 000 pairs, in the LDS tier (default) and with "cf_lds_max_pairs" 0 in the global tier
The event pair brackets the whole call — the staged offsets, the kernel, the status read-back — not the kernel alone.
gather_useful_gbps counts 8 B per (trigger, neighbour) pair; gather_line_gbps the 128-B lines those reads touch (two arrays, each
trigger's run of 4 x neighbours bytes at an arbitrary alignment).  Beside them: the ceiling scripts/micro/gather128.hip measures
for random 128-B lines, when its binary has been built next to the source."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pairec_amd as pa  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/cf_sweep.json"
rows = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
nn = int(sys.argv[3]) if len(sys.argv) > 3 else 50
K, RS, REPS = 1000, (1, 32, 256), 3


def log(*a):
    print(*a, flush=True)


stream = torch.cuda.Stream()
ctx = pa.Context(0, stream.cuda_stream)
t = pa.Table(ctx, rows, 64)
sim = pa.SimTable(ctx, t)
rng = np.random.default_rng(5)
step = 7919                                         # row r's neighbours: (base_r + j * step) mod rows, distinct for j < neighbours
chunk = 1_000_000
for r0 in range(0, rows, chunk):
    n = min(chunk, rows - r0)
    base = rng.integers(0, rows, n, dtype=np.int64)
    nb = ((base[:, None] + step * np.arange(nn, dtype=np.int64)[None, :]) % rows).astype(np.uint32).reshape(-1)
    sm = rng.random(n * nn, dtype=np.float32)
    sim.upload(np.arange(n + 1, dtype=np.uint64) * nn, nb, sm, r0)
log("uploaded", sim.info())

ceiling = None
exe = os.path.join(ROOT, "scripts", "micro", "gather128")
if os.path.exists(exe):
    txt = subprocess.run([exe], capture_output=True, text=True, timeout=300).stdout
    rates = [float(x) for x in re.findall(r"([0-9.]+) TB/s", txt)]
    ceiling = max(rates) * 1e3 if rates else None
log("gather128 ceiling GB/s:", ceiling)

vp = C.c_void_p
out = {"rows": rows, "neighbours": nn, "k": K, "reps": REPS, "gather128_ceiling_gbps": ceiling, "cases": []}
d_rows, d_sc = ctx.malloc(256 * K * 8), ctx.malloc(256 * K * 8)
for name, nt, tiers in (("t200", 200, ("default",)), ("t120", 120, ("default", "global"))):
    for R in RS:
        trig = rng.integers(0, rows, R * nt).astype(np.uint32)
        pref = rng.uniform(0.5, 5.0, R * nt)
        off = (np.arange(R + 1) * nt).astype(np.uint32)
        d_trig, d_pref = ctx.to_device(trig), ctx.to_device(pref)
        cnt = np.zeros(R, np.uint32)
        pairs = R * nt * nn
        lines = R * nt * 2 * ((4 * nn + 127) // 128 + 1)
        for tier in tiers:
            ctx.set_option("cf_lds_max_pairs", 0 if tier == "global" else 6144)

            def call():
                pa._lib.check(ctx.L.pg_cf_recall_dev(ctx.h, sim.h, vp(d_trig), vp(d_pref), off.ctypes.data, R, K, None, vp(d_rows), vp(d_sc),
                                                     cnt.ctypes.data))

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
            e = {"shape": name, "triggers": nt, "R": R, "tier": "lds" if tier == "default" and nt * nn <= 6144 else "global",
                 "call_ms": round(m, 4), "requests_per_s": round(R / m * 1e3, 1), "gather_useful_gbps": round(pairs * 8 / m / 1e6, 2),
                 "gather_line_gbps": round(lines * 128 / m / 1e6, 2), "min_count": int(cnt.min())}
            out["cases"].append(e)
            log(json.dumps(e))
        ctx.set_option("cf_lds_max_pairs", 6144)
        ctx.free(d_trig)
        ctx.free(d_pref)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(out, fh, indent=1)
log("wrote", out_path)
ctx.free(d_rows)
ctx.free(d_sc)
sim.destroy()
t.destroy()
ctx.close()
