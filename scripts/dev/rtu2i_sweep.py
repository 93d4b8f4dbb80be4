"""Developer aid (GPU box): what RealTimeU2IRecall on the device costs, in one process, one JSON file.
   python scripts/dev/rtu2i_sweep.py [out.json] [rows] [neighbours]
Similarity table: `rows` item rows (2 M by default) with `neighbours` (50) distinct neighbours each.  256 requests of 1 024 events
over ~400 items each, the usual decay expression, TriggerCount 200: 200 triggers x 50 neighbours = 10 000 pairs per request, K =
1 000.  HIP-event time around each of the three calls with everything resident on the device, median of 7 after a warm-up:
   triggers   pg_rtu2i_triggers_dev   events → trigger lists
   expand     pg_rtu2i_expand_dev     those trigger lists → the answer
   recall     pg_rtu2i_recall_dev     events → the answer, the two kernels back to back
The event pair brackets the whole call — the staged offsets, the kernels, the status read-back — not the kernels alone."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pairec_amd as pa  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/rtu2i.json"
rows = int(sys.argv[2]) if len(sys.argv) > 2 else 2_000_000
nn = int(sys.argv[3]) if len(sys.argv) > 3 else 50
R, EVENTS, T, K, REPS, NOW = 256, 1024, 200, 1000, 7, 1_760_000_000


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
    sim.upload(np.arange(n + 1, dtype=np.uint64) * nn, nb, rng.random(n * nn, dtype=np.float32), r0)
log("uploaded", sim.info())

conf = pa.RtU2I("exp(-0.0000012 * (currentTime - eventTime))", ["click", "like", "play", "buy"], event_weight="click:1;like:2;buy:5",
                event_play_time="play:5", trigger_count=T, limit=EVENTS)
ev_rows = np.concatenate([rng.integers(0, rows, 400)[rng.integers(0, 400, EVENTS)] for _ in range(R)]).astype(np.uint32)
ev_code = rng.integers(0, 4, R * EVENTS).astype(np.uint16)
ev_pt = rng.uniform(0.0, 60.0, R * EVENTS)
ev_time = np.concatenate([np.sort(NOW - rng.integers(0, 30 * 86400, EVENTS))[::-1] for _ in range(R)]).astype(np.int64)
off = (np.arange(R + 1) * EVENTS).astype(np.uint32)
now = np.full(R, NOW, np.int64)
d_ev = [ctx.to_device(a) for a in (ev_rows, ev_code, ev_pt, ev_time)]
d_tr, d_tw, d_tc = ctx.malloc(R * T * 4), ctx.malloc(R * T * 8), ctx.malloc(R * 4)
d_rows, d_sc = ctx.malloc(R * K * 8), ctx.malloc(R * K * 8)

conf.triggers_dev(ctx, rows, d_ev[0], d_ev[1], d_ev[2], d_ev[3], off, now, d_tr, d_tw, d_tc)
tc = np.empty(R, np.uint32)
ctx.d2h(tc, d_tc)
toff = (np.arange(R + 1) * T).astype(np.uint32)     # the lists at their stride; a short list ends in padding rows, which contribute nothing
counts = {}


def triggers():
    conf.triggers_dev(ctx, rows, d_ev[0], d_ev[1], d_ev[2], d_ev[3], off, now, d_tr, d_tw, d_tc)


def expand():
    counts["expand"] = sim.rtu2i_expand_dev(d_tr, d_tw, toff, K, d_rows, d_sc)


def recall():
    counts["recall"] = sim.rtu2i_recall_dev(conf, d_ev[0], d_ev[1], d_ev[2], d_ev[3], off, now, K, d_rows, d_sc)


out = {"rows": rows, "neighbours": nn, "requests": R, "events": EVENTS, "trigger_count": T, "k": K, "reps": REPS,
       "min_triggers": int(tc.min()), "cases": []}
for name, call in (("triggers", triggers), ("expand", expand), ("recall", recall)):
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
    e = {"call": name, "call_ms": round(m, 4), "requests_per_s": round(R / m * 1e3, 1)}
    if name in counts:
        e["min_count"] = int(counts[name].min())
    out["cases"].append(e)
    log(json.dumps(e))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(out, fh, indent=1)
log("wrote", out_path)
for p in d_ev + [d_tr, d_tw, d_tc, d_rows, d_sc]:
    ctx.free(p)
conf.free()
sim.destroy()
t.destroy()
ctx.close()
