"""Developer aid (GPU box): what PriorityAdjustCountFilterV2 on the device costs, one process, one JSON.
   python scripts/dev/trim2_sweep.py [out.json] [requests]
Shape: `requests` (256) requests x the merge of three recall answers of 5 000 + 2 000 + 1 000 candidates (30 % of the second and
third lists' entries repeat ids of the lists before them), quotas 600 fix / accumulate 1 500 / accumulate 2 000, every fan-in array
carried.  HIP-event times, median of REPS calls after a warm-up, everything resident on the device:
   trim2_ms           pg_candidates_trim2_dev (key build, three sorts per request in one segmented call, the cut)
   trim_quotas_ms     pg_candidates_trim_dev with the same rules on the same inputs in the same run: one sort and one walk
   snake_refill_ms    pg_candidates_blend_dev, PG_BLEND_SNAKE_REFILL with weights 5 / 2 / 1 cut to 2 000: three sorts, a compaction
                      and a serial walk
These two are the only yardsticks there are."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pairec_amd as pa  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/trim2.json"
R = int(sys.argv[2]) if len(sys.argv) > 2 else 256
KS, REPS, N, KEEP = (5000, 2000, 1000), 7, 1_000_000, 2000
CAP = sum(KS)
ENTRIES = [(0, 5), (1, 2), (2, 1)]
QUOTAS = [(0, pa.TRIM_FIX, 600), (1, pa.TRIM_ACCUMULATE, 1500), (2, pa.TRIM_ACCUMULATE, 2000)]


def log(*a):
    print(*a, flush=True)


def timed(fn):
    fn()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(float(np.median(ms)), 4), [round(x, 4) for x in ms]


stream = torch.cuda.Stream()
ctx = pa.Context(0, stream.cuda_stream)
rng = np.random.default_rng(10)
src, seen = [], None
for i, k in enumerate(KS):
    rows = np.empty((R, k), np.uint64)
    for q in range(R):
        fresh = rng.choice(N, k, replace=False).astype(np.uint64)
        if seen is not None:
            n_old = int(0.3 * k)
            fresh[:n_old] = rng.choice(seen[q], n_old, replace=False)
            rng.shuffle(fresh)
        rows[q] = fresh
    sc = rng.random((R, k))
    src.append((rows, sc if i == 1 else sc.astype(np.float32)))
    seen = rows if seen is None else np.concatenate([seen, rows], axis=1)
shapes = [(R, CAP), (R, CAP), (R, CAP), (3, R, CAP), (R, CAP), (R,)]
dtypes = [np.uint64, np.float64, np.uint8, np.float64, np.uint32, np.uint32]
d_m = [ctx.malloc(int(np.prod(s)) * np.dtype(t).itemsize) for s, t in zip(shapes, dtypes)]
dev = [(ctx.to_device(r), ctx.to_device(s), r.shape[1], s.dtype == np.float64) for r, s in src]
ctx.fanin_merge_dev(dev, R, *d_m)
ctx.synchronize()
cnt = np.empty(R, np.uint32)
ctx.d2h(cnt, d_m[5])
out = {"requests": R, "k": list(KS), "cap": CAP, "keep": KEEP, "reps": REPS, "entries": ENTRIES, "mean_union": float(cnt.mean())}

out["quotas"] = [list(r) for r in QUOTAS]
oc = max(pa.blend_out_cap((pa.BLEND_SNAKE_REFILL, KEEP, ENTRIES), CAP), pa.trim_out_cap(QUOTAS, CAP), pa.trim2_out_cap(QUOTAS, CAP))
d_t = [ctx.malloc(R * oc * 8), ctx.malloc(R * oc * 8), ctx.malloc(R * oc), ctx.malloc(3 * R * oc * 8), ctx.malloc(R * oc * 4), ctx.malloc(R * 4)]
kept = np.empty(R, np.uint32)
args = (R, CAP, d_m[0], d_m[1], d_m[2], d_m[5], d_m[3], 3, d_m[4], 0, 0, d_t[0], d_t[1], d_t[2], d_t[3], d_t[4], 0, d_t[5])
for name, fn in (("trim2", lambda: ctx.candidates_trim2_dev(QUOTAS, *args)), ("trim_quotas", lambda: ctx.candidates_trim_dev(QUOTAS, *args)),
                 ("snake_refill", lambda: ctx.candidates_blend_dev((pa.BLEND_SNAKE_REFILL, KEEP, ENTRIES), *args))):
    out[name + "_ms"], out[name + "_ms_all"] = timed(fn)
    ctx.synchronize()
    ctx.d2h(kept, d_t[5])
    out[name + "_mean_kept"] = float(kept.mean())
    assert np.all(kept <= oc)
log(json.dumps({k: v for k, v in out.items() if k.endswith("_ms") or k.endswith("_kept")}))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(out, fh, indent=1)
log("wrote", out_path)
for p in d_m + d_t + [x for d in dev for x in d[:2]]:
    ctx.free(p)
ctx.close()
