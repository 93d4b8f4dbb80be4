"""Developer aid (GPU box): what DiversityAdjustCountFilter on the device costs, one process, one JSON.
   python scripts/dev/classcut_sweep.py [out.json] [requests] [store rows]
Shape: `requests` (256) requests x the merge of three recall answers of 5 000 + 2 000 + 1 000 candidates (30 % of the second and
third lists' entries repeat ids of the lists before them), six int32 columns over a store of 10 M rows, four overlapping classes cut
to 2 000 per request with every fan-in array carried.  HIP-event times, median of REPS calls after a warm-up, everything resident
on the device:
   classcut_ms      pg_candidates_classcut_dev: the mask launch, the score sort, the cut kernel
   masks_ms         pg_classcut_masks_dev alone (six scattered 4-byte loads per candidate, four programs)
   trim_quotas_ms   pg_candidates_trim_dev on the same inputs in the same run, quotas 600 / accumulate 1 500 / accumulate 2 000: the
                    only yardstick there is — the same sort, one walk over disjoint classes
and, counted on the host from the masks the device made: each class's share of the real entries and the chunks of 1 024 positions
its walk visits (mean over the requests) — what the cut kernel's time is made of."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pairec_amd as pa  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/classcut.json"
R = int(sys.argv[2]) if len(sys.argv) > 2 else 256
N = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
KS, REPS = (5000, 2000, 1000), 7
CAP = sum(KS)
RECALLS = ["r0", "r1", "r2"]
CLASSES = [("recall_name == 'r0' && c0 == 3", pa.TRIM_FIX, 400), ("c1 < 5 || c2 in (1, 2, 3)", pa.TRIM_ACCUMULATE, 1000),
           ("c3 + c4 > 9 && recall_score > 0.2", pa.TRIM_ACCUMULATE, 1600), ("c5 >= 0", pa.TRIM_ACCUMULATE, 2000)]
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
    rows = rng.integers(0, N, (R, k)).astype(np.uint64)
    if seen is not None:
        n_old = int(0.3 * k)
        for q in range(R):
            rows[q, :n_old] = rng.choice(seen[q], n_old, replace=False)
            rng.shuffle(rows[q])
    sc = rng.random((R, k))
    src.append((rows, sc if i == 1 else sc.astype(np.float32)))
    seen = rows if seen is None else np.concatenate([seen, rows], axis=1)
fs = pa.Features(ctx, N)
for j in range(6):
    fs.set_column("c%d" % j, pa.F_I32, rng.integers(0, 10, N).astype(np.int32))
ctx.synchronize()
shapes = [(R, CAP), (R, CAP), (R, CAP), (3, R, CAP), (R, CAP), (R,)]
dtypes = [np.uint64, np.float64, np.uint8, np.float64, np.uint32, np.uint32]
d_m = [ctx.malloc(int(np.prod(s)) * np.dtype(t).itemsize) for s, t in zip(shapes, dtypes)]
dev = [(ctx.to_device(r), ctx.to_device(s), r.shape[1], s.dtype == np.float64) for r, s in src]
ctx.fanin_merge_dev(dev, R, *d_m)
ctx.synchronize()
cnt = np.empty(R, np.uint32)
ctx.d2h(cnt, d_m[5])
cc = pa.classcut_compile(CLASSES, [("c%d" % j, pa.F_I32) for j in range(6)], RECALLS)
out = {"requests": R, "k": list(KS), "cap": CAP, "store_rows": N, "reps": REPS, "classes": [list(c) for c in CLASSES], "quotas": QUOTAS,
       "mean_union": float(cnt.mean()), "column_bytes": 6 * 4 * N}

oc = max(cc.out_cap(CAP), pa.trim_out_cap(QUOTAS, CAP))
d_t = [ctx.malloc(R * oc * 8), ctx.malloc(R * oc * 8), ctx.malloc(R * oc), ctx.malloc(3 * R * oc * 8), ctx.malloc(R * oc * 4), ctx.malloc(R * 4)]
d_masks = ctx.malloc(R * CAP)
kept = np.empty(R, np.uint32)
out["classcut_ms"], out["classcut_ms_all"] = timed(lambda: ctx.candidates_classcut_dev(
    cc, fs, R, CAP, d_m[0], d_m[1], d_m[2], d_m[5], d_m[3], 3, d_m[4], 0, 0, d_t[0], d_t[1], d_t[2], d_t[3], d_t[4], 0, d_t[5]))
ctx.d2h(kept, d_t[5])
out["classcut_mean_kept"] = float(kept.mean())
out["masks_ms"], out["masks_ms_all"] = timed(lambda: ctx.classcut_masks_dev(cc, fs, R, CAP, d_m[0], d_m[1], d_m[2], d_m[5], d_masks))
out["trim_quotas_ms"], out["trim_quotas_ms_all"] = timed(lambda: ctx.candidates_trim_dev(
    QUOTAS, R, CAP, d_m[0], d_m[1], d_m[2], d_m[5], d_m[3], 3, d_m[4], 0, 0, d_t[0], d_t[1], d_t[2], d_t[3], d_t[4], 0, d_t[5]))
ctx.d2h(kept, d_t[5])
out["trim_mean_kept"] = float(kept.mean())

# what the cut walks, counted on the host from the device's masks: class c visits chunks until its rank reaches its limit
masks, score = np.empty((R, CAP), np.uint8), np.empty((R, CAP), np.float64)
ctx.d2h(masks, d_masks)
ctx.d2h(score, d_m[1])
share, chunks = np.zeros(len(CLASSES)), np.zeros(len(CLASSES))
for q in range(R):
    order = np.argsort(-score[q], kind="stable")
    m = masks[q][order]
    taken, acc = np.zeros(CAP, bool), 0
    for c, (_, ty, count) in enumerate(CLASSES):
        member = ((m >> c) & 1).astype(bool)
        share[c] += member.sum() / max(int(cnt[q]), 1)
        limit = count if ty == pa.TRIM_FIX else max(0, count - acc)
        rank = np.cumsum(member)
        window = member & (rank <= limit)
        reach = np.flatnonzero(rank >= limit)
        chunks[c] += 0 if limit == 0 else (int(reach[0]) // 1024 + 1 if reach.size else (CAP + 1023) // 1024)
        picks = window & ~taken
        taken |= picks
        if ty != pa.TRIM_FIX:
            acc += int(picks.sum())
out["class_share_of_real"] = [round(float(x / R), 4) for x in share]
out["class_chunks_walked"] = [round(float(x / R), 2) for x in chunks]
log(json.dumps({k: v for k, v in out.items() if k.endswith("_ms") or k.endswith("_kept") or k.startswith("class_")}))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(out, fh, indent=1)
log("wrote", out_path)
for p in d_m + d_t + [d_masks] + [x for d in dev for x in d[:2]]:
    ctx.free(p)
cc.free()
fs.destroy()
ctx.close()
