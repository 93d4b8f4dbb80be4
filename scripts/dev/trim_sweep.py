"""Developer aid (GPU box): what the candidate trim and the coarse-rank cascade cost beside ranking the whole
union with the fine model, one process, one JSON.
   python scripts/dev/trim_sweep.py [out.json] [requests]
Shape: `requests` (256) requests x the merge of three recall answers of 5 000 + 2 000 + 1 000 candidates (30 % of the second and
third lists' entries repeat ids of the lists before them) over a 1 M x 128 synthetic table, cut to 2 000 per request.  HIP-event
times, median of REPS calls after a warm-up, everything resident on the device:
   trim_ms      (a) pg_candidates_trim_dev alone (its score sort included): the quotas 600 / accumulate 1 500 / accumulate 2 000
                with every carried array, and the single top-2 000 rule carrying rows, score and source
   cascade_ms   (b) pg_recommend_cascade_dnn3_dev: coarse DNN3 128-128 over the union, cut to 2 000, fine DNN3 512-256
   full_ms      (c) what the engine offered before: pg_recommend_candidates_dnn3_dev with the fine model on the whole union
(b) and (c) return synchronised, so their events include the wait for the call's end.  Both models PG_PREC_BF16X3."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pairec_amd as pa  # noqa: E402
from pairec_amd import _lib  # noqa: E402
from oracle import oracle as o  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/trim.json"
R = int(sys.argv[2]) if len(sys.argv) > 2 else 256
KS, REPS, N, DIM, KEEP = (5000, 2000, 1000), 7, 1_000_000, 128, 2000
CAP = sum(KS)
QUOTAS = [(0, pa.TRIM_FIX, 600), (1, pa.TRIM_ACCUMULATE, 1500), (2, pa.TRIM_ACCUMULATE, 2000)]
TOP = [(pa.TRIM_ANY, pa.TRIM_FIX, KEEP)]


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
out = {"requests": R, "k": list(KS), "cap": CAP, "keep": KEEP, "reps": REPS, "table_rows": N, "mean_union": float(cnt.mean())}

# (a) the trim alone
oc = pa.trim_out_cap(QUOTAS, CAP)
d_t = [ctx.malloc(R * oc * 8), ctx.malloc(R * oc * 8), ctx.malloc(R * oc), ctx.malloc(3 * R * oc * 8), ctx.malloc(R * oc * 4), ctx.malloc(R * 4)]
out["trim_quotas_ms"], out["trim_quotas_ms_all"] = timed(lambda: ctx.candidates_trim_dev(
    QUOTAS, R, CAP, d_m[0], d_m[1], d_m[2], d_m[5], d_m[3], 3, d_m[4], 0, 0, d_t[0], d_t[1], d_t[2], d_t[3], d_t[4], 0, d_t[5]))
out["trim_quotas_out_cap"] = oc
out["trim_top_ms"], out["trim_top_ms_all"] = timed(lambda: ctx.candidates_trim_dev(
    TOP, R, CAP, d_m[0], d_m[1], d_m[2], d_m[5], 0, 0, 0, 0, 0, d_t[0], d_t[1], d_t[2], 0, 0, 0, d_t[5]))
kept = np.empty(R, np.uint32)
ctx.d2h(kept, d_t[5])
assert np.all(kept == np.minimum(cnt, KEEP))
log(json.dumps({k: v for k, v in out.items() if k.startswith("trim")}))

# (b) the cascade and (c) the fine model over the whole union
t = pa.Table(ctx, N, DIM)
t.fill_synthetic(o.SEED_TABLE)
wc, wf = o.Dnn3Weights(h1=128, h2=128, seed=o.SEED_WEIGHTS ^ 0x77), o.Dnn3Weights()
coarse = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_BF16X3, pa.pack_dnn3(wc.w1, wc.b1, wc.w2, wc.b2, wc.w3, wc.b3, 128))
fine = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_BF16X3, pa.pack_dnn3(wf.w1, wf.b1, wf.w2, wf.b2, wf.w3, wf.b3, 128))
ec, ef = pa.Expr("${coarse}*(1+${current_score})^0.1"), pa.Expr("${fine}*(1+${current_score})^0.1+0.5*${coarse}")
e1 = pa.Expr("${fine}*(1+${current_score})^0.1")
d_users = ctx.to_device(o.synth_rows(o.SEED_QUERY, 0, R, DIM))
nk, n = R * KEEP, R * CAP
d_c = [ctx.malloc(nk * 8), ctx.malloc(nk * 8), ctx.malloc(nk), ctx.malloc(2 * nk * 4), ctx.malloc(nk * 8), ctx.malloc(nk * 4), ctx.malloc(R * 4)]
d_f = [ctx.malloc(n * 4), ctx.malloc(n * 8), ctx.malloc(n * 4)]
v = C.c_void_p


def cascade():
    _lib.check(ctx.L.pg_recommend_cascade_dnn3_dev(ctx.h, t.h, coarse.h, ec.h, b"coarse", fine.h, ef.h, b"fine", v(d_users), R, CAP, v(d_m[0]),
                                                   v(d_m[1]), v(d_m[2]), v(d_m[5]), KEEP, *[v(p) for p in d_c]))


def full():
    _lib.check(ctx.L.pg_recommend_candidates_dnn3_dev(ctx.h, t.h, fine.h, e1.h, b"fine", v(d_users), R, CAP, v(d_m[0]), v(d_m[1]), v(d_m[5]),
                                                      *[v(p) for p in d_f]))


# (alternating, so that both see the same machine)
out["cascade_ms"], out["cascade_ms_all"] = timed(cascade)
out["full_ms"], out["full_ms_all"] = timed(full)
c2, _ = timed(cascade)
f2, _ = timed(full)
out["cascade_ms_again"], out["full_ms_again"] = c2, f2
ctx.d2h(kept, d_c[6])
assert np.all(kept == np.minimum(cnt, KEEP))
log(json.dumps({k: v_ for k, v_ in out.items() if k.startswith(("cascade", "full"))}))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(out, fh, indent=1)
log("wrote", out_path)
for e in (ec, ef, e1):
    e.free()
for p in d_m + d_t + d_c + d_f + [d_users] + [x for d in dev for x in d[:2]]:
    ctx.free(p)
coarse.destroy()
fine.destroy()
t.destroy()
ctx.close()
