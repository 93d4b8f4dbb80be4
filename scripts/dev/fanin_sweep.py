"""Developer aid (GPU box): what the fan-in merge costs beside the host route it replaces, one process, one JSON.
   python scripts/dev/fanin_sweep.py [out.json] [requests]
Shape: `requests` (256) requests x three recall answers of 5 000 (fp32 scores), 2 000 (fp64) and 1 000 (fp32) candidates, where
10 % or 50 % of the second and third lists' entries repeat ids of the lists before them.  Per overlap:
   merge_ms     HIP-event time around pg_fanin_merge_dev with every output wanted, lists resident on the device; median of REPS
                launches after a warm-up, in the LDS tier (default: cap = 8 000 <= 8 192) and with "fanin_lds_max_cap" 0 in the
                scratch tier.  The outputs of both tiers are compared with each other, and request 0 with the host route's answer.
   host_ms      wall time of the route without the kernel: D2H of the six input arrays, ph_unique_filter (the host mirror's
                UniqueFilter over boxed module::Items, std::map) request by request, H2D of rows / scores / counts.  The JSON the
                mirror's test entry point takes is built beforehand and NOT timed; parsing it inside the call is."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pairec_amd as pa  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/fanin.json"
R = int(sys.argv[2]) if len(sys.argv) > 2 else 256
KS, F64, REPS = (5000, 2000, 1000), (False, True, False), 7
CAP = sum(KS)


def log(*a):
    print(*a, flush=True)


def lists(rng, overlap):
    """[(rows [R][k] u64, scores [R][k])]: ids distinct inside a list, `overlap` of lists 2 and 3 drawn from the lists before"""
    src, seen = [], None
    for k, f64 in zip(KS, F64):
        rows = np.empty((R, k), np.uint64)
        for q in range(R):
            fresh = rng.choice(50_000_000, k, replace=False).astype(np.uint64) + np.uint64(1 << 24)
            if seen is not None:
                n_old = int(round(overlap * k))
                fresh[:n_old] = rng.choice(seen[q], n_old, replace=False)
                rng.shuffle(fresh)
            rows[q] = fresh
        sc = rng.standard_normal((R, k))
        src.append((rows, sc if f64 else sc.astype(np.float32)))
        seen = rows if seen is None else np.concatenate([seen, rows], axis=1)
    return src


H = C.CDLL(os.path.join(ROOT, "pairec_amd", "libpairec_host.so"))
H.ph_unique_filter.restype = C.c_char_p
H.ph_unique_filter.argtypes = [C.c_char_p]
stream = torch.cuda.Stream()
ctx = pa.Context(0, stream.cuda_stream)
rng = np.random.default_rng(9)
out = {"requests": R, "k": list(KS), "cap": CAP, "reps": REPS, "cases": []}
shapes = [(R, CAP), (R, CAP), (R, CAP), (3, R, CAP), (R, CAP), (R,)]
dtypes = [np.uint64, np.float64, np.uint8, np.float64, np.uint32, np.uint32]
d_out = [ctx.malloc(int(np.prod(s)) * np.dtype(t).itemsize) for s, t in zip(shapes, dtypes)]
for overlap in (0.1, 0.5):
    src = lists(rng, overlap)
    dev = [(ctx.to_device(r), ctx.to_device(s), r.shape[1], s.dtype == np.float64) for r, s in src]
    answers = {}
    case = {"overlap": overlap}
    for tier in ("lds", "scratch"):
        ctx.set_option("fanin_lds_max_cap", 8192 if tier == "lds" else 0)
        ctx.fanin_merge_dev(dev, R, *d_out)
        ctx.synchronize()
        ms = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx.fanin_merge_dev(dev, R, *d_out)
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        got = [np.empty(s, t) for s, t in zip(shapes, dtypes)]
        for a, p in zip(got, d_out):
            ctx.d2h(a, p)
        answers[tier] = got
        case["merge_ms_" + tier] = round(float(np.median(ms)), 4)
        case["merge_ms_" + tier + "_all"] = [round(x, 4) for x in ms]
    ctx.set_option("fanin_lds_max_cap", 8192)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(answers["lds"], answers["scratch"]))
    case["mean_count"] = float(answers["lds"][5].mean())
    # the host route; the JSON of every request first, outside the clock
    texts = []
    for q in range(R):
        items = []
        for s, (rows, sc) in enumerate(src):
            items += [{"id": str(r), "score": float(v), "retrieve_id": "s%d" % s, "algo_scores": {}}
                      for r, v in zip(rows[q].tolist(), sc[q].astype(np.float64).tolist())]
        texts.append(json.dumps(items).encode())
    host_in = [np.empty_like(a) for pair in src for a in pair]
    h_rows, h_sc, h_cnt = np.full((R, CAP), np.uint64(0xFFFFFFFFFFFFFFFF)), np.full((R, CAP), -np.inf), np.zeros(R, np.uint32)
    ctx.synchronize()
    t0 = time.perf_counter()
    for a, (d_r, d_s, _, _) in zip(host_in[0::2], dev):
        ctx.d2h(a, d_r)
    for a, (d_r, d_s, _, _) in zip(host_in[1::2], dev):
        ctx.d2h(a, d_s)
    t1 = time.perf_counter()
    first = None
    for q in range(R):
        ans = H.ph_unique_filter(texts[q])
        if q == 0:
            first = json.loads(ans)
        h_cnt[q] = ans.count(b'"id"')
    t2 = time.perf_counter()
    ctx.h2d(d_out[0], h_rows)
    ctx.h2d(d_out[1], h_sc)
    ctx.h2d(d_out[5], h_cnt)
    ctx.synchronize()
    t3 = time.perf_counter()
    assert np.array_equal(h_cnt, answers["lds"][5])
    assert [int(it["id"]) for it in first] == answers["lds"][0][0, :h_cnt[0]].tolist()
    case.update(host_ms=round((t3 - t0) * 1e3, 2), host_d2h_ms=round((t1 - t0) * 1e3, 2), host_unique_filter_ms=round((t2 - t1) * 1e3, 2),
                host_h2d_ms=round((t3 - t2) * 1e3, 2))
    out["cases"].append(case)
    log(json.dumps(case))
    for d_r, d_s, _, _ in dev:
        ctx.free(d_r)
        ctx.free(d_s)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(out, fh, indent=1)
log("wrote", out_path)
for p in d_out:
    ctx.free(p)
ctx.close()
