#!/usr/bin/env python3
"""TrafficControlSort's macro control on the device beside MultiRecallMixSort, the neighbouring page-shaping
sort, at one shape: 256 requests x 5 000 entries, 8 targets (traffic) / the three strategies of scripts/mixsort_bench.py (mix).

Timed with HIP events around one call on the context's stream (median of 20 after a warm-up; device milliseconds, no copies):
pg_traffic_sort_dev with mixed alphas (every chain runs), with every alpha 0 (the same compaction, sort and compose, no chain and no
table look-up), with the alphas but no member anywhere (the chains run at full length, no entry looks anything up: against the
all-zero call this is what the T + 1 sequential fp64 chains cost, against the full call what step 6 costs), and pg_mix_sort_dev.  The traffic answer is compared with pg_traffic_sort_host before anything is printed.  Prints one JSON line;
with a path argument it is written there too."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import pairec_amd as pa  # noqa: E402
from mixsort_bench import STRATEGIES, COLS, SIZE, ROWS  # noqa: E402

NQ, N, T, RUNS = 256, 5000, 8, 20


def timed(stream, ctx, call):
    ms = []
    for it in range(RUNS + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        ctx.synchronize()
        if it:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms


def main():
    rng = np.random.default_rng(12)
    score = -np.sort(-rng.uniform(0.001, 1.0, (NQ, N)), axis=1)
    member = np.zeros((NQ, N), np.uint8)
    for t in range(T):
        member |= (rng.random((NQ, N)) < 0.3).astype(np.uint8) << t
    alpha = np.tile(np.array([4.0, -6.0, 2.5, 0.9, -0.3, 25.0, -1.0, -15.0]), (NQ, 1)) * rng.uniform(0.5, 1.5, (NQ, T))
    order = np.stack([rng.permutation(N) for _ in range(NQ)]).astype(np.uint32)
    s2, m2 = np.empty_like(score), np.empty_like(member)
    for q in range(NQ):                                  # list entry j is element order[q][j]
        s2[q, order[q]] = score[q]
        m2[q, order[q]] = member[q]
    score, member = s2, m2
    traffic = pa.traffic_compile([(100 + t, 1 + t % 2) for t in range(T)])
    want = traffic.sort_host(SIZE, NQ, N, score=score, member=member, order=order, alpha=alpha, page_no=2)
    store = {"is_ad": (rng.random(ROWS) < 0.05).astype(np.int32), "slot": rng.integers(-5, 120, ROWS).astype(np.int32),
             "fresh": rng.random(ROWS).astype(np.float32)}
    rows = rng.integers(0, ROWS, (NQ, N)).astype(np.uint64)
    source = rng.choice(4, size=(NQ, N), p=[0.1, 0.1, 0.4, 0.4]).astype(np.uint8)
    seed = rng.integers(0, 1 << 63, NQ).astype(np.uint64)
    mix = pa.mix_compile(STRATEGIES, COLS, 0, False)
    stream = torch.cuda.Stream()
    out = {"nq": NQ, "entries": N, "targets": T, "ctx_size": SIZE, "runs": RUNS}
    with pa.Context(0, stream=stream.cuda_stream) as ctx:
        fs = pa.Features(ctx, ROWS)
        for name, dt in COLS:
            fs.set_column(name, dt, store[name], default=0.0)
        d = {k: ctx.to_device(v) for k, v in dict(score=score, member=member, order=order, alpha=alpha, zero=np.zeros((NQ, T)), nobody=np.zeros((NQ, N), np.uint8), rows=rows, source=source,
                                                  seed=seed).items()}
        d_out, d_cnt, d_cid, d_pos = ctx.malloc(NQ * N * 4), ctx.malloc(NQ * 4), ctx.malloc(NQ * N * 4), ctx.malloc(NQ * N * 8)
        run = lambda a: ctx.traffic_sort_dev(traffic, SIZE, NQ, N, d["score"], d["member"], d["order"], 0, d[a], d_out, d_cnt, d_cid, d_pos, page_no=2)  # noqa: E731
        out["traffic_zero_alpha_ms"], _ = timed(stream, ctx, lambda: run("zero"))
        run_m = lambda m: ctx.traffic_sort_dev(traffic, SIZE, NQ, N, d["score"], d[m], d["order"], 0, d["alpha"], d_out, d_cnt, d_cid, d_pos, page_no=2)  # noqa: E731
        out["traffic_no_member_ms"], _ = timed(stream, ctx, lambda: run_m("nobody"))
        out["traffic_ms"], out["traffic_ms_all"] = timed(stream, ctx, lambda: run("alpha"))
        got = (np.empty((NQ, N), np.uint32), np.empty(NQ, np.uint32), np.empty((NQ, N), np.int32), np.empty((NQ, N), np.float64))
        for a, p in zip(got, (d_out, d_cnt, d_cid, d_pos)):
            ctx.d2h(a, p)
        assert all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got, want)), "the device answer differs from the host statement"
        out["mix_ms"], _ = timed(stream, ctx, lambda: ctx.mix_sort_dev(mix, fs, SIZE, NQ, N, d["rows"], d["source"], d["order"], 0, d["seed"], 0, 0, d_out, d_cnt))
        for p in list(d.values()) + [d_out, d_cnt, d_cid, d_pos]:
            ctx.free(p)
        fs.destroy()
    mix.free()
    traffic.free()
    out["share_of_entries_moved"] = float((want[0] != order).mean())
    line = json.dumps(out)
    print(line, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
