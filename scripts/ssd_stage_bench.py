#!/usr/bin/env python3
"""SSDSort on the device beside the per-request calls: 256 requests x 500 candidates, dim 128 with the appended 1
(d1 = 129), page 100, window 5.

stage      pg_ssd_sort_dev over device arrays, ssd_norm_quality_score 0 and 1, counts uniform (500) and ragged (100 ... 500): HIP
           events around the call, device milliseconds, median of 7 after a warm-up, no copies.  A few requests are compared with
           pg_ssd before anything is written.
coalescer  the same 256 requests through pg_coalescer_ssd from 256 threads: wall clock from the first call to the last return,
           median of 5 rounds, and the coalescer's own device_ms per round.
single     pg_ssd alone at 500 x 129, page 100: wall clock per call over 5 rounds of 20 calls.

--baseline-only runs the last two alone, and --root imports the package from another checkout of the project: together they
measure the parent commit on the same box in the same session (profiles/ssd_stage.json keeps the parent's two runs under
"parent_commit_runs", merged in by hand).  Writes profiles/ssd_stage.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ, N, DIM, TOPN, WINDOW, GAMMA, N_TAB = 256, 500, 128, 100, 5, 0.25, 20000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssd_stage.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import pairec_amd as pa

    rng = np.random.default_rng(23)
    centers = rng.standard_normal((12, DIM)).astype(np.float32)
    tab = (centers[rng.integers(0, 12, N_TAB)] + 0.2 * rng.standard_normal((N_TAB, DIM))).astype(np.float32)
    rows = np.stack([rng.choice(N_TAB, N, replace=False) for _ in range(NQ)]).astype(np.uint64)
    score = np.sort(rng.random((NQ, N)), axis=1)[:, ::-1].copy()
    ragged = np.linspace(100, N, NQ).astype(np.uint32)
    out = {"nq": NQ, "candidates": N, "d1": DIM + 1, "page": TOPN, "window": WINDOW, "gamma": GAMMA, "baseline_only": bool(args.baseline_only)}

    stream = torch.cuda.Stream()
    with pa.Context(0, stream=stream.cuda_stream) as ctx:
        t = pa.Table(ctx, N_TAB, DIM)
        t.upload(tab)

        # ---- pg_ssd alone
        cand0, rel0 = rows[0].astype(np.uint32), score[0]
        pa.ssd(ctx, t, cand0, rel0, GAMMA, TOPN, WINDOW)
        single = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(20):
                pa.ssd(ctx, t, cand0, rel0, GAMMA, TOPN, WINDOW)
            single.append((time.perf_counter() - t0) / 20 * 1e3)
        out["single_ms_per_call"] = statistics.median(single)
        out["single_ms_rounds"] = single

        # ---- the 256 requests through the coalescer from 256 threads
        co = pa.Coalescer(ctx, t, 100, algos=[], depth=1, max_wait_us=3000, max_rerank_items=512)
        wall, dev = [], []
        for rnd in range(6):
            gate = threading.Barrier(NQ + 1)

            def call(i):
                gate.wait()
                co.ssd(rows[i].astype(np.uint32), score[i], GAMMA, TOPN, WINDOW)
            th = [threading.Thread(target=call, args=(i,)) for i in range(NQ)]
            for x in th:
                x.start()
            before = co.stats()
            d0, b0 = before.device_ms[4], before.batches[4]
            gate.wait()
            t0 = time.perf_counter()
            for x in th:
                x.join()
            ms = (time.perf_counter() - t0) * 1e3
            st = co.stats()
            if rnd:
                wall.append(ms)
                dev.append({"device_ms": st.device_ms[4] - d0, "batches": int(st.batches[4] - b0)})
        co.destroy()
        out["coalescer_wall_ms"] = statistics.median(wall)
        out["coalescer_wall_ms_rounds"] = wall
        out["coalescer_rounds"] = dev

        # ---- the stage
        if not args.baseline_only:
            d_rows, d_score, d_cnt = ctx.to_device(rows), ctx.to_device(score), ctx.to_device(ragged)
            d_pos, d_n, d_q = ctx.malloc(NQ * N * 4), ctx.malloc(NQ * 4), ctx.malloc(NQ * N * 8)
            out["stage"] = {}
            for mode in (0, 1):
                for name, d_count in (("uniform", 0), ("ragged", d_cnt)):
                    ms = []
                    for it in range(8):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        ctx.ssd_sort_dev(t, NQ, N, 0, d_rows, d_score, 0, d_count, 0, GAMMA, TOPN, WINDOW, d_pos, d_n, 0, d_q,
                                         norm_quality_score=mode)
                        e1.record(stream)
                        ctx.synchronize()
                        if it:
                            ms.append(e0.elapsed_time(e1))
                    pos = np.empty((NQ, N), np.uint32)
                    ctx.d2h(pos, d_pos)
                    for q in (0, 100, NQ - 1):                           # against pg_ssd on the same request
                        c = N if not d_count else int(ragged[q])
                        want, _ = pa.ssd(ctx, t, rows[q, :c].astype(np.uint32), score[q, :c], GAMMA, TOPN, WINDOW, norm_quality_score=mode)
                        assert np.array_equal(pos[q, :TOPN], want), (mode, name, q)
                    out["stage"]["mode%d_%s" % (mode, name)] = {"device_ms": statistics.median(ms), "device_ms_all": ms}
            for p in (d_rows, d_score, d_cnt, d_pos, d_n, d_q):
                ctx.free(p)
        t.destroy()
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
