"""Cost of pg_mind_interests_dev (csrc/mind.hip) and of the recall it feeds.

Interests: 256 requests, sequences of 64 and of 256 valid rows over a 1 M-row sequence table, K = 4 and 8 interests, three
routing iterations, d_user 128, h1 256, d_out 128, normalised.  Each shape is first checked against tests/mind_ref.py in fp64 on
its first four requests (1e-5: a wiring check, the bars are the tests'), then warmed up and timed with device events around
windows of back-to-back calls, each window sized from a trial to last about half a second.

Recall: pg_mind_recall_dev for 32 requests x 8 interests at k = 5000 (lists of 625) over the benchmark's item table (ROWS x 128,
synthetic), beside pg_recall_topk_dev of 256 queries at depth 625 over the same table — the same number of queries in one pass —
and the interests kernel alone for those 32 requests: its share of the call.  Both recalls end synchronised, so they are timed
with the host clock around a window of calls.

Prints one JSON document, and writes it to the path given as the first argument, if any; the second argument overrides ROWS."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pairec_amd as pa  # noqa: E402
from mind_ref import mind_interests  # noqa: E402

SEQ_ROWS, ROWS, D_USER, H1, D_OUT, N_ITER, N_REQ = 1_000_000, 100_000_000, 128, 256, 128, 3, 256


def weights(rng, K):
    u = lambda shape, fan, g=1.0: (rng.uniform(-1, 1, shape) * (g * np.sqrt(3.0 / fan))).astype(np.float32)   # noqa: E731
    return (u((64, 64), 64), rng.standard_normal((K, pa.MIND_MAX_SEQ)).astype(np.float32), u((64, H1), 64, 2.0), u((D_USER, H1), D_USER), u((H1,), H1),
            u((H1, D_OUT), H1), u((D_OUT,), H1))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else ROWS
    rng = np.random.default_rng(5)
    out = {"interests": {}, "recall": {}, "counters_collected": False}
    stream = torch.cuda.Stream()
    with pa.Context(0, stream=stream.cuda_stream) as ctx:
        def device_window(call, reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                call()
            e1.record(stream)
            ctx.synchronize()
            return e0.elapsed_time(e1) / reps

        def host_window(call, reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3 / reps

        def timed(window, call, target_ms=500.0):
            window(call, 3)                                                             # warm-up
            reps = max(3, int(target_ms / window(call, 3)))
            ms = [window(call, reps) for _ in range(5)]
            return {"ms_per_call": statistics.median(ms), "ms_windows": ms, "calls_per_window": reps}

        seq_tab = (rng.standard_normal((SEQ_ROWS, 64)) / 8).astype(np.float32)
        st = pa.Table(ctx, SEQ_ROWS, 64)
        st.upload(seq_tab)
        users = rng.standard_normal((N_REQ, D_USER)).astype(np.float32)
        d_u = ctx.to_device(users)
        models = {}
        for K in (4, 8):
            w = weights(rng, K)
            models[K] = pa.RankModel(ctx, pa.MODEL_MIND, pa.PREC_F32, pa.pack_mind(*w, N_ITER, 1))
            for n in (64, 256):
                seqs = rng.integers(0, SEQ_ROWS, (N_REQ, n)).astype(np.uint32)
                d_sr, d_so = ctx.to_device(seqs.reshape(-1)), ctx.to_device((np.arange(N_REQ + 1) * n).astype(np.uint32))
                d_o = ctx.malloc(N_REQ * K * D_OUT * 4)
                call = lambda: models[K].mind_interests_dev(st, d_u, d_sr, d_so, N_REQ, d_o)   # noqa: E731
                call()
                got = np.empty((N_REQ, K, D_OUT), dtype=np.float32)
                ctx.d2h(got, d_o)
                err = float(np.max(np.abs(got[:4] - mind_interests(w, seq_tab, users[:4], seqs[:4], N_ITER, 1))))
                assert err <= 1e-5, "interests differ from mind_ref at K %d n %d: %.3e" % (K, n, err)
                res = timed(device_window, call)
                res.update({"checked_max_err": err, "us_per_request": res["ms_per_call"] * 1e3 / N_REQ})
                out["interests"]["K%d_n%d" % (K, n)] = res
                print(K, n, res, flush=True)
                for p in (d_sr, d_so, d_o):
                    ctx.free(p)

        # the recall: 32 requests x 8 interests = 256 queries in one table pass
        K, n_req, k, n = 8, 32, 5000, 256
        items = pa.Table(ctx, rows, D_OUT)
        items.fill_synthetic(7)
        seqs = rng.integers(0, SEQ_ROWS, (n_req, n)).astype(np.uint32)
        d_sr, d_so = ctx.to_device(seqs.reshape(-1)), ctx.to_device((np.arange(n_req + 1) * n).astype(np.uint32))
        d_q, d_rows, d_sc = ctx.malloc(n_req * K * D_OUT * 4), ctx.malloc(n_req * k * 8), ctx.malloc(n_req * k * 4)
        m = models[K]
        out["recall"] = {"item_rows": rows, "requests": n_req, "interests": K, "list_depth": k // K,
                         "mind_recall_dev": timed(host_window, lambda: m.mind_recall_dev(st, items, d_u, d_sr, d_so, n_req, k, d_rows, d_sc), 2000.0),
                         "interests_alone": timed(device_window, lambda: m.mind_interests_dev(st, d_u, d_sr, d_so, n_req, d_q)),
                         "recall_topk_dev_256_queries": timed(host_window, lambda: items.recall_topk_dev(d_q, n_req * K, k // K, d_rows, d_sc), 2000.0)}
        out["recall"]["interests_share_of_call"] = out["recall"]["interests_alone"]["ms_per_call"] / out["recall"]["mind_recall_dev"]["ms_per_call"]
        print(out["recall"], flush=True)
        for p in (d_u, d_sr, d_so, d_q, d_rows, d_sc):
            ctx.free(p)
        for mm in models.values():
            mm.destroy()
        items.destroy()
        st.destroy()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
