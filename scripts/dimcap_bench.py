#!/usr/bin/env python3
"""The value cap on the device: 256 requests x 5 000 entries over a 10 M-row feature store, candidate rows uniform
over the store (1 % outside it), the key column holding ~50 or ~5 000 distinct values, at limit 1 and 10.

Timed: pg_candidates_dimcap_dev with HIP events around the call (median of 7 after a warm-up; device milliseconds, no copies),
and — as context, not a bar — pg_item_state_filter_dev at the same shape on the same box with a one-term rule over the same
column.  Answers are compared with pg_candidates_dimcap_host before anything is written.  Writes profiles/dimcap.json."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pairec_amd as pa  # noqa: E402

NQ, N, STORE = 256, 5000, 10_000_000


def event_ms(ctx, stream, launch):
    ms = []
    for it in range(8):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch()
        e1.record(stream)
        ctx.synchronize()
        if it:
            ms.append(e0.elapsed_time(e1))
    return ms


def main():
    rng = np.random.default_rng(11)
    store = {"v50": rng.integers(1, 51, STORE).astype(np.int32), "v5000": rng.integers(1, 5001, STORE).astype(np.int64)}
    rows = rng.integers(0, STORE, (NQ, N)).astype(np.uint64)
    rows[rng.random((NQ, N)) < 0.01] += np.uint64(STORE)
    score = rng.standard_normal((NQ, N))
    inside = rows < np.uint64(STORE)
    idx = np.where(inside, rows, 0).astype(np.int64)
    out = {"nq": NQ, "entries": N, "store_rows": STORE, "cases": {}}
    stream = torch.cuda.Stream()
    with pa.Context(0, stream=stream.cuda_stream) as ctx:
        fs = pa.Features(ctx, STORE)
        fs.set_column("v50", pa.F_I32, store["v50"])
        fs.set_column("v5000", pa.F_I64, store["v5000"])
        d_rows, d_score = ctx.to_device(rows), ctx.to_device(score)
        d_o = [ctx.malloc(NQ * N * 8), ctx.malloc(NQ * N * 8), ctx.malloc(NQ * 4)]
        filt = {}
        for col in ("v50", "v5000"):
            cond = pa.cond_compile([{"Conditions": [{"Name": col, "Operator": "lessThan", "Type": "int", "Value": 25 if col == "v50" else 2500}]}],
                                   [("v50", pa.F_I32), ("v5000", pa.F_I64)])
            filt[col] = event_ms(ctx, stream, lambda: ctx.item_state_filter_dev(cond, fs, NQ, N, d_rows, d_score, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                                                                d_o[0], d_o[1], 0, 0, 0, 0, d_o[2]))
            cond.free()
        for col in ("v50", "v5000"):
            for limit in (1, 10):
                conf = (col, limit, pa.DIMCAP_NULL_KEEP, None)
                dev = event_ms(ctx, stream, lambda: ctx.candidates_dimcap_dev(conf, fs, NQ, N, d_rows, d_score, 0, 0, 0, 0, 0, 0, 0,
                                                                              d_o[0], d_o[1], 0, 0, 0, 0, d_o[2]))
                got_rows, got_cnt = np.empty((NQ, N), np.uint64), np.empty(NQ, np.uint32)
                ctx.d2h(got_rows, d_o[0])
                ctx.d2h(got_cnt, d_o[2])
                want = pa.candidates_dimcap_host(conf, store[col][idx].astype(np.int64), rows, score, inside.astype(np.uint8))
                assert np.array_equal(got_cnt, want[6]) and np.array_equal(got_rows, want[0]), (col, limit)
                d, f = statistics.median(dev), statistics.median(filt[col])
                name = "%s_limit_%d" % (col, limit)
                out["cases"][name] = {"device_ms": d, "device_ms_all": dev, "item_state_filter_ms": f, "item_state_filter_ms_all": filt[col],
                                      "ratio_to_item_state_filter": d / f, "kept_share": float(got_cnt.sum()) / (NQ * N)}
                print(name, out["cases"][name], flush=True)
        for p in [d_rows, d_score] + d_o:
            ctx.free(p)
        fs.destroy()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "dimcap.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
