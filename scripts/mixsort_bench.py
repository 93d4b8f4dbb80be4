#!/usr/bin/env python3
"""MultiRecallMixSort on the device beside its host statement: 256 requests x 5 000 entries, S = 100, RemainItem
off; two fix_position strategies (ten configured positions claimed by a recall; a position column, Number 8, claimed by a condition)
and one random_position strategy (NumberRate 0.2, claimed by a recall and a float condition).

The list is a ranked one: d_order is a permutation per request, as pg_sort_scores_dev leaves it.  Timed: pg_mix_sort_dev with HIP
events around the call (median of 7 after a warm-up; device milliseconds, no copies), and pg_mix_sort_host on the same arrays
(wall clock, median of 3, the gather of the columns into entry-aligned arrays included; the function spreads the requests over
at most 16 threads).  Both answers are compared before anything
is written.  Writes profiles/mixsort.json."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pairec_amd as pa  # noqa: E402

NQ, N, SIZE, ROWS = 256, 5000, 100, 1_000_000
STRATEGIES = [
    {"MixStrategy": "fix_position", "Positions": [1, 4, 6, 8, 10, 20, 30, 40, 50, 60], "SourceMask": 0b0001},
    {"MixStrategy": "fix_position", "PositionField": "slot", "Number": 8,
     "Conditions": [{"Name": "is_ad", "Operator": "equal", "Type": "int", "Value": 1}]},
    {"MixStrategy": "random_position", "NumberRate": 0.2, "SourceMask": 0b0010,
     "Conditions": [{"Name": "fresh", "Operator": "greater", "Type": "float", "Value": 0.9}]},
]
COLS = [("is_ad", pa.F_I32), ("slot", pa.F_I32), ("fresh", pa.F_F32)]


def main():
    rng = np.random.default_rng(11)
    store = {"is_ad": (rng.random(ROWS) < 0.05).astype(np.int32), "slot": rng.integers(-5, 120, ROWS).astype(np.int32),
             "fresh": rng.random(ROWS).astype(np.float32)}
    rows = rng.integers(0, ROWS, (NQ, N)).astype(np.uint64)
    source = rng.choice(4, size=(NQ, N), p=[0.1, 0.1, 0.4, 0.4]).astype(np.uint8)
    order = np.stack([rng.permutation(N) for _ in range(NQ)]).astype(np.uint32)
    seed = rng.integers(0, 1 << 63, NQ).astype(np.uint64)
    out = {"nq": NQ, "entries": N, "size": SIZE, "remain_item": False, "store_rows": ROWS, "threads_host": min(16, os.cpu_count() or 1),
           "strategies": STRATEGIES}
    mix = pa.mix_compile(STRATEGIES, COLS, 0, False)
    idx = rows.astype(np.int64)
    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        want, want_cnt = mix.sort_host(SIZE, NQ, N, cols={k: v[idx] for k, v in store.items()}, source=source, order=order, seed=seed)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    stream = torch.cuda.Stream()
    with pa.Context(0, stream=stream.cuda_stream) as ctx:
        fs = pa.Features(ctx, ROWS)
        for name, dt in COLS:
            fs.set_column(name, dt, store[name], default=0.0)
        d_in = [ctx.to_device(a) for a in (rows, source, order, seed)]
        d_out, d_cnt = ctx.malloc(NQ * N * 4), ctx.malloc(NQ * 4)
        dev_ms = []
        for it in range(8):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx.mix_sort_dev(mix, fs, SIZE, NQ, N, d_in[0], d_in[1], d_in[2], 0, d_in[3], 0, 0, d_out, d_cnt)
            e1.record(stream)
            ctx.synchronize()
            if it:
                dev_ms.append(e0.elapsed_time(e1))
        got, got_cnt = np.empty((NQ, N), np.uint32), np.empty(NQ, np.uint32)
        ctx.d2h(got, d_out)
        ctx.d2h(got_cnt, d_cnt)
        assert np.array_equal(got, want) and np.array_equal(got_cnt, want_cnt)
        for p in d_in + [d_out, d_cnt]:
            ctx.free(p)
        fs.destroy()
    mix.free()
    moved = float((want[:, :SIZE] != order[:, :SIZE]).mean())
    out.update({"device_ms": statistics.median(dev_ms), "device_ms_all": dev_ms, "host_ms": statistics.median(host_ms), "host_ms_all": host_ms,
                "share_of_page_slots_moved": moved})
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mixsort.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
