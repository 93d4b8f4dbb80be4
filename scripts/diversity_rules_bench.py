#!/usr/bin/env python3
"""DiversityRuleSort on the device beside its host statement: 256 requests x 5 000 candidates, ctx.Size 100.

  (a) one rule, WindowSize 10 / FrequencySize 2 over a category column;
  (b) three weighted rules (category W10 F2 w3, author IntervalSize 1 w2, (category, author) W30 F3 w1) and one exclusion rule
      (positions 1-3, is_ad = 1).

Values: category is Zipf-like over 40 values (p ~ 1 / (rank + 1)), author uniform over 500, is_ad 1 for 5 % of the entries — a
ranked list in which a few categories crowd the head.  Timed: pg_diversity_rules_dev with HIP events around the call (median of 7
after a warm-up; device milliseconds, no copies), and pg_diversity_rules_host on the same arrays (wall clock, median of 3; the
function spreads the requests over at most 16 threads).  Both answers are compared before anything is written.  Writes
profiles/diversity_rules.json."""
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

NQ, N, SIZE = 256, 5000, 100


def inputs(seed):
    rng = np.random.default_rng(seed)
    p = 1.0 / (np.arange(40) + 1.0)
    category = rng.choice(40, size=(NQ, N), p=p / p.sum())
    author = rng.integers(0, 500, (NQ, N))
    is_ad = (rng.random((NQ, N)) < 0.05).astype(np.int64)
    return np.ascontiguousarray(np.stack([category, author, is_ad]), dtype=np.int64)


CONFIGS = {
    "a_one_rule_w10_f2": {"size": SIZE, "rules": [{"dims": [0], "window": 10, "frequency": 2}]},
    "b_three_weighted_rules_one_exclusion": {
        "size": SIZE,
        "rules": [{"dims": [0], "window": 10, "frequency": 2, "weight": 3}, {"dims": [1], "interval": 1, "weight": 2},
                  {"dims": [0, 1], "window": 30, "frequency": 3, "weight": 1}],
        "exclusions": [{"positions": [1, 2, 3], "terms": [(2, pa.WHERE_EQ, 1)]}]},
}


def main():
    dims = inputs(7)
    out = {"nq": NQ, "candidates": N, "size": SIZE, "threads_host": min(16, os.cpu_count() or 1),
           "values": "category Zipf-like over 40 values (p ~ 1/(rank+1)), author uniform over 500, is_ad 5 %", "configs": {}}
    stream = torch.cuda.Stream()
    with pa.Context(0, stream=stream.cuda_stream) as ctx:
        d_dims = ctx.to_device(dims)
        d_order = ctx.malloc(NQ * N * 4)
        for name, cfg in CONFIGS.items():
            host_ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                want = pa.diversity_rules_host(cfg, dims)
                host_ms.append((time.perf_counter() - t0) * 1e3)
            dev_ms = []
            for it in range(8):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ctx.diversity_rules_dev(cfg, dims.shape[0], NQ, N, 0, d_dims, 0, 0, d_order)
                e1.record(stream)
                ctx.synchronize()
                if it:
                    dev_ms.append(e0.elapsed_time(e1))
            got = np.empty((NQ, N), np.uint32)
            ctx.d2h(got, d_order)
            assert np.array_equal(got, want), name
            moved = float((want[:, :SIZE + 1] != np.arange(SIZE + 1)).mean())
            out["configs"][name] = {"device_ms": statistics.median(dev_ms), "device_ms_all": dev_ms, "host_ms": statistics.median(host_ms),
                                    "host_ms_all": host_ms, "share_of_page_slots_moved": moved}
            print(name, out["configs"][name], flush=True)
        ctx.free(d_dims)
        ctx.free(d_order)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "diversity_rules.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
