#!/usr/bin/env python3
"""ItemStateFilter and BoostScoreSort on the device beside their host statements: 256 requests x 5 000 candidates
over a 10 M-row feature store, candidate rows uniform over the store (1 % outside it).

  (a) one rule, two int terms (status = 1 AND stock > 0);
  (b) four rules: `in` over 16 values, a float comparison, a `user.` right-hand side, no condition — with expressions that name
      two columns.  Timed as a filter on its rule 0 and as a boost over all four rules, first match and filter_all.

Timed: pg_item_state_filter_dev / pg_boost_scores_dev with HIP events around the call (median of 7 after a warm-up; device
milliseconds, no copies), and pg_cond_match_host / pg_boost_scores_host on the same candidates, the requests spread over at most 16
threads (wall clock, median of 3; the gather of the candidates' values from the store's host copy is not timed).  Answers are
compared before anything is written.  The bytes the columns imply — one 128-byte line per referenced column per candidate — are
set beside the random-line ceiling scripts/micro/gather128.hip measured (profiles/r6_gather128_microbench.txt: 53 G lines/s).
Writes profiles/cond.json."""
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pairec_amd as pa  # noqa: E402

NQ, N, STORE = 256, 5000, 10_000_000
LINE_CEILING = 53e9                      # random 128-byte lines per second (profiles/r6_gather128_microbench.txt)
DECL = [("status", pa.F_I32), ("stock", pa.F_I32), ("category", pa.F_I32), ("price", pa.F_F32), ("quality", pa.F_F64), ("level", pa.F_I64)]
RULES_A = [{"Conditions": [{"Name": "status", "Operator": "equal", "Type": "int", "Value": 1},
                           {"Name": "stock", "Operator": "greater", "Type": "int", "Value": 0}]}]
RULES_B = [
    {"Conditions": [{"Name": "category", "Operator": "in", "Type": "int", "Value": list(range(0, 48, 3))}], "Expression": "score * 1.5 + quality"},
    {"Conditions": [{"Name": "price", "Operator": "less", "Type": "float", "Value": 20.0}], "Expression": "score + price / 100"},
    {"Conditions": [{"Name": "level", "Operator": "greaterThan", "Type": "int64", "Value": "user.level"}], "Expression": "round(score * quality, 3)"},
    {"Conditions": [], "Expression": "score * 0.9 - price * quality / 1000"},
]


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


def host_ms(fn):
    out, ms = None, []
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        for _ in range(3):
            t0 = time.perf_counter()
            out = list(pool.map(fn, range(NQ)))
            ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def main():
    rng = np.random.default_rng(11)
    store = {"status": (rng.random(STORE) < 0.9).astype(np.int32), "stock": rng.integers(0, 20, STORE).astype(np.int32),
             "category": rng.integers(0, 200, STORE).astype(np.int32), "price": (rng.random(STORE) * 100).astype(np.float32),
             "quality": rng.random(STORE), "level": rng.integers(0, 10, STORE).astype(np.int64)}
    rows = rng.integers(0, STORE, (NQ, N)).astype(np.uint64)
    rows[rng.random((NQ, N)) < 0.01] += np.uint64(STORE)
    score = rng.standard_normal((NQ, N))
    users = [{"level": int(rng.integers(0, 10))} for _ in range(NQ)]
    inside = rows < np.uint64(STORE)
    idx = np.where(inside, rows, 0).astype(np.int64)
    gathered = [{k: v[idx[q]] for k, v in store.items()} for q in range(NQ)]
    out = {"nq": NQ, "candidates": N, "store_rows": STORE, "threads_host": min(16, os.cpu_count() or 1), "line_ceiling_per_s": LINE_CEILING,
           "cases": {}}
    stream = torch.cuda.Stream()
    with pa.Context(0, stream=stream.cuda_stream) as ctx:
        fs = pa.Features(ctx, STORE)
        for name, dt in DECL:
            fs.set_column(name, dt, store[name])
        d_rows, d_score = ctx.to_device(rows), ctx.to_device(score)
        d_o = [ctx.malloc(NQ * N * 8), ctx.malloc(NQ * N * 8), ctx.malloc(NQ * 4), ctx.malloc(NQ * N)]

        def lines(cond_cols):
            return NQ * N * cond_cols

        def record(name, dev, host, n_cols):
            d = statistics.median(dev)
            out["cases"][name] = {"device_ms": d, "device_ms_all": dev, "host_ms": statistics.median(host), "host_ms_all": host,
                                  "referenced_columns": n_cols, "lines_per_s": lines(n_cols) / (d * 1e-3),
                                  "share_of_line_ceiling": lines(n_cols) / (d * 1e-3) / LINE_CEILING}
            print(name, out["cases"][name], flush=True)

        for name, rules, n_cols in (("a_filter_one_rule_two_int_terms", RULES_A, 2), ("b_filter_rule0_in_16", RULES_B, 3)):
            cond = pa.cond_compile([{"Conditions": r["Conditions"]} for r in rules], DECL)
            uv, up = cond.pack_user(users)
            d_uv, d_up = ctx.to_device(uv), ctx.to_device(up)
            dev = event_ms(ctx, stream, lambda: ctx.item_state_filter_dev(cond, fs, NQ, N, d_rows, d_score, 0, 0, 0, 0, 0, 0, 0, d_uv, d_up,
                                                                          d_o[0], d_o[1], 0, 0, 0, 0, d_o[2]))
            want, host = host_ms(lambda q: cond.match_host(gathered[q], inside[q], users[q]))
            got_rows, got_cnt = np.empty((NQ, N), np.uint64), np.empty(NQ, np.uint32)
            ctx.d2h(got_rows, d_o[0])
            ctx.d2h(got_cnt, d_o[2])
            for q in range(NQ):
                assert got_cnt[q] == want[q].sum() and np.array_equal(got_rows[q, :got_cnt[q]], rows[q][want[q]]), (name, q)
            record(name, dev, host, n_cols)
            out["cases"][name]["kept_share"] = float(got_cnt.sum()) / (NQ * N)
            ctx.free(d_uv)
            ctx.free(d_up)
            cond.free()
        cond = pa.cond_compile(RULES_B, DECL, boost=True)
        uv, up = cond.pack_user(users)
        d_uv, d_up = ctx.to_device(uv), ctx.to_device(up)
        for fa in (False, True):
            name = "b_boost_four_rules_" + ("filter_all" if fa else "first_match")
            dev = event_ms(ctx, stream, lambda: ctx.boost_scores_dev(cond, fs, fa, NQ, N, d_rows, d_score, 0, d_uv, d_up, d_o[1], d_o[3]))
            want, host = host_ms(lambda q: cond.boost_host(score[q], gathered[q], inside[q], users[q], fa))
            got_s, got_r = np.empty((NQ, N), np.float64), np.empty((NQ, N), np.uint8)
            ctx.d2h(got_s, d_o[1])
            ctx.d2h(got_r, d_o[3])
            for q in range(NQ):
                assert np.array_equal(got_r[q], want[q][1]) and np.array_equal(got_s[q].view(np.uint64), want[q][0].view(np.uint64)), (name, q)
            record(name, dev, host, 4)
        ctx.free(d_uv)
        ctx.free(d_up)
        cond.free()
        for p in [d_rows, d_score] + d_o:
            ctx.free(p)
        fs.destroy()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "cond.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
