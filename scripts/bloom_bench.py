#!/usr/bin/env python3
"""The exposure Bloom filter on the device: nq in {1, 32, 256} requests x 5 000 candidates, the keys the decimal
ids of a 10 M-row store (1 % of the candidates outside it), 4 096 slots at their design load — every bit set with probability
1 - exp(-k n / m), written through pg_bloom_slot_write — for (m, k) = (6 235 225, 4) [n = 1 M, p = 0.05] and (958 506, 7)
[n = 100 K, p = 0.01]; each request names a slot of its own.

Timed: pg_bloom_filter_dev and pg_bloom_add_dev with HIP events around the call (median of 7 after a warm-up; device
milliseconds, no copies), and — the yardstick of the same slot, not a bar — pg_item_state_filter_dev with a one-term integer rule on
the same lists.  Counted: the 128-byte lines a call touches, one key line plus k probe lines per candidate, over the time, as a
share of the random-line ceiling of scripts/micro/gather128.hip (53 G lines/s).  One request's Exists is compared
with pg_bloom_exists_host before anything is written.  Writes profiles/bloom_filter.json."""
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pairec_amd as pa  # noqa: E402

CAP, STORE, SLOTS = 5000, 10_000_000, 4096
SHAPES = [(6235225, 4, 1_000_000), (958506, 7, 100_000)]
NQS = (1, 32, 256)
LINE_CEILING = 53e9


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
    rng = np.random.default_rng(23)
    out = {"cap": CAP, "store_rows": STORE, "slots": SLOTS, "runs_per_figure": 7, "line_ceiling_per_s": LINE_CEILING, "cases": {}}
    stream = torch.cuda.Stream()
    with pa.Context(0, stream=stream.cuda_stream) as ctx:
        keys = pa.BloomKeys(ctx, ids=np.arange(STORE, dtype=np.int64))
        fs = pa.Features(ctx, STORE)
        fs.set_column("state", pa.F_I32, rng.integers(0, 4, STORE).astype(np.int32))
        cond = pa.cond_compile([{"Conditions": [{"Name": "state", "Operator": "less", "Type": "int", "Value": 2}]}], [("state", pa.F_I32)])
        nq_max = max(NQS)
        rows = rng.integers(0, STORE, (nq_max, CAP)).astype(np.uint64)
        rows[rng.random((nq_max, CAP)) < 0.01] += np.uint64(STORE)
        score = rng.standard_normal((nq_max, CAP))
        slots = rng.choice(SLOTS, nq_max, replace=False).astype(np.uint32)
        d_o = [ctx.malloc(nq_max * CAP * 8), ctx.malloc(nq_max * CAP * 8), ctx.malloc(nq_max * 4)]
        for m, k, n in SHAPES:
            b = pa.Bloom(ctx, m, k, SLOTS)
            fill = 1.0 - math.exp(-k * n / m)
            buf = np.packbits(rng.random((b.nbytes + SLOTS) * 8) < fill)
            for s in range(SLOTS):
                b.slot_write(s, buf[s:s + b.nbytes])
            # every filter first, the adds behind them: an add changes what a later filter of the same slot keeps
            dev = {nq: (ctx.to_device(rows[:nq]), ctx.to_device(score[:nq]), ctx.to_device(slots[:nq])) for nq in NQS}      # (heads of the largest batch's arrays: [nq][cap] stays dense)
            res = {}
            for nq in NQS:
                d_rows, d_score, d_slots = dev[nq]
                flt = event_ms(ctx, stream, lambda: ctx.bloom_filter_dev(b, keys, nq, CAP, d_rows, d_score, 0, 0, 0, 0, 0, 0, 0, d_slots,
                                                                         d_o[0], d_o[1], 0, 0, 0, 0, d_o[2]))
                cnt = np.empty(nq, np.uint32)
                ctx.d2h(cnt, d_o[2])
                if nq == 1:
                    off, data = pa.bloom_pack_keys([str(int(r)).encode() if r < STORE else b"" for r in rows[0]])
                    local = np.where(rows[:1] < np.uint64(STORE), np.arange(CAP, dtype=np.uint64)[None, :], np.uint64(CAP + 7))
                    want = pa.bloom_exists_host(m, k, None, b.slot_read(int(slots[0]))[None, :], off, data, local, np.zeros(1, np.uint32))
                    assert int(cnt[0]) == CAP - int(want.sum()), (m, k, int(cnt[0]), int(want.sum()))
                ist = event_ms(ctx, stream, lambda: ctx.item_state_filter_dev(cond, fs, nq, CAP, d_rows, d_score, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                                                              d_o[0], d_o[1], 0, 0, 0, 0, d_o[2]))
                res[nq] = (flt, ist, float(cnt.sum()) / (nq * CAP))
            for nq in NQS:
                d_rows, d_score, d_slots = dev[nq]
                add = event_ms(ctx, stream, lambda: ctx.bloom_add_dev(b, keys, nq, CAP, d_rows, 0, d_slots))
                flt, ist, kept = res[nq]
                f, a, i = statistics.median(flt), statistics.median(add), statistics.median(ist)
                lines = nq * CAP * (1 + k)
                name = "m%d_k%d_nq%d" % (m, k, nq)
                out["cases"][name] = {"filter_ms": f, "filter_ms_all": flt, "add_ms": a, "add_ms_all": add, "item_state_filter_ms": i,
                                      "item_state_filter_ms_all": ist, "lines_per_call": lines, "filter_lines_per_s": lines / (f * 1e-3),
                                      "filter_share_of_line_ceiling": lines / (f * 1e-3) / LINE_CEILING,
                                      "add_lines_per_s": lines / (a * 1e-3), "add_share_of_line_ceiling": lines / (a * 1e-3) / LINE_CEILING,
                                      "kept_share": kept, "slot_fill": fill, "slot_bytes_all_requests": nq * b.nbytes}
                print(name, out["cases"][name], flush=True)
            for ps in dev.values():
                for p in ps:
                    ctx.free(p)
            b.free()
        for p in d_o:
            ctx.free(p)
        cond.free()
        fs.destroy()
        keys.free()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "bloom_filter.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
