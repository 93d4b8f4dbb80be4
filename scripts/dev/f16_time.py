"""Developer aid: the DNN3 rank stage at 512-256 per precision mode — BF16, BF16X3, F16X2, F16 — in ONE process on one box
(boxes differ by +-3 %: only the ratios mean anything).  1.28 M items per launch (256 x 5 000 random rows of a 4 M-row table),
device-event time of the rank stage (pg stats' last_rank_ms: tile list, user partial, kernel, and for the fp16 modes the
BF16X3 launch over the empty fallback list), modes interleaved round by round, median and range of the rounds; each mode's
max |score - PREC_F32's| over the 1.28 M items; and the rank stage inside a 256-request recommend step, BF16X3 against
F16X2.  Writes profiles/f16_modes.json.  GPU box.

    python scripts/dev/f16_time.py [table rows] [rounds]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import pairec_amd as pa
from oracle import oracle as o

R, K = 256, 5000
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 25
ctx = pa.Context(0)
t = pa.Table(ctx, rows, 128)
t.fill_synthetic(o.SEED_TABLE)
rng = np.random.default_rng(5)
nI = R * K
cand = rng.integers(0, rows, nI).astype(np.uint32)
offs = (np.arange(R + 1) * K).astype(np.uint32)
us = o.synth_rows(o.SEED_QUERY, 0, R, 128)
d_u, d_c, d_o = ctx.to_device(us), ctx.to_device(cand), ctx.to_device(offs)
d_out = ctx.malloc(nI * 4)
w = o.Dnn3Weights()
blob = pa.pack_dnn3(w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, 128)
precs = {"bf16": pa.PREC_BF16, "bf16x3": pa.PREC_BF16X3, "f16x2": pa.PREC_F16X2, "f16": pa.PREC_F16}
models = {k_: pa.RankModel(ctx, pa.MODEL_DNN3, v, blob) for k_, v in precs.items()}
m32 = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_F32, blob)


def scores(m):
    m.rank_dnn3_dev(t, d_u, d_c, d_o, R, nI, d_out)
    ctx.synchronize()
    out = np.empty(nI, dtype=np.float32)
    ctx.d2h(out, d_out)
    return out


ref = scores(m32).astype(np.float64)
result = {"items_per_launch": nI, "table_rows": rows, "shape": "256-512-256-1", "rounds": rounds, "modes": {}}
for name, m in models.items():
    result["modes"][name] = {"max_abs_dscore_vs_f32": float(np.max(np.abs(scores(m).astype(np.float64) - ref)))}
times = {k_: [] for k_ in models}
for rd in range(rounds + 3):                      # three warm-up rounds, dropped
    for name, m in models.items():
        for _ in range(3):                        # the third of three back-to-back calls: the clock has settled on the kernel
            m.rank_dnn3_dev(t, d_u, d_c, d_o, R, nI, d_out)
        ctx.synchronize()
        if rd >= 3:
            times[name].append(ctx.stats().last_rank_ms)
for name, v in times.items():
    result["modes"][name].update({"rank_stage_ms_median": float(np.median(v)), "rank_stage_ms_min": float(np.min(v)),
                                  "rank_stage_ms_max": float(np.max(v))})
for name in ("f16x2", "f16"):
    result["modes"][name]["f16_stats"] = models[name].f16_stats()
x3 = result["modes"]["bf16x3"]["rank_stage_ms_median"]
for name in models:
    result["modes"][name]["ratio_to_bf16x3"] = result["modes"][name]["rank_stage_ms_median"] / x3

# the rank stage inside a recommend step (scan → rank → fuse → sort), 256 requests x 5 000
ex = pa.Expr("${gpu_dnn}*(1+${current_score})^0.1")
q = o.synth_rows(o.SEED_QUERY, 0, R, 128)
step = {"bf16x3": [], "f16x2": []}
for rd in range(8):
    for name in step:
        pa.recommend_dnn3(ctx, t, models[name], ex, "gpu_dnn", q, K)
        ctx.synchronize()
        if rd >= 2:
            step[name].append(ctx.stats().last_rank_ms)
result["recommend_step_rank_stage_ms"] = {k_: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
                                          for k_, v in step.items()}
result["note"] = ("device-event ms of the rank stage, one process, modes interleaved; medians of `rounds` rounds after 3 warm-up "
                  "rounds; ratios are same-process, absolute times move +-3 % between boxes")
print(json.dumps(result))
out_path = os.environ.get("F16_TIME_OUT", os.path.join(ROOT, "profiles", "f16_modes.json"))
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
