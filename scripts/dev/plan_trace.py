"""One process per build under rocprofv3 --kernel-trace: pipeline steps at 1, 8, 32 and 256 requests on the 100 M x 128 table, then
no_pilot recalls at 1 M x 128, K = 200, with 1, 64 and 256 queries.  argv: ROOT of the tree to import, OUT.json for the counters.
--compare A_DIR B_DIR A.json B.json: the two traces launch by launch (dispatch order) and the counters."""
import sys, os, json, glob, csv

if sys.argv[1] == "--compare":
    def load(d):
        p = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        assert len(p) == 1, p
        rows = list(csv.DictReader(open(p[0])))
        rows.sort(key=lambda r: int(r["Dispatch_Id"]))
        keys = [k for k in rows[0] if k.startswith("Grid_Size") or k.startswith("Workgroup_Size") or k in ("LDS_Block_Size", "Scratch_Size", "VGPR_Count", "Accum_VGPR_Count", "SGPR_Count")]
        return [(r["Kernel_Name"],) + tuple(r[k] for k in keys) for r in rows], keys
    a, keys = load(sys.argv[2])
    b, _ = load(sys.argv[3])
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
    if first is None and len(a) != len(b):
        first = min(len(a), len(b))
    ca, cb = json.load(open(sys.argv[4])), json.load(open(sys.argv[5]))
    out = {"compared_fields": ["Kernel_Name"] + keys, "launches_parent": len(a), "launches_new": len(b), "first_difference": first,
           "distinct_kernels": len(set(x[0] for x in a)), "counters_equal": ca == cb, "counters_parent": ca, "counters_new": cb}
    if first is not None:
        out["at_first_difference"] = {"parent": a[first] if first < len(a) else None, "new": b[first] if first < len(b) else None}
    json.dump(out, open(os.path.join(os.path.dirname(sys.argv[4]), "trace_compare.json"), "w"), indent=1)
    print("launches", len(a), len(b), "first difference", first, "counters equal", ca == cb)
    for s in ca:
        print(s, ca[s], "|", cb.get(s))
    sys.exit(0 if first is None and ca == cb else 1)

ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT)
os.chdir(ROOT)
import numpy as np
import pairec_amd as pa
from oracle import oracle as o
import bench

NAMES = ("recall_rows_scanned", "recall_rescans", "recall_predicted", "recall_suspects", "recall_rescored", "recall_calls")
def snap(ctx):
    s = ctx.stats()
    return {n: int(getattr(s, n)) for n in NAMES}
def delta(a, b):
    return {n: b[n] - a[n] for n in NAMES}

res = {}
ctx = pa.Context(0)
K = 5000
t = pa.Table(ctx, 100_000_000, 128)
t.fill_synthetic(o.SEED_TABLE)
w = o.Dnn3Weights()
model = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_BF16X3, pa.pack_dnn3(w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, 128))
expr = pa.Expr(bench.RANK_EXPR)
cal = [ctx.to_device(bench.make_queries(o, 100_000 + s, 256, 128)) for s in range(10)]
p256 = bench.Pipeline1(pa, ctx, t, model, expr, 256, K, depth=1)
for d in cal:
    p256.step(d)
p256.drain()
for R in (1, 8, 32, 256):
    d = [ctx.to_device(bench.make_queries(o, 3000 + 17 * i, R, 128)) for i in range(6)]
    one = bench.Pipeline1(pa, ctx, t, model, expr, R, K, depth=1)
    for i in range(4):
        one.step(d[i])
    one.drain()
    ctx.synchronize()
    s0 = snap(ctx)
    for i in range(3):
        one.begin(d[i % 6])
        one.drain()
    ctx.synchronize()
    res["step_%d" % R] = dict(delta(s0, snap(ctx)), scan_bytes=int(ctx.last_scan_kernel()[1]))
    print("step", R, res["step_%d" % R], flush=True)
t.destroy()

t2 = pa.Table(ctx, 1_000_000, 128)
t2.fill_synthetic(o.SEED_TABLE)
ctx.set_option("no_pilot", 1)
for nq in (1, 64, 256):
    q = bench.make_queries(o, 4000 + nq, nq, 128)
    t2.recall_topk(q, 200)                      # (builds the table's statistics and shadows on first use)
    s0 = snap(ctx)
    rows, scores, counts = t2.recall_topk(q, 200)
    res["no_pilot_%d" % nq] = dict(delta(s0, snap(ctx)), scan_bytes=int(ctx.last_scan_kernel()[1]),
                                   answer_sha=__import__("hashlib").sha256(rows.tobytes() + scores.tobytes()).hexdigest()[:16])
    print("no_pilot", nq, res["no_pilot_%d" % nq], flush=True)
ctx.set_option("no_pilot", 0)
json.dump(res, open(OUT, "w"), indent=1)
print("trace job done")
