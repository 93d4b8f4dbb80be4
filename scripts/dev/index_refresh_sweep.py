"""Developer aid (GPU box): pg_index_refresh beside pg_index_build, one process, one JSON file.
   python scripts/dev/index_refresh_sweep.py [out.json] [rows] [n_lists]
Run the whole script under a time limit of its own as well: timeout -k 10 900 python scripts/dev/index_refresh_sweep.py ...
Table: pg_table_fill_mixture, 1 000 centres at sigma 0.1, dim 128 (100 M rows by default), the default list count.  Steps, each
under its own time limit — an alarm with the signal's default action, so the kernel ends the process even while it sits in a
device call that never returns; nothing after a failed step is started:
   build        pg_index_build ms
   full         a forced full refresh: wall ms, last_assign_ms, its share of the bf16 matrix peak, rows_confirmed_wide; the arrays
                equal the built ones
   incremental  after uploads of 16 / 4 096 / 1 M / 10 M rows (other rows of the same mixture): refresh ms, rows moved
   crossover    the written share of the table at which the incremental refresh costs what the full one does (interpolated)
   recall       ms at R = 1 / 32 through the refreshed index beside the built one's (measured before the first write)
Every refreshed batch is compared with the table's pass (ids, score bits, counts)."""
import json
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

import pairec_amd as pa  # noqa: E402
from oracle import oracle as o  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/index_refresh.json"
rows = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
n_lists = int(sys.argv[3]) if len(sys.argv) > 3 else 0
D, K, CENTRES, SIGMA, SEED = 128, 5000, 1000, 0.1, 0x5EED0009
BF16_PEAK = 2.5e15                                   # dense bf16 FLOP/s of the MI355X's matrix pipe
UPLOADS = (16, 4096, 1_000_000, 10_000_000)


def log(*a):
    print(*a, flush=True)


class step:
    """a step of the run under its own time limit: SIGALRM's default action (no Python handler: one would wait for the
    interpreter, which a blocked device call never re-enters) ends the process when the step overruns"""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.seconds)
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, exc_type, *a):
        signal.alarm(0)
        log("step %s: %.1f s%s" % (self.name, time.perf_counter() - self.t0, "" if exc_type is None else " FAILED"))
        return False                                  # (an exception ends the run: nothing more is started on the GPU)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2]))


def recall_ms(ix, q, reps=5):
    ms = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        got = ix.recall_topk(q, K)
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), got


def checked(ix, t, checks):
    r = {}
    for R in (1, 32):
        ms, got = recall_ms(ix, q_all[:R])
        checks.append(same(got, t.recall_topk(q_all[:R], K)))
        r["R%d_ms" % R] = round(ms, 3)
    return r


ctx = pa.Context(0)
q_all = o.synth_mixture_rows(SEED, 4242, 32, D, CENTRES, SIGMA, stream=1)
out = {"rows": rows, "dim": D, "k": K, "centres": CENTRES, "sigma": SIGMA}
checks = []
with step("fill", 120):
    t = pa.Table(ctx, rows, D)
    t.fill_mixture(SEED, CENTRES, SIGMA)
with step("build", 600):
    ix = pa.Index(ctx, t, n_lists=n_lists)
    st = ix.stats()
    out["n_lists"], out["build_ms"] = st["n_lists"], round(st["build_ms"], 1)
    log("build: %.0f ms, %d lists" % (st["build_ms"], st["n_lists"]))
with step("recall_built", 120):
    out["recall_built"] = checked(ix, t, checks)
with step("full", 600):
    built = ix.read()
    ix.refresh(mode="full", force=True)
    rs = ix.refresh_stats()
    flops = 3.0 * 2.0 * rows * st["n_lists"] * D    # three bf16 products per term
    out["full"] = {"ms": round(rs["last_ms"], 1), "assign_ms": round(rs["last_assign_ms"], 1),
                   "of_build": round(rs["last_ms"] / st["build_ms"], 4),
                   "assign_share_of_bf16_peak": round(flops / (rs["last_assign_ms"] * 1e-3) / BF16_PEAK, 4),
                   "rows_confirmed_wide": rs["rows_confirmed_wide"], "rows_moved": rs["rows_moved"]}
    again = ix.read()
    out["full"]["arrays_equal_build"] = all(np.array_equal(bits(again[n]), bits(built[n])) for n in built)
    del built, again
    out["full"]["recall"] = checked(ix, t, checks)
    log(json.dumps(out["full"]))
out["incremental"] = []
ctx.set_option("index_refresh_full_fraction", 1.0)   # (the log keeps every upload: the mode is chosen here)
for i, m in enumerate(UPLOADS):
    if m > rows // 2:
        continue
    with step("incremental_%d" % m, 600):
        row0 = (rows // 7) * (i + 1) % (rows - m)
        for a in range(0, m, 1_000_000):              # other rows of the same mixture, a million at a time
            n = min(1_000_000, m - a)
            t.upload(o.synth_mixture_rows(SEED, rows + row0 + a, n, D, CENTRES, SIGMA), row0=row0 + a)
        b = ix.refresh_stats()
        ix.refresh(mode="incremental")
        rs = ix.refresh_stats()
        e = {"rows_written": m, "ms": round(rs["last_ms"], 1), "assign_ms": round(rs["last_assign_ms"], 1),
             "of_build": round(rs["last_ms"] / st["build_ms"], 5), "rows_reassigned": rs["rows_reassigned"] - b["rows_reassigned"],
             "rows_moved": rs["rows_moved"] - b["rows_moved"], "recall": checked(ix, t, checks)}
        out["incremental"].append(e)
        log(json.dumps(e))
        # (the log is not cleared by a refresh: the next step's dirty set holds this one's rows too, as rows_reassigned shows)
# the crossover of the two modes, from the incremental refreshes' slope over the rows they re-assigned
inc = out["incremental"]
if len(inc) >= 2 and inc[-1]["rows_reassigned"] > inc[0]["rows_reassigned"]:
    slope = (inc[-1]["ms"] - inc[0]["ms"]) / (inc[-1]["rows_reassigned"] - inc[0]["rows_reassigned"])
    if slope > 0:
        out["crossover_fraction"] = round(max(0.0, (out["full"]["ms"] - inc[0]["ms"]) / slope) / rows, 4)
out["exact_batches"] = "%d/%d" % (sum(checks), len(checks))
out["all_exact"] = all(checks)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(out, fh, indent=1)
log("wrote %s, all exact: %s" % (out_path, out["all_exact"]))
ix.destroy()
t.destroy()
ctx.close()
