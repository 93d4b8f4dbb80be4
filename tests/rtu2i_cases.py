"""Inputs the CPU and GPU tests of RealTimeU2IRecall share (tests/test_rtu2i_cpu.py, tests/test_gpu_rtu2i.py): the grid of exp
arguments and its encoding as events, and seeded event batches."""
import math

import numpy as np

import rtu2i_ref as ref

# exp's argument as an exact quotient of two integers the events can carry: eventTime / 2^a / 2^a with currentTime = 2^a
# (both divisions by a power of two are exact); the second program negates it (the unary minus is exact, and the only way to -0.0)
EXP_POS = "exp(eventTime / currentTime / currentTime)"
EXP_NEG = "exp(-(eventTime / currentTime / currentTime))"
DECAY = "exp(-0.0000012 * (currentTime - eventTime))"
NOW = 1_760_000_000


def exp_grid():
    """±0, ±2^-28 and the thresholds with their neighbours, arguments whose result is subnormal, ±Inf, NaN, 10 000 seeded values"""
    pts = [0.0, -0.0, math.inf, -math.inf, math.nan]
    for c in (2.0 ** -28, ref.OVERFLOW, -ref.UNDERFLOW):
        for v in (np.nextafter(c, 0.0), c, np.nextafter(c, math.inf)):
            pts += [float(v), -float(v)]
    rng = np.random.default_rng(2801)
    pts += [float(x) for x in rng.uniform(-745.13, -708.4, 200)]        # exp(x) < 2^-1022
    pts += [float(x) for x in rng.uniform(-745.0, 710.0, 10000)]
    pts += [float(x) for x in rng.uniform(-1.0, 1.0, 500) * 2.0 ** rng.integers(-40, 0, 500)]   # small arguments around 2^-28
    return pts


def encode_exp(x):
    """x → (negate, event_time, now) with x = ±(event_time / now / now) in binary64, exactly"""
    if x != x:
        return False, 0, 0                                              # 0 / 0 = NaN
    if math.isinf(x):
        return x < 0, 1, 0                                              # 1 / 0 = +Inf
    neg, ax = math.copysign(1.0, x) < 0, abs(x)
    if ax == 0.0:
        return neg, 0, 2
    mant, e = math.frexp(ax)
    m, e = int(mant * 2 ** 53), e - 53
    while m % 2 == 0:
        m, e = m // 2, e + 1
    if e > 0:
        m, e = m << e, 0
    a = (-e + 1) // 2
    m <<= 2 * a + e
    assert a <= 62 and m < 2 ** 62 and float(m) / 2.0 ** a / 2.0 ** a == ax
    return neg, m, 1 << a


def exp_requests(grid):
    """the grid as requests of at most 256 one-event items that share a clock → [(negate, point indices, event_times, now)]"""
    groups = {}
    for i, x in enumerate(grid):
        neg, m, now = encode_exp(x)
        groups.setdefault((neg, now), []).append((i, m))
    out = []
    for (neg, now), pts in sorted(groups.items()):
        for b in range(0, len(pts), 256):
            chunk = pts[b:b + 256]
            out.append((neg, [p[0] for p in chunk], np.array([p[1] for p in chunk], np.int64), now))
    return out


def run_exp_grid(grid, run):
    """run(negate, rows, codes, times, now) → (trigger rows, weights, counts) over requests of one clock each; → per grid point
    the weight's bits, or None where the item was dropped (a non-finite weight)"""
    res = [None] * len(grid)
    reqs = exp_requests(grid)
    for neg in (False, True):
        mine = [r for r in reqs if r[0] == neg]
        for b in range(0, len(mine), 256):
            part = mine[b:b + 256]
            rows = [np.arange(len(r[1]), dtype=np.uint32) for r in part]
            tr, tw, tc = run(neg, rows, [np.zeros(len(r), np.uint16) for r in rows], [r[2] for r in part], [r[3] for r in part])
            for q, r in enumerate(part):
                for j in range(int(tc[q])):
                    res[r[1][int(tr[q, j])]] = int(tw[q].view(np.uint64)[j])
    return res


def random_batch(rng, nq, table_rows, n_codes, max_events=1024, pool=None):
    """nq requests of seeded events: items drawn from a small pool (so that items repeat), some rows beyond the table, codes up
    to n_codes + 1 (beyond the dictionary), play times around the thresholds the tests use → rows, codes, play_time, times, now"""
    rows, codes, pt, times, now = [], [], [], [], []
    for _ in range(nq):
        n = int(rng.integers(0, max_events + 1))
        p = pool if pool is not None else int(rng.integers(1, 400))
        items = rng.integers(0, table_rows, p)
        r = items[rng.integers(0, p, n)].astype(np.uint32)
        r[rng.random(n) < 0.03] = table_rows + 3
        r[rng.random(n) < 0.01] = ref.U32MAX
        rows.append(r)
        codes.append(rng.integers(0, n_codes + 2, n).astype(np.uint16))
        pt.append(rng.choice([0.0, 3.0, 5.0, np.nextafter(5.0, 6.0), 30.0, 31.5], n))
        t = NOW + int(rng.integers(-1000, 1000))
        now.append(t)
        times.append(np.sort(t - rng.integers(0, 30 * 86400, n))[::-1].astype(np.int64))
    return rows, codes, pt, times, now
