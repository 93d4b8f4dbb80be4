"""The PG_MODEL_GBDT parity inputs, shared by test_gpu_rank_gbdt.py (which runs them) and test_rank_gbdt_cpu.py (which checks that
they meet the nodes they are there for).  Values and thresholds come from one small grid, so a value equal to its threshold is
common; the first trees' roots are set by hand on the columns that hold the awkward values."""
import functools

import numpy as np

import pairec_amd as pa

ROWS = 500
BASE = 0.3
GRID = (np.arange(-4, 5) * 0.5).astype(np.float32)
THRESHOLDS = np.concatenate([GRID, GRID, [np.inf, -np.inf]]).astype(np.float32)
BIG = 2 ** 60 + 2 ** 36 + 1                                 # int64: 0x5D800001 in one rounding to fp32, 0x5D800000 by way of a double
BIG_THR = np.array([0x5D800001], dtype=np.uint32).view(np.float32)[0]
DTYPES = (pa.F_F32, pa.F_F64, pa.F_I64, pa.F_I32)           # of item column k: DTYPES[k % 4]
NP = {pa.F_F32: np.float32, pa.F_F64: np.float64, pa.F_I64: np.int64, pa.F_I32: np.int32}
T8 = pa.gbdt_chunk_trees(8)
NARROW = (0, 1, 63, 64, 65, 200)                            # candidates per request: the one-wave tile's edges, an empty request, 4 tiles
WIDE = (pa.GBDT_WIDE_TILE - 1, pa.GBDT_WIDE_TILE, pa.GBDT_WIDE_TILE + 1, 0, 1, pa.GBDT_WIDE_ITEMS)    # the call takes the wide tile
# (n_user, n_item, depth (0: source trees of depths 1..8 with early leaves), n_tree, objective, le, leaves, candidates per request)
PARITY = [
    (5, 3, 8, 1, 1, False, "plain", NARROW),
    (5, 3, 8, T8 - 1, 1, False, "plain", NARROW),
    (5, 3, 8, T8, 1, False, "plain", NARROW),
    (5, 3, 8, T8 + 1, 1, False, "plain", NARROW),
    (64, 64, 0, 3 * T8 + 3, 1, False, "cancel", NARROW),    # four chunks: both buffers reused; the largest one-wave LDS
    (0, 1, 1, pa.gbdt_chunk_trees(1) + 1, 0, False, "plain", NARROW),
    (5, 3, 0, 3 * T8, 0, True, "plain", NARROW),
    (40, 40, 8, T8 + 1, 1, False, "cancel", WIDE),          # 80 features: the largest wide-tile LDS
]
MIXED, LE = PARITY[4], PARITY[6]


@functools.lru_cache(maxsize=None)
def columns(n_item):
    """item column k: (dtype, values [ROWS], default)"""
    rng = np.random.default_rng(7)
    cols = []
    for k in range(n_item):
        dt = DTYPES[k % 4]
        v = rng.choice(GRID, ROWS).astype(NP[dt]) if dt in (pa.F_F32, pa.F_F64) else rng.integers(-2, 3, ROWS).astype(NP[dt])
        if k == 0:
            v[0:10], v[10:20] = np.nan, -0.0
        if k == 1:
            v[5:15] = np.nan
        if k == 2:
            v[20:30] = BIG
        cols.append((dt, v, 1.5 if dt in (pa.F_F32, pa.F_F64) else -3))
    return cols


@functools.lru_cache(maxsize=None)
def inputs(n_user, n_item, reqs):
    """users [n_req][n_user], candidate rows, offsets, and x [n][n_user + n_item]: the feature vectors as the model sees them"""
    rng = np.random.default_rng(11)
    off = np.concatenate([[0], np.cumsum(reqs)]).astype(np.uint32)
    users = rng.choice(GRID, (len(reqs), n_user)).astype(np.float32)
    if n_user:
        users[[2, 5], 0] = np.nan
    cand = rng.integers(0, ROWS, int(off[-1])).astype(np.uint32)
    cand[off[5]:off[5] + 30] = np.arange(30)                               # every awkward row, in the request of several tiles
    cand[[off[2] + 3, off[5] + 40, off[5] + 41]] = [ROWS, ROWS + 7, 0xFFFFFFFF]   # past the store: the columns' defaults
    x = np.empty((len(cand), n_user + n_item), dtype=np.float32)
    x[:, :n_user] = users[np.repeat(np.arange(len(reqs)), reqs)]
    for k, (dt, v, default) in enumerate(columns(n_item)):
        x[:, n_user + k] = np.where(cand < ROWS, v[np.minimum(cand, ROWS - 1)].astype(np.float32), np.float32(NP[dt](default)))
    return users, cand, off, x


@functools.lru_cache(maxsize=None)
def forest(case):
    """the case's pointer trees"""
    n_user, n_item, depth, n_tree, _, _, leaves, _ = case
    rng = np.random.default_rng(1000 * n_tree + 10 * depth + n_item)

    def leaf_value():
        if leaves == "cancel":                                             # 1e8 down to 1e-3, both signs: an fp32 sum or another order shows
            return np.float32(rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-3, 8))
        return np.float32(rng.standard_normal())

    def grow(tr, level, d):
        i = len(tr["feature"])
        for k in tr:
            tr[k].append(0)
        tr["left"][i] = tr["right"][i] = -1
        if level == d or (depth == 0 and level >= 1 and rng.random() < 0.15):
            tr["value"][i] = leaf_value()
            return i
        tr["feature"][i], tr["threshold"][i], tr["missing_left"][i] = rng.integers(n_user + n_item), rng.choice(THRESHOLDS), rng.integers(2)
        tr["left"][i] = grow(tr, level + 1, d)
        tr["right"][i] = grow(tr, level + 1, d)
        return i

    trees = []
    for t in range(n_tree):
        tr = {k: [] for k in ("feature", "threshold", "left", "right", "missing_left", "value")}
        grow(tr, 0, depth or 1 + (7 - t) % 8)
        trees.append({k: np.asarray(v, dtype=np.float32 if k in ("threshold", "value") else np.int64) for k, v in tr.items()})
    # roots by hand: (feature, threshold, missing_left)
    f = lambda k: n_user + k                                               # noqa: E731
    roots = [(f(0), 0.0, 1), (f(0), 0.0, 0)]                               # fp32 NaN both ways; -0.0 against +0.0
    roots += [(f(1), 0.5, 1), (f(1), 0.5, 0)] if n_item > 1 else []        # fp64 NaN both ways
    roots += [(f(2), BIG_THR, 0)] if n_item > 2 else []                    # the int64 between its two fp32 roundings
    roots += [(0, 0.0, 1), (0, 0.0, 0)] if n_user else []                  # a NaN user feature both ways
    roots += [(f(0), np.inf, 0), (f(0), -np.inf, 1)]
    for tr, (feat, thr, ml) in zip(trees, roots):
        tr["feature"][0], tr["threshold"][0], tr["missing_left"][0] = feat, thr, ml
    return trees


def blob(case):
    return pa.pack_gbdt(forest(case), case[0], case[1], BASE, case[4], le=case[5])
