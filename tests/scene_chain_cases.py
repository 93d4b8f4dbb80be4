"""Everything one scene batch needs, from a seed: the fixtures of tests/test_scene_chain_cpu.py and tests/test_gpu_scene_chain.py.

A scene is the middle and the tail of a request as a host would enqueue it on one context (include/pairec_gpu.h; the order of
tests/scene_chain_ref.py): three recall answers per request → fan-in → ItemStateFilter → recall quotas → SnakeFilter → the value
cap → the class cut → quotas over RecallScores → BoostScore (in place) → score sort → DistinctId → MixSort → SSDSort, and
DiversityRuleSort as a side branch of the last list.  `world()` holds what every batch shares (the embedding table's seed, the
feature store's columns, the rule sets); `batch(shape, seed)` holds one batch's host arrays.

Three shapes, the smallest that cross the stages' tier boundaries (the constants are the sources'):

  small   3 requests, k = 40 / 30 / 20, cap 90: every scratch layout far below one 1 MiB arena granule.
  mid     5 requests, k = 500 / 400 / 300, cap 1 200: every list stage's cap (1 200, 1 100, 1 060, 1 050, 1 030 out) is past the
          1 024-position chunk of the walks (trim.hip, trim2.hip, classcut.hip, dimcap.hip, diversity.hip); every LDS tier.
  large   2 requests, k = 3 000 / 3 000 / 2 400, cap 8 400: past fan-in's LDS tier (8 192: the scratch tier's tables), past the
          one-workgroup score sort (8 192 keys: the trim sorts 8 400-entry segments through kSlotWork), past blend's LDS list
          (2 064) and, with 6 500 entries into the value cap, past dimcap's LDS tier (6 144).  The trims bring the list to 4 600
          before the sort stages: DiversityRuleSort's cap <= 8 192, SSD's cut list <= 8 192, the mix size 64 <= 4 096.

Scratch slots between small and large (a slot is whole MiB, grows and never shrinks; sizes from the layouts at the scratch_carve /
scratch_reserve calls of csrc/*.hip, for the widths above).  Every small layout is a few KiB to 142 KiB: one granule each.  Large:
  grows     kSlotWork only: SSD's prepared embeddings, nq x n_max x d1 x 8 B = 2 x 4 600 x 129 x 8 = 9.1 MiB (ssd.hip; small: 3 x 46 x
            129 x 8 = 139 KiB, one granule) — scratch_reserve frees and reallocates it.  (The > 8 192-key sort of the trim carves
            2 x 16 384 x 12 B = 384 KiB of the same slot first: still inside the granule.  mid's SSD needs 5 x 1 030 x 129 x 8 =
            5.1 MiB, so the slot grows between small and mid as well.)
  new       kSlotDimcap: only the scratch tier (cap > 6 144) reserves it, 2 x 13 000 slots x 12 B = 305 KiB; small and mid use LDS.
  stays     kSlotFanin 834 KiB (2 x 32 768 slots x 12 B + 2 x 8 400 x 4 B — the nearest to a granule), kSlotBlend 707 KiB (6 lists x
            7 000 x 16 B + picks), kSlotTrim2 366 KiB (6 x 5 200 x 12 B), kSlotDiversity 276 KiB, kSlotSsdStage about 260 KiB,
            kSlotDiversityPlanes 144 KiB, kSlotTrim 66 KiB, kSlotClasscut 64 KiB, kSlotMix below 64 KiB: with two requests none
            leaves its first granule — these are overwritten by every batch, not reallocated."""
import numpy as np

import blend_ref
import classcut_ref
import diversity_ref
import trim_ref
from oracle import oracle as o

U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
F_I32, F_I64, F_F32, F_F64 = 1, 2, 3, 4                  # pg_feature_dtype (pairec_amd.F_*; kept here so the CPU reference needs no library)
FIX, ACC = trim_ref.FIX, trim_ref.ACCUMULATE

TABLE_ROWS, TABLE_DIM, TABLE_SEED = 20_000, 128, o.SEED_TABLE
STORE_ROWS = 600                                         # candidates' rows reach far past it
DECL = [("cat", F_I32), ("big", F_I64), ("w", F_F32), ("x", F_F64)]
RECALLS = ["r0", "r1", "r2"]

SHAPES = {
    # nq, the sources' k, the range the rows are drawn from, then per stage what sizes its output
    "small": dict(nq=3, ks=(40, 30, 20), row_hi=660, trim=(12, 40, 60), retain=60, dim_limit=1, classcut=(10, 25, 40), trim2=(10, 20, 36),
                  mix_size=12, ctx_size=10, topn=10, div_size=12),
    "mid": dict(nq=5, ks=(500, 400, 300), row_hi=6000, trim=(150, 550, 950), retain=1060, dim_limit=6, classcut=(150, 600, 900),
                trim2=(160, 500, 870), mix_size=40, ctx_size=24, topn=20, div_size=30),
    "large": dict(nq=2, ks=(3000, 3000, 2400), row_hi=TABLE_ROWS, trim=(1100, 4000, 5900), retain=6500, dim_limit=8,
                  classcut=(900, 3000, 4300), trim2=(800, 2000, 3800), mix_size=64, ctx_size=50, topn=20, div_size=40),
}

FILTER = [{"Conditions": [{"Name": "cat", "Operator": "not_equal", "Type": "int", "Value": 5},
                          {"Operator": "bool", "Type": "or", "Configs": [
                              {"Name": "cat", "Operator": "is_null"},
                              {"Name": "w", "Operator": "greater", "Type": "float", "Value": "user.lim"}]}]}]
BOOST = [{"Conditions": [{"Name": "cat", "Operator": "less", "Type": "int", "Value": 3}], "Expression": "score * 2 + x"},
         {"Conditions": [{"Name": "big", "Operator": "greater", "Type": "int64", "Value": 20 << 32}], "Expression": "score - w"},
         {"Conditions": [{"Name": "lim", "Domain": "user", "Operator": "is_not_null"}], "Expression": "round(score * 8) / 8 + 0.0625"}]
DISTINCT = [{"Conditions": [{"Name": "cat", "Operator": "equal", "Type": "int", "Value": 1}]},
            {"Conditions": [{"Name": "age", "Domain": "user", "Operator": "greater", "Type": "int", "Value": "item.cat"},
                            {"Name": "big", "Operator": "less", "Type": "int64", "Value": 9 << 32}]}]
DISTINCT_IDS = [1001, -7]
MIX = [{"MixStrategy": "fix_position", "Positions": [2, 5, 1], "SourceMask": 0b010,
        "Conditions": [{"Name": "cat", "Operator": "equal", "Type": "int", "Value": 2}]},
       {"MixStrategy": "random_position", "Number": 3,
        "Conditions": [{"Name": "age", "Domain": "user", "Operator": "greater", "Type": "int", "Value": 30}]}]
# the classes of DiversityAdjustCountFilter as classcut_ref trees; the library compiles their rendering
CLASS_TREES = [("or", ("rn_eq", "r2"), ("cmp", "<", ("col", "cat"), ("num", 3.0))),
               ("cmp", ">=", ("score",), ("num", 0.0)),
               ("not", ("rn_eq", "r0"))]
SSD = dict(gamma=0.25, window=5, norm_quality_score=1, filter_source_mask=0b100)
DIV_COLS = ["cat", "big"]


class Obj:
    pass


def world(seed=2024):
    """what every batch of a session shares: the store's columns, the table's host copy (made on first use), the rule sets"""
    w = Obj()
    rng = np.random.default_rng(seed)
    S = STORE_ROWS
    w.store = {"cat": rng.integers(0, 6, S).astype(np.int32), "big": rng.integers(0, 40, S).astype(np.int64) << 32,
               "w": (rng.integers(-4, 5, S) * 0.125).astype(np.float32), "x": rng.integers(-8, 9, S) * 0.5}
    w.defaults = {"cat": -3, "big": 11}                  # what a row outside the store reads in DiversityRuleSort's planes
    w.class_exprs = [classcut_ref.render(t) for t in CLASS_TREES]
    w._tab = None
    return w


def table(w):
    """the embedding table's rows as fill_synthetic(TABLE_SEED) leaves them, fp32 [TABLE_ROWS][TABLE_DIM]"""
    if w._tab is None:
        w._tab = o.synth_rows(TABLE_SEED, 0, TABLE_ROWS, TABLE_DIM)
    return w._tab


def scene(shape):
    """one scene configuration: a rule set for every stage, sized for the shape"""
    p = SHAPES[shape]
    cfg = Obj()
    cfg.filter, cfg.boost, cfg.distinct, cfg.distinct_ids = FILTER, BOOST, DISTINCT, DISTINCT_IDS
    cfg.trim = [(2, FIX, p["trim"][0]), (0, ACC, p["trim"][1]), (1, ACC, p["trim"][2])]
    cfg.blend = (blend_ref.SNAKE_REFILL, p["retain"], [(1, 2), (0, 3), (2, 1)])
    cfg.dimcap = ("big", p["dim_limit"], 0, None)        # DIMCAP_NULL_KEEP: an entry outside the store is kept
    cfg.class_rules = [(FIX, p["classcut"][0]), (ACC, p["classcut"][1]), (ACC, p["classcut"][2])]
    cfg.trim2 = [(1, FIX, p["trim2"][0]), (2, ACC, p["trim2"][1]), (0, ACC, p["trim2"][2])]
    cfg.mix, cfg.mix_size, cfg.mix_remain, cfg.ctx_size = MIX, p["mix_size"], True, p["ctx_size"]
    cfg.ssd = dict(SSD, topn=p["topn"])
    cfg.div = {"size": p["div_size"], "explore_item_size": 300, "exclude_source_mask": 0b100,
               "rules": [{"dims": [0], "interval": 1, "weight": 2}, {"dims": [1, 0], "window": 3, "frequency": 1, "weight": 1}],
               "exclusions": [{"positions": [1, 2], "terms": [(0, diversity_ref.EQ, -3)]}]}
    return cfg


def _scores(rng, shape):
    """a recall's scores: descending along a list mostly, 40 % from a handful of values (ties inside and across the sources),
    with NaN, +0 and -0 sprinkled in"""
    s = np.sort(rng.standard_normal(shape), axis=1)[:, ::-1].copy()
    tie = rng.random(shape) < 0.4
    s[tie] = rng.integers(-2, 3, shape)[tie] * 0.5
    r = rng.random(shape)
    s[r < 0.01] = np.nan
    s[(r >= 0.01) & (r < 0.03)] = 0.0
    s[(r >= 0.03) & (r < 0.05)] = -0.0
    return s


def batch(shape, seed):
    """one batch's host arrays: b.sources = [(rows [nq][k] u64, scores [nq][k] f32 | f64)] — source 1's scores are fp64 —, b.p32
    a carried fp32 plane [1][nq][cap] (a coarse model's score, say), b.users / b.seeds / b.enable, b.cfg the scene"""
    p = SHAPES[shape]
    rng = np.random.default_rng(seed)
    b = Obj()
    b.shape, b.seed, b.nq, b.cfg = shape, seed, p["nq"], scene(shape)
    nq, hi = p["nq"], p["row_hi"]
    inside = min(hi, STORE_ROWS + STORE_ROWS // 10)
    weight = np.where(np.arange(hi) < inside, 4.0, 1.0)               # rows in and just past the store are drawn 4 x as often
    weight /= weight.sum()
    b.sources, seen = [], None
    for i, k in enumerate(p["ks"]):
        rows = np.empty((nq, k), np.uint64)
        for q in range(nq):
            fresh = rng.choice(hi, k, replace=False, p=weight).astype(np.uint64)
            if seen is not None:
                n_old = int(0.10 * k)                                 # 10 % of a list repeats ids of the lists before it
                fresh[:n_old] = rng.choice(seen[q][seen[q] != U64MAX], n_old, replace=False)
                rng.shuffle(fresh)
            dup = rng.choice(k, max(2, k // 50), replace=False)        # duplicates inside a source
            fresh[dup[1:]] = fresh[dup[:-1]]
            pad = rng.random(k) < 0.015                               # padding anywhere in a list, one inside it at the least
            pad[rng.integers(1, k - 1)] = True
            fresh[pad] = U64MAX
            rows[q] = fresh
        sc = _scores(rng, (nq, k))
        b.sources.append((rows, sc if i == 1 else sc.astype(np.float32)))
        seen = rows if seen is None else np.concatenate([seen, rows], axis=1)
    b.cap = sum(p["ks"])
    b.p32 = rng.integers(-64, 64, (1, nq, b.cap)).astype(np.float32) * np.float32(0.03125)
    # users: every request its own threshold; the last one has no `lim` (its in-store candidates fail the filter's second term)
    b.users = [{"age": 25 + 4 * q, "lim": -0.3 + 0.125 * q} for q in range(nq)]
    del b.users[-1]["lim"]
    b.users[0]["lim"] = -1.0                                          # request 0: every in-store candidate passes that term
    b.seeds = (np.uint64(0x9E3779B97F4A7C15) * (np.arange(nq, dtype=np.uint64) + np.uint64(seed))).astype(np.uint64)
    b.enable = np.ones(nq, np.uint8)
    if nq > 2:
        b.enable[1] = 0                                               # one request passes SSD and the diversity rules untouched
    return b


BATCH_SEEDS = {"small": 11, "mid": 12, "large": 13}
