"""DiversityRuleSort on the device (csrc/diversity.hip): every order compared for exact equality with
tests/diversity_ref.py, the specification tests/test_diversity_cpu.py holds against the reference's loops.  The shapes sit on the
kernel's edges: a wave (64 lanes), the chunk a step scans at a time (PG_DIV_CHUNK = 1024 entries), several chunks, the largest
request; requests are kept short where the specification is slow (it walks the result's tail entry by entry)."""
import json
import os

import numpy as np
import pytest

import diversity_ref as ref
import pairec_amd as pa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK, WAVE = ref.CHUNK, ref.WAVE


def check(ctx, cfg, dims, count=None, source=None, enable=None):
    dims = np.ascontiguousarray(dims, dtype=np.int64)
    want = ref.diversity_rules(cfg, dims, count, source, enable)
    got = ctx.diversity_rules(cfg, dims, count, source, enable)
    assert got.dtype == np.uint32 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first difference at request %d slot %d: %d, expected %d" % (bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(pa.diversity_rules_host(cfg, dims, count, source, enable), want)
    return want


def one(cols):
    return np.asarray(cols, dtype=np.int64).reshape(len(cols), 1, -1)


# ---- sizes -------------------------------------------------------------------------------------------------------------------------

SIZES_CFG = {"size": 12, "explore_item_size": 700,
             "rules": [{"dims": [0], "window": 4, "frequency": 1, "weight": 2}, {"dims": [1, 0], "interval": 1}, {"dims": [2], "window": 6, "frequency": 2, "weight": -1}],
             "exclusions": [{"positions": [1, 2, 9, 13], "terms": [(1, ref.NE, 0), (2, ref.LT, 2)]}], "exclude_source_mask": 0b100}


SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 8192]


@pytest.mark.parametrize("n,nq", [(n, nq) for nq in (1, 3) for n in SIZES] + [(n, 256) for n in SIZES if n <= 1025])
def test_sizes(ctx, n, nq):
    rng = np.random.default_rng(n * 1000 + nq)
    dims = rng.integers(0, 3, (3, nq, n))
    source = rng.integers(0, 3, (nq, n)).astype(np.uint8)
    count = None
    if nq > 1:                                                       # ragged: empty, full and everything between
        count = rng.integers(0, n + 1, nq).astype(np.uint32)
        if nq > 8:                                                   # (the specification is slow: most of many requests are short)
            count[np.arange(nq) % 8 != 1] %= 97
        count[0], count[-1] = n, 0
    want = check(ctx, SIZES_CFG, dims, count, source)
    for q in range(min(nq, 3)):
        c = n if count is None else int(count[q])
        assert sorted(want[q, :c].tolist()) == list(range(c)) and (want[q, c:] == ref.NONE).all()


# ---- adversarial values ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weights", [(0, 0), (3, 1), (-2, 4)])
def test_every_candidate_shares_one_value(ctx, weights):
    """no candidate ever passes: every step falls back, to the first evaluated entry or the first of the largest w"""
    n = 2 * CHUNK + 77
    dims = np.stack([np.full(n, 9), (np.arange(n) // 3) % 2]).reshape(2, 1, n)
    cfg = {"size": 40, "rules": [{"dims": [0], "interval": 1, "weight": weights[0]}, {"dims": [1], "window": 3, "frequency": 1, "weight": weights[1]}]}
    want = check(ctx, cfg, dims)
    assert want[0, :2].tolist() == ([0, 1] if weights == (0, 0) else [0, 3])


def test_all_values_distinct(ctx):
    n = 2 * CHUNK + 5
    dims = np.stack([np.arange(n) * 7 + 1, -np.arange(n)]).reshape(2, 1, n)
    cfg = {"size": 300, "rules": [{"dims": [0], "interval": 1}, {"dims": [1, 0], "window": 50, "frequency": 1, "weight": 1}]}
    assert check(ctx, cfg, dims)[0].tolist() == list(range(n))


@pytest.mark.parametrize("run", [WAVE + 1, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + WAVE, 2 * CHUNK + 3])
def test_two_values_in_long_runs(ctx, run):
    """the first passing candidate lies a run away: across waves, at a chunk's last and first lane, chunks apart"""
    n = min(5 * run + 9, ref.MAX_N)
    dims = ((np.arange(n) // run) % 2).reshape(1, 1, n)
    want = check(ctx, {"size": 24, "rules": [{"dims": [0], "interval": 1}]}, dims)
    assert want[0, :4].tolist() == [0, run, 1, run + 1]
    check(ctx, {"size": 24, "rules": [{"dims": [0], "window": 4, "frequency": 2, "weight": 1}]}, np.repeat(dims, 2, axis=1), np.array([n, n - run], np.uint32))


# ---- windows and intervals -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("x", [WAVE - 1, WAVE, WAVE + 1, CHUNK - 1, CHUNK, CHUNK + 1])
def test_window_and_interval_about_a_wave_and_the_chunk(ctx, x):
    """window - 1 = interval = x: the tail the rules look at ends one short of, at, and one past the boundary"""
    rng = np.random.default_rng(x)
    n = x + 150
    col1 = np.zeros(n, np.int64)
    col1[[x + 60, x + 90, x + 120]] = 1                              # what breaks a run of x equal values lies 60 entries on
    dims = np.stack([(rng.random(n) < 0.25).astype(np.int64), col1]).reshape(2, 1, n)
    cfg = {"size": x + 40, "rules": [{"dims": [0], "window": x + 1, "frequency": (3 * x) // 4 + 2}, {"dims": [1], "interval": x}]}
    want = check(ctx, cfg, dims)
    assert want[0].tolist() != list(range(n)) and x + 60 in want[0, :x + 2].tolist()


def test_window_wider_than_the_request(ctx):
    rng = np.random.default_rng(11)
    n = 150
    dims = rng.integers(0, 4, (1, 2, n))
    for window in (n, n + 1, 20000, 2**31 - 1):
        check(ctx, {"size": n, "rules": [{"dims": [0], "window": window, "frequency": 3}, {"dims": [0], "interval": 2**31 - 1}]}, dims)


# ---- weights ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weights", [(5, 2), (5, -2), (-1, 2)])
def test_weight_ties_across_chunks_go_to_the_first(ctx, weights):
    """every candidate fails rule 0; rule 1 splits them into two classes of equal w that both span chunk edges"""
    n = 2 * CHUNK + 300
    col1 = np.where(np.arange(n) < CHUNK + 76, 7, 8)
    dims = np.stack([np.zeros(n, np.int64), col1]).reshape(2, 1, n)
    cfg = {"size": 30, "rules": [{"dims": [0], "window": 2, "frequency": 1, "weight": weights[0]}, {"dims": [1], "interval": 1, "weight": weights[1]}]}
    want = check(ctx, cfg, dims)
    if weights[1] > 0:
        assert want[0, :4].tolist() == [0, CHUNK + 76, 1, CHUNK + 77]
    else:
        assert want[0, :4].tolist() == [0, 1, 2, 3]


# ---- the explore bound ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [CHUNK - 1, CHUNK, CHUNK + 1])
@pytest.mark.parametrize("d", [-2, -1, 0, 1])
def test_explore_bound_about_a_chunk_edge(ctx, p, d):
    """the only passing candidate sits at position p; f = 1, so it is evaluated iff p - 1 < explore_item_size"""
    n = 2 * CHUNK + 10
    dims = (np.arange(n) >= p).astype(np.int64).reshape(1, 1, n)
    explore = p + d
    want = check(ctx, {"size": 6, "explore_item_size": explore, "rules": [{"dims": [0], "interval": 1}]}, dims)
    assert want[0, 1] == (p if p - 1 < explore else 1)
    weighted = {"size": 6, "explore_item_size": explore, "rules": [{"dims": [0], "interval": 1, "weight": 1}, {"dims": [0], "window": 3, "frequency": 1, "weight": 2}]}
    check(ctx, weighted, dims)


# ---- exclusion positions ----------------------------------------------------------------------------------------------------------------

def test_exclusion_positions(ctx):
    rng = np.random.default_rng(3)
    n, D = CHUNK + 200, 20
    dims = rng.integers(0, 3, (2, 2, n))
    for positions in ([1], [D + 1], [D + 2], [n + 5, 9000], [1, 2, 3, D, D + 1], list(range(1, 65))):
        for terms in ([(1, ref.EQ, 0)], [(1, ref.GE, 0)], [(0, ref.NE, 1), (1, ref.LE, 1)]):      # (GE 0: everything is kept off the positions)
            cfg = {"size": D, "rules": [{"dims": [0], "window": 3, "frequency": 1}], "exclusions": [{"positions": positions, "terms": terms},
                                                                                                 {"positions": [2], "terms": [(0, ref.EQ, 2)]}]}
            check(ctx, cfg, dims)
    everything_at_1 = {"size": D, "rules": [{"dims": [0], "interval": 1}], "exclusions": [{"positions": [1], "terms": [(0, ref.GE, 0)]}]}
    assert check(ctx, everything_at_1, dims)[0, 0] == 0                                          # all match at position 1: entry 0
    everything_at_3 = {"size": D, "rules": [{"dims": [0], "interval": 1}], "exclusions": [{"positions": [3], "terms": [(0, ref.GE, 0)]}]}
    want = check(ctx, everything_at_3, dims)                                                     # the loop ends after two picks
    assert want[0, 2:].tolist() == [p for p in range(n) if p not in want[0, :2].tolist()]


# ---- tuples and 64-bit values ---------------------------------------------------------------------------------------------------------

def test_four_column_tuples_that_fold_alike(ctx):
    """tuples that differ in the last column only, and tuples whose other columns differ by multiples of 2^32 or swap halves: equal
    in every 32-bit fold (low words, xor or sum of the halves), different as tuples"""
    rng = np.random.default_rng(4)
    n = CHUNK + 90
    a, b = 5, 5 + (1 << 32)
    c, d = (3 << 32) | 9, (9 << 32) | 3
    triples = [(a, 6, 7), (b, 6, 7), (a, 6 + (1 << 32), 7 - (1 << 32)), (c, 6, 7), (d, 6, 7), (-a, 6, 7)]
    pick = rng.integers(0, len(triples), n)
    cols = [np.array([triples[i][k] for i in pick], dtype=np.int64) for k in range(3)] + [rng.integers(0, 2, n).astype(np.int64)]
    dims = np.stack(cols).reshape(4, 1, n)
    cfg = {"size": 200, "rules": [{"dims": [0, 1, 2, 3], "window": 8, "frequency": 1, "weight": 2}, {"dims": [3, 0], "interval": 1}]}
    want = check(ctx, cfg, dims)
    assert want[0].tolist() != list(range(n))


def test_int64_values_beyond_32_bits(ctx):
    rng = np.random.default_rng(6)
    n = 700
    values = np.array([0, 1, 1 << 32, (1 << 32) + 1, -1, -(1 << 32), (1 << 63) - 1, -(1 << 63), 1 << 40], dtype=np.int64)
    dims = values[rng.integers(0, values.size, (2, 2, n))]
    cfg = {"size": 120, "rules": [{"dims": [0], "window": 5, "frequency": 1}, {"dims": [1], "interval": 1}],
           "exclusions": [{"positions": [1, 2, 3, 50], "terms": [(0, ref.GE, 1 << 40)]}, {"positions": [4], "terms": [(1, ref.LT, -(1 << 32) + 1), (0, ref.NE, -(1 << 63))]}]}
    check(ctx, cfg, dims)


# ---- gates ----------------------------------------------------------------------------------------------------------------------------

def test_enable_bytes_and_sources_set_aside(ctx):
    rng = np.random.default_rng(8)
    nq, n = 6, CHUNK + 40
    dims = rng.integers(0, 2, (1, nq, n))
    source = rng.integers(0, 3, (nq, n)).astype(np.uint8)
    source[2] = 1                                                    # request 2: every entry is set aside
    source[3, ::2] = 200                                             # sources past the mask's 32 bits are never set aside
    enable = np.array([1, 0, 1, 1, 0, 255], np.uint8)
    cfg = {"size": 30, "explore_item_size": 5, "rules": [{"dims": [0], "interval": 1}], "exclude_source_mask": 0b10}
    want = check(ctx, cfg, dims, None, source, enable)
    for q in (1, 2, 4):
        assert want[q].tolist() == list(range(n))
    assert want[0].tolist() != list(range(n)) and (source[0, want[0, -5:]] == 1).all()
    check(ctx, dict(cfg, exclude_source_mask=0b111), dims, None, source)                          # every source: all identities but request 3
    check(ctx, {"size": 30}, dims, np.full(nq, 17, np.uint32))                                    # no rules


# ---- the reference's own cases ------------------------------------------------------------------------------------------------------

def test_golden_cases_on_the_device(ctx):
    with open(os.path.join(ROOT, "tests", "golden", "diversity_rule_sort.json")) as f:
        cases = json.load(f)["cases"]
    for case in cases:
        cols = [case["columns"][name] for name in case["column_names"]]
        cfg = dict(case["config"], exclusions=[{"positions": e["positions"], "terms": [tuple(t) for t in e["terms"]]}
                                               for e in case["config"].get("exclusions", [])])
        assert ctx.diversity_rules(cfg, one(cols))[0].tolist() == case["expected_order"], case["name"]
        assert ctx.diversity_rules_one(cfg, np.asarray(cols, np.int64)).tolist() == case["expected_order"], case["name"]


# ---- the feature store ------------------------------------------------------------------------------------------------------------------

def test_features_entry_reads_the_store(ctx):
    rng = np.random.default_rng(9)
    store_rows, nq, n = 5000, 3, CHUNK + 30
    cat = rng.integers(0, 4, store_rows).astype(np.int32)
    author = (rng.integers(0, 50, store_rows).astype(np.int64) << 33) - 7
    fs = pa.Features(ctx, store_rows)
    try:
        fs.set_column("category", pa.F_I32, cat, default=-3)
        fs.set_column("author", pa.F_I64, author, default=11)
        fs.set_column("price", pa.F_F32, rng.random(store_rows).astype(np.float32))
        fs.set_column("empty", pa.F_I32, None, default=1)
        rows = np.stack([rng.permutation(store_rows + 400)[:n] for _ in range(nq)]).astype(np.uint64)   # some rows lie outside the store
        rows[0, :3] = [np.iinfo(np.uint64).max, store_rows, store_rows - 1]
        inside = rows < store_rows
        safe = np.where(inside, rows, 0).astype(np.int64)
        dims = np.stack([np.where(inside, cat[safe], -3), np.where(inside, author[safe], 11)]).astype(np.int64)
        assert (~inside).sum() > 50
        cfg = {"size": 60, "rules": [{"dims": [0], "window": 4, "frequency": 1, "weight": 1}, {"dims": [1, 0], "interval": 1}],
               "exclusions": [{"positions": [1, 2], "terms": [(0, ref.EQ, -3)]}]}
        count = np.array([n, n - 100, 5], np.uint32)
        want = check(ctx, cfg, dims, count)
        assert np.array_equal(ctx.diversity_rules_features(cfg, fs, ["category", "author"], rows, count), want)
        # a column set without values holds its default in every row: it is served, and reads as a constant plane
        const = np.stack([dims[0], np.ones_like(dims[0])])
        assert np.array_equal(ctx.diversity_rules_features(cfg, fs, ["category", "empty"], rows, count), check(ctx, cfg, const, count))
        for names, word in ((["category", "price"], "int32 / int64"), (["category", "nope"], "no column")):
            with pytest.raises(pa._lib.PgError) as ei:
                ctx.diversity_rules_features(cfg, fs, names, rows, count)
            assert ei.value.code == -1 and word in str(ei.value)
        assert np.array_equal(ctx.diversity_rules_features(cfg, fs, ["category", "author"], rows, count), want)     # the context is still usable
    finally:
        fs.destroy()


# ---- stream order ------------------------------------------------------------------------------------------------------------------------

def test_two_calls_back_to_back_need_no_synchronise_between_them(ctx):
    """both calls use the same context scratch: the second is ordered behind the first on the context's stream"""
    rng = np.random.default_rng(10)
    nq, n = 4, CHUNK + 50
    dims_a, dims_b = rng.integers(0, 3, (2, nq, n)), rng.integers(0, 5, (2, nq, n))
    cfg_a = {"size": 50, "rules": [{"dims": [0], "interval": 1}, {"dims": [1], "window": 5, "frequency": 2, "weight": 1}]}
    cfg_b = {"size": 35, "rules": [{"dims": [0, 1], "window": 9, "frequency": 1}], "exclusions": [{"positions": [1, 4], "terms": [(0, ref.EQ, 0)]}]}
    want_a, want_b = check(ctx, cfg_a, dims_a), check(ctx, cfg_b, dims_b)
    bufs = [ctx.to_device(np.ascontiguousarray(dims_a, dtype=np.int64)), ctx.to_device(np.ascontiguousarray(dims_b, dtype=np.int64)),
            ctx.malloc(nq * n * 4), ctx.malloc(nq * n * 4)]
    try:
        ctx.diversity_rules_dev(cfg_a, 2, nq, n, 0, bufs[0], 0, 0, bufs[2])
        ctx.diversity_rules_dev(cfg_b, 2, nq, n, 0, bufs[1], 0, 0, bufs[3])
        ctx.synchronize()
        got_a, got_b = np.empty((nq, n), np.uint32), np.empty((nq, n), np.uint32)
        ctx.d2h(got_a, bufs[2])
        ctx.d2h(got_b, bufs[3])
    finally:
        for b in bufs:
            ctx.free(b)
    assert np.array_equal(got_a, want_a) and np.array_equal(got_b, want_b)
