"""numpy restatement of what the persistent rank kernels walk (csrc/rank_mlp.hip: build_tiles_*; rank_ws.hip, rank_rs.hip,
rank_2r.hip, rank_is.hip), and the ragged batches tests/test_gpu_rank_persistent.py puts through them.

  tile_table       requests -> tiles of at most `tile_items` items: no tile for a request without items, no tile over two
                   requests, a request's last tile holds what is left
  ranges           workgroup b of G walks tiles [n_tiles * b / G, n_tiles * (b + 1) / G)
  ragged_requests  a seeded batch of the edge sizes, one run of 1-item requests longer than the prefetch depth, one run of
                   three empty requests, an empty first and last request
  coverage         what such a batch makes the kernels' tile loops do, in figures; check_coverage names the conditions
                   (the issue's "coverage conditions") a batch misses
  batch_for        the batch of a (tile_items, G): the first seed whose batch meets every condition
  chunks           the same requests cut at request boundaries into calls of at most `max_tiles` tiles: zero tiles or one
                   per workgroup, the regime the other rank tests hold to the oracle item by item
  sample_items     the stratified sample the oracle scores"""
from collections import namedtuple

import numpy as np

EDGE_SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 257, 333, 700, 5000)
ONE_RUN = 12              # consecutive 1-item requests: every tile a new request for longer than the prefetch depth (3)
EMPTY_RUN = 3             # consecutive requests without items, between two that have some
IS_WAVES = 8              # rank_is.hip: a workgroup's waves take tiles t_begin + wave, + 8, ...
# tiles per workgroup the batches aim at: a range has to hold the whole 1-item run (12 tiles) with room to spare, which is
# more than the 5 a steady-state loop needs (prefetch depth 3 + the tail); the per-wave kernel needs 3 per wave
TILES_PER_WG = 14
TILES_PER_WG_WAVES = 3 * IS_WAVES

TileTable = namedtuple("TileTable", "tile_req tile_item0 tile_cnt tile_items")
Batch = namedtuple("Batch", "sizes offsets one_run empty_run")       # the runs as (first request, number of requests)


def tile_table(req_offsets, tile_items):
    off = np.asarray(req_offsets, dtype=np.int64)
    n_req = off.size - 1
    per = (np.diff(off) + tile_items - 1) // tile_items
    tile_req = np.repeat(np.arange(n_req, dtype=np.int64), per)
    req_tile0 = np.concatenate([[0], np.cumsum(per)])[:-1]
    k = np.arange(tile_req.size, dtype=np.int64) - req_tile0[tile_req]
    tile_item0 = off[tile_req] + k * tile_items
    tile_cnt = np.minimum(tile_items, off[tile_req + 1] - tile_item0)
    return TileTable(tile_req, tile_item0, tile_cnt, tile_items)


def ranges(n_tiles, G):
    """t_begin [G], t_end [G] as the kernels compute them (64-bit product, truncating division)"""
    b = np.arange(G + 1, dtype=np.int64)
    edge = (n_tiles * b) // G
    return edge[:-1], edge[1:]


def ragged_requests(seed, target_items):
    rng = np.random.default_rng(seed)
    pieces = [[1] * ONE_RUN, [65] + [0] * EMPTY_RUN + [129]]
    total = ONE_RUN + 65 + 129
    while total < target_items:
        for s in rng.permutation(EDGE_SIZES):
            pieces.append([int(s)])
            total += int(s)
            if total >= target_items:
                break
    order = rng.permutation(len(pieces))
    sizes, one_run, empty_run = [0], None, None
    for p in order:
        if p == 0:
            one_run = (len(sizes), ONE_RUN)
        if p == 1:
            empty_run = (len(sizes) + 1, EMPTY_RUN)
        sizes.extend(pieces[p])
    sizes.append(0)
    sizes = np.asarray(sizes, dtype=np.int64)
    return Batch(sizes, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32), one_run, empty_run)


def one_run_tiles(batch, tt):
    """tile indices of the 1-item run (one tile per request)"""
    r0, n = batch.one_run
    t = np.nonzero((tt.tile_req >= r0) & (tt.tile_req < r0 + n))[0]
    assert t.size == n and np.all(tt.tile_cnt[t] == 1)
    return t


def empty_run_tiles(batch, tt):
    """the last tile before the run of empty requests and the first one behind it"""
    r0, n = batch.empty_run
    assert np.all(batch.sizes[r0:r0 + n] == 0) and batch.sizes[r0 - 1] > 0 and batch.sizes[r0 + n] > 0
    before = np.nonzero(tt.tile_req == r0 - 1)[0][-1]
    after = np.nonzero(tt.tile_req == r0 + n)[0][0]
    assert after == before + 1
    return np.array([before, after])


def partial_then_full(tt, t_begin, t_end):
    """per range: the tiles t with tile_cnt < tile_items whose successor t + 1 is full and in the same range"""
    n = tt.tile_cnt.size
    hit = np.zeros(n, bool)
    hit[:-1] = (tt.tile_cnt[:-1] < tt.tile_items) & (tt.tile_cnt[1:] == tt.tile_items)
    out = []
    for b, e in zip(t_begin, t_end):
        out.append(np.nonzero(hit[b:max(e - 1, b)])[0] + b)
    return out


def coverage(batch, tt, G, waves=1):
    n_tiles = tt.tile_req.size
    tb, te = ranges(n_tiles, G)
    length = te - tb
    partial = tt.tile_cnt < tt.tile_items
    change = np.zeros(n_tiles, bool)
    change[1:] = tt.tile_req[1:] != tt.tile_req[:-1]
    csum = np.concatenate([[0], np.cumsum(change)])
    # a change inside a range: between two of ITS tiles (the first tile of a range always loads the request)
    ranges_with_change = int(np.sum(csum[np.maximum(te, tb + 1)] - csum[tb + 1] > 0))
    ptf = partial_then_full(tt, tb, te)
    run = one_run_tiles(batch, tt)
    wg_first = np.searchsorted(te, run[0], side="right")
    wg_last = np.searchsorted(te, run[-1], side="right")
    nonempty = length > 0
    return {
        "n_tiles": n_tiles, "G": G, "min_range": int(length.min()),
        "min_tiles_per_wave": int(length.min() // waves),           # (the last wave of the shortest range)
        "ranges_with_request_change": ranges_with_change,
        "ranges_with_partial_then_full": int(sum(1 for x in ptf if x.size)),
        "one_run_inside_one_range": bool(wg_first == wg_last),
        "ranges_starting_partial": int(np.sum(partial[tb[nonempty]])),
        "ranges_ending_partial": int(np.sum(partial[te[nonempty] - 1])),
    }


def check_coverage(batch, tt, G, waves=1):
    """the conditions the GPU tests rely on; returns the ones that do not hold (none: the batch is fit for use)"""
    c = coverage(batch, tt, G, waves)
    missed = []
    if c["min_range"] < 5:
        missed.append("a workgroup's range has %d tiles (< 5)" % c["min_range"])
    if waves > 1 and c["min_tiles_per_wave"] < 3:
        missed.append("a wave has %d tiles (< 3)" % c["min_tiles_per_wave"])
    if 4 * c["ranges_with_request_change"] < G:
        missed.append("%d of %d ranges contain a request change (< a quarter)" % (c["ranges_with_request_change"], G))
    if c["ranges_with_partial_then_full"] < 16:
        missed.append("%d ranges contain a partial tile followed by a full one (< 16)" % c["ranges_with_partial_then_full"])
    if not c["one_run_inside_one_range"]:
        missed.append("the 1-item run straddles a range boundary")
    if c["ranges_starting_partial"] < 1:
        missed.append("no range starts with a partial tile")
    if c["ranges_ending_partial"] < 1:
        missed.append("no range ends with a partial tile")
    return missed


def target_items(tile_items, G, waves=1):
    return (TILES_PER_WG_WAVES if waves > 1 else TILES_PER_WG) * G * tile_items


# (tile_items, G, waves) -> the first seed of range(MAX_SEED) whose batch meets every condition, written down for the
# workgroup counts of an MI355X (256 CUs; 512 where two register-stationary workgroups share a CU) and held to that by
# tests/test_rank_tiles_cpu.py; another device's count is searched the same way
SEEDS = {(64, 256, 1): 4, (64, 512, 1): 2, (128, 256, 1): 1, (32, 256, IS_WAVES): 2}
MAX_SEED = 64


def batch_for(tile_items, G, waves=1):
    """(seed, batch, tile table) or (None, None, the conditions the last seed missed)"""
    target = target_items(tile_items, G, waves)
    known = SEEDS.get((tile_items, G, waves))
    missed = None
    for seed in ([known] if known is not None else range(MAX_SEED)):
        batch = ragged_requests(seed, target)
        tt = tile_table(batch.offsets, tile_items)
        missed = check_coverage(batch, tt, G, waves)
        if not missed:
            return seed, batch, tt
    return None, None, missed


def chunks(sizes, tile_items, max_tiles):
    """[(r0, r1)]: consecutive request ranges of at most max_tiles tiles each, as few as a greedy cut makes them"""
    per = (np.asarray(sizes, dtype=np.int64) + tile_items - 1) // tile_items
    if per.size and per.max() > max_tiles:
        raise ValueError("a request of %d tiles does not fit a call of %d" % (per.max(), max_tiles))
    out, r0, acc = [], 0, 0
    for r, p in enumerate(per):
        if acc + p > max_tiles:
            out.append((r0, r))
            r0, acc = r, 0
        acc += int(p)
    if r0 < per.size:
        out.append((r0, per.size))
    return out


def tile_items_of(tt, tiles):
    tiles = np.asarray(tiles, dtype=np.int64)
    if tiles.size == 0:
        return np.zeros(0, np.int64)
    return np.concatenate([np.arange(tt.tile_item0[t], tt.tile_item0[t] + tt.tile_cnt[t]) for t in tiles])


def sample_items(batch, tt, G, seed, n_ranges=16, n_random=2000):
    """sorted item indices: the first and last tile of n_ranges ranges (the first range, the last, seeded picks), the
    1-item run, the tiles around the empty run, every partial tile followed by a full one (both) in n_ranges ranges, and
    n_random random items.  Whole tiles, so that every slot of a tile is seen: 4 500 to 7 500 items with 32- and 64-item
    tiles, 10 000 to 12 000 with 128-item tiles."""
    rng = np.random.default_rng(seed)
    n_tiles = tt.tile_req.size
    n_items = int(batch.offsets[-1])
    tb, te = ranges(n_tiles, G)
    live = np.nonzero(te > tb)[0]
    picks = np.unique(np.concatenate([[live[0], live[-1]], rng.choice(live, min(n_ranges - 2, live.size), replace=False)]))
    tiles = [tb[picks], te[picks] - 1, one_run_tiles(batch, tt), empty_run_tiles(batch, tt)]
    ptf = partial_then_full(tt, tb, te)
    with_ptf = np.array([b for b in range(G) if ptf[b].size], dtype=np.int64)
    for b in rng.choice(with_ptf, min(n_ranges, with_ptf.size), replace=False):
        tiles += [ptf[b], ptf[b] + 1]
    fixed = np.unique(tile_items_of(tt, np.unique(np.concatenate(tiles))))
    return np.unique(np.concatenate([fixed, rng.choice(n_items, min(n_random, n_items), replace=False)]))


def locate(tt, G, item, waves=1):
    """where an item sits in the big call: (tile, workgroup, position of the tile in the workgroup's range, range length)"""
    t = int(np.searchsorted(tt.tile_item0, item, side="right") - 1)
    tb, te = ranges(tt.tile_req.size, G)
    b = int(np.searchsorted(te, t, side="right"))
    return {"item": int(item), "tile": t, "request": int(tt.tile_req[t]), "slot": int(item - tt.tile_item0[t]), "tile_cnt": int(tt.tile_cnt[t]),
            "workgroup": b, "pos_in_range": int(t - tb[b]), "range_len": int(te[b] - tb[b]),
            **({"wave": int((t - tb[b]) % waves), "trip": int((t - tb[b]) // waves)} if waves > 1 else {})}
