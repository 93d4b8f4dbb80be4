"""CPU tests of tests/rank_tiles_ref.py: the numpy tile table against a plain loop, and the batches of
tests/test_gpu_rank_persistent.py against the conditions that make them a test of the persistent kernels' tile loops —
shown here for the workgroup counts of an MI355X (256, and 512 where two workgroups share a CU) with the seeds written
down in rank_tiles_ref.SEEDS, asserted again on the device for the count it reports."""
import numpy as np
import pytest

import rank_tiles_ref as rt

CONFIGS = [(64, 256, 1), (64, 512, 1), (128, 256, 1), (32, 256, rt.IS_WAVES)]      # (tile items, workgroups, waves)


def _tiles_by_loop(off, tile_items):
    req, item0, cnt = [], [], []
    for r in range(len(off) - 1):
        i = int(off[r])
        while i < int(off[r + 1]):
            req.append(r)
            item0.append(i)
            cnt.append(min(tile_items, int(off[r + 1]) - i))
            i += tile_items
    return np.array(req), np.array(item0), np.array(cnt)


@pytest.mark.parametrize("tile_items", [32, 64, 128])
def test_tile_table_is_the_loop_over_requests(tile_items):
    sizes = [0, 0, 5000, 1, 0, 333, 128, 129, 64, 65, 127, 257, 0, 0, 0, 1, 1, 32, 33, 31, 256, 0]
    off = np.concatenate([[0], np.cumsum(sizes)])
    tt = rt.tile_table(off, tile_items)
    req, item0, cnt = _tiles_by_loop(off, tile_items)
    assert np.array_equal(tt.tile_req, req) and np.array_equal(tt.tile_item0, item0) and np.array_equal(tt.tile_cnt, cnt)
    assert tt.tile_cnt.min() >= 1 and tt.tile_cnt.sum() == off[-1]
    assert not np.isin(np.nonzero(np.array(sizes) == 0)[0], tt.tile_req).any()          # no tile for an empty request
    assert np.all(off[tt.tile_req] <= tt.tile_item0) and np.all(tt.tile_item0 + tt.tile_cnt <= off[tt.tile_req + 1])
    last = np.concatenate([tt.tile_req[1:] != tt.tile_req[:-1], [True]])
    assert np.all(tt.tile_cnt[~last] == tile_items)                                     # only a request's last tile is short
    assert rt.tile_table([0], tile_items).tile_req.size == 0 and rt.tile_table([0, 0, 0], tile_items).tile_req.size == 0


@pytest.mark.parametrize("n_tiles,G", [(0, 256), (1, 256), (255, 256), (256, 256), (257, 256), (3853, 256), (7586, 512), (2 ** 31 + 5, 304)])
def test_ranges_partition_the_tiles(n_tiles, G):
    tb, te = rt.ranges(n_tiles, G)
    assert tb[0] == 0 and te[-1] == n_tiles and np.array_equal(tb[1:], te[:-1])
    assert (te - tb).min() == n_tiles // G and (te - tb).max() == -(-n_tiles // G)
    for b in (0, 1, G // 3, G - 1):
        assert tb[b] == (n_tiles * b) // G and te[b] == (n_tiles * (b + 1)) // G


def test_ragged_requests_hold_every_piece():
    for seed in range(6):
        b = rt.ragged_requests(seed, 100_000)
        s = b.sizes
        assert s[0] == 0 and s[-1] == 0 and set(s.tolist()) == set(rt.EDGE_SIZES)
        assert 100_000 <= s.sum() < 100_000 + 5000 and np.array_equal(b.offsets, np.concatenate([[0], np.cumsum(s)]))
        r0, n = b.one_run
        assert n >= 12 and np.all(s[r0:r0 + n] == 1)
        r0, n = b.empty_run
        assert n == 3 and np.all(s[r0:r0 + n] == 0) and s[r0 - 1] > 0 and s[r0 + n] > 0
        again = rt.ragged_requests(seed, 100_000)
        assert np.array_equal(again.sizes, s) and again.one_run == b.one_run and again.empty_run == b.empty_run
    assert not np.array_equal(rt.ragged_requests(0, 100_000).sizes, rt.ragged_requests(1, 100_000).sizes)


@pytest.mark.parametrize("tile_items,G,waves", CONFIGS)
def test_committed_seeds_meet_the_coverage_conditions(tile_items, G, waves):
    seed, batch, tt = rt.batch_for(tile_items, G, waves)
    assert seed is not None and seed == rt.SEEDS[(tile_items, G, waves)], tt
    assert rt.check_coverage(batch, tt, G, waves) == []
    c = rt.coverage(batch, tt, G, waves)
    print(tile_items, G, waves, "seed", seed, "items", int(batch.offsets[-1]), c)
    # the conditions once more, from the tile table alone
    tb, te = rt.ranges(tt.tile_req.size, G)
    assert tt.tile_req.size >= 5 * G and (te - tb).min() >= 5
    if waves > 1:
        for b in (0, int(np.argmin(te - tb)), G - 1):
            assert min(len(range(tb[b] + w, te[b], waves)) for w in range(waves)) >= 3
    full = tt.tile_cnt == tile_items
    n_change = n_ptf = starts = ends = 0
    for b in range(G):
        r = tt.tile_req[tb[b]:te[b]]
        n_change += bool(np.any(r[1:] != r[:-1]))
        f = full[tb[b]:te[b]]
        n_ptf += bool(np.any(~f[:-1] & f[1:]))
        starts += not f[0]
        ends += not f[-1]
    assert (n_change, n_ptf, starts, ends) == (c["ranges_with_request_change"], c["ranges_with_partial_then_full"],
                                               c["ranges_starting_partial"], c["ranges_ending_partial"])
    assert 4 * n_change >= G and n_ptf >= 16 and starts >= 1 and ends >= 1
    run = rt.one_run_tiles(batch, tt)
    assert run.size >= 12 and np.array_equal(run, np.arange(run[0], run[0] + run.size))
    inside = [b for b in range(G) if tb[b] <= run[0] and run[-1] < te[b]]
    assert len(inside) == 1
    # the seed written down is the first that does it: the search finds it again
    known = rt.SEEDS.pop((tile_items, G, waves))
    try:
        assert rt.batch_for(tile_items, G, waves)[0] == known
    finally:
        rt.SEEDS[(tile_items, G, waves)] = known


def test_a_batch_that_misses_a_condition_is_named():
    batch = rt.ragged_requests(0, 20_000)
    tt = rt.tile_table(batch.offsets, 64)
    missed = rt.check_coverage(batch, tt, 256)
    assert any("< 5" in m for m in missed)                                       # about one tile per workgroup
    assert any("wave has" in m for m in rt.check_coverage(batch, tt, 16, rt.IS_WAVES))


@pytest.mark.parametrize("tile_items,G,waves", CONFIGS)
def test_chunks_cover_every_request_once_in_order(tile_items, G, waves):
    _, batch, tt = rt.batch_for(tile_items, G, waves)
    ch = rt.chunks(batch.sizes, tile_items, G)
    assert ch[0][0] == 0 and ch[-1][1] == batch.sizes.size
    assert all(a[1] == b[0] for a, b in zip(ch[:-1], ch[1:])) and all(r0 < r1 for r0, r1 in ch)
    per = (batch.sizes + tile_items - 1) // tile_items
    assert all(per[r0:r1].sum() <= G for r0, r1 in ch)
    # greedy: the next request would not have fitted
    assert all(per[r0:r1].sum() + per[r1] > G for r0, r1 in ch[:-1])
    assert sum(per[r0:r1].sum() for r0, r1 in ch) == tt.tile_req.size
    print(tile_items, G, "chunks", len(ch))


def test_chunks_at_the_limit():
    assert rt.chunks([5000], 64, 79) == [(0, 1)] and rt.chunks([5000], 128, 40) == [(0, 1)]
    with pytest.raises(ValueError):
        rt.chunks([5000], 64, 78)
    assert rt.chunks([64, 64, 65, 0, 0, 1], 64, 2) == [(0, 2), (2, 5), (5, 6)]
    assert rt.chunks([0, 0], 64, 4) == [(0, 2)] and rt.chunks([], 64, 4) == []


@pytest.mark.parametrize("tile_items,G,waves", CONFIGS)
def test_sample_holds_its_strata(tile_items, G, waves):
    _, batch, tt = rt.batch_for(tile_items, G, waves)
    s = rt.sample_items(batch, tt, G, seed=5)
    assert np.array_equal(s, np.unique(s)) and s[0] >= 0 and s[-1] < batch.offsets[-1]
    tb, te = rt.ranges(tt.tile_req.size, G)
    for t in (tb[0], te[0] - 1, tb[G - 1], te[G - 1] - 1, *rt.one_run_tiles(batch, tt), *rt.empty_run_tiles(batch, tt)):
        assert np.isin(rt.tile_items_of(tt, [t]), s).all()
    ptf = rt.partial_then_full(tt, tb, te)
    whole = [b for b in range(G) if ptf[b].size and np.isin(rt.tile_items_of(tt, np.concatenate([ptf[b], ptf[b] + 1])), s).all()]
    assert len(whole) >= 16
    assert 2000 <= s.size <= 14_000
    where = rt.locate(tt, G, int(s[-1]), waves)
    assert where["workgroup"] == G - 1 and where["pos_in_range"] == where["range_len"] - 1
