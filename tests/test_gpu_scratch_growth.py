"""A scratch slot that grows between calls (csrc/api.cpp scratch_reserve; the layouts of csrc/blend.hip and csrc/diversity.hip):
small -> large -> small on ONE fresh context, every answer equal to the library's host statement.  The arena hands out whole
MiB: the small calls' layouts lie far below one granule, the large calls' above it, so the second call frees and reallocates the
slot — with the total its layout states — and the third runs in the grown buffer.

  blend, SNAKE with 4 entries: offsets (n_seg + 1) x 4 | orders n_seg x cap x 4 | keys n_seg x cap x 8 | lists n_seg x cap x 4 |
    picks nq x out_cap x 4, n_seg = 4 nq.  nq = 2, cap = 64: under 9 KiB.  nq = 8, cap = 4096: 0.5 + 1 + 0.5 MiB and the picks; its
    32 lists of 4 096 keys also take the split sort, whose runs (32 x 4096 x 12 B = 1.5 MiB) grow the shared work slot under it.
  diversity, 2 rules: keys and counts nq x 2 x cap x 4 each | tables (nq << bits) x 4 with 2^bits >= max(2 cap, 1024).
    nq = 2, cap = 64: 10 KiB.  nq = 16, cap = 8192: 1 + 1 + 1 MiB."""
import numpy as np
import pytest

import blend_ref
import pairec_amd as pa

pytestmark = pytest.mark.gpu

SMALL_LARGE_SMALL = ("small", "large", "small")


@pytest.fixture()
def fresh_ctx():
    """a context whose slots are all empty (the session's has served other tests)"""
    c = pa.Context(0)
    yield c
    c.close()


def blend_case(seed, nq, cap, n_src=4):
    rng = np.random.default_rng(seed)
    rows = rng.permutation(nq * cap).reshape(nq, cap).astype(np.uint64) + np.uint64(1 << 20)
    rows[rng.random((nq, cap)) < 0.05] = blend_ref.U64MAX
    score = rng.standard_normal((nq, cap))
    tie = rng.random((nq, cap)) < 0.3
    score[tie] = rng.integers(-2, 3, (nq, cap))[tie] * 0.5
    source = rng.integers(0, n_src, (nq, cap)).astype(np.uint8)
    count = rng.integers(cap // 2, cap + 1, nq).astype(np.uint32)
    mask = np.uint32(1) << source.astype(np.uint32)
    p64 = np.full((n_src, nq, cap), np.nan)
    for s in range(n_src):
        held = (rng.random((nq, cap)) < 0.3) & (source != s)
        mask = mask | (held.astype(np.uint32) << np.uint32(s))
        p64[s] = np.where(held, rng.standard_normal((nq, cap)), p64[s])
        p64[s] = np.where(source == s, score, p64[s])
    return rows, score, source, count, p64, mask.astype(np.uint32)


def test_blend_slot_grows_between_calls(fresh_ctx):
    shapes = {"small": (2, 64), "large": (8, 4096)}
    entries = [(3, 2), (2, 1), (1, 5), (0, 1)]
    for mode in (blend_ref.SNAKE_REFILL, blend_ref.SNAKE_SKIP):
        for i, size in enumerate(SMALL_LARGE_SMALL):
            nq, cap = shapes[size]
            conf = (mode, (2 * cap) // 3, entries)
            case = blend_case(100 * mode + i, nq, cap)
            want = pa.candidates_blend_host(conf, *case)
            assert int(want[-1].max()) > cap // 4                        # (a blend that keeps something)
            blend_ref.same(fresh_ctx.candidates_blend(conf, *case), want)


def test_diversity_slot_grows_between_calls(fresh_ctx):
    shapes = {"small": (2, 64), "large": (16, 8192)}
    cfg = {"size": 40, "explore_item_size": 600,
           "rules": [{"dims": [0], "window": 4, "frequency": 1, "weight": 2}, {"dims": [1, 0], "interval": 1}]}
    for i, size in enumerate(SMALL_LARGE_SMALL):
        nq, cap = shapes[size]
        rng = np.random.default_rng(7 + i)
        dims = rng.integers(0, 3, (2, nq, cap)).astype(np.int64)
        count = rng.integers(cap // 2, cap + 1, nq).astype(np.uint32)
        count[0] = cap
        want = pa.diversity_rules_host(cfg, dims, count)
        assert want[0].tolist() != list(range(cap))                      # (rules that move something)
        got = fresh_ctx.diversity_rules(cfg, dims, count)
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s call %d: first difference at request %d slot %d" % (size, i, bad[0][0], bad[0][1])
