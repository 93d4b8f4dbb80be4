"""GPU tests of the shard-side exchange calls — the glue kernels of the multi-GPU path (csrc/group.hip, misc.hip, the merge of
recall_select.hip) — each against its plain numpy statement in tests/shard_ref.py, bit for bit: rows and slots exact, scores as uint32 /
uint64 bits, NaN by NaN-ness.  Every output buffer is filled with a sentinel first (0xA5 bytes) and carries a guard region behind
the specified extent; whatever the call is not specified to write must still hold the sentinel afterwards.  Refusal cases pass
only arguments the host checks before anything is launched."""
import contextlib

import numpy as np
import pytest

import pairec_amd as pa
import shard_ref as sr
from oracle import oracle as o

pytestmark = pytest.mark.gpu

PAD = sr.PAD
GUARD = 64                                     # elements behind every output's specified extent
SENT = 0xA5


class Bufs:
    """device buffers of one test, freed together"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def put(self, a):
        p = self.ctx.to_device(np.ascontiguousarray(a))
        self.ptrs.append(p)
        return p

    def out(self, n, dtype):
        """n elements + GUARD, every byte the sentinel"""
        return self.put(np.full((n + GUARD) * np.dtype(dtype).itemsize, SENT, dtype=np.uint8))

    def get(self, p, n, dtype):
        """(the n specified elements, guard untouched?)"""
        a = np.zeros(n + GUARD, dtype=dtype)
        self.ctx.d2h(a, p)
        return a[:n], bool(np.all(a[n:].view(np.uint8) == SENT))

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []


@contextlib.contextmanager
def bufs(ctx):
    b = Bufs(ctx)
    try:
        yield b
    finally:
        b.free()


def sentinel(n, dtype):
    return np.full(n * np.dtype(dtype).itemsize, SENT, dtype=np.uint8).view(dtype)


@contextlib.contextmanager
def knobs(ctx, **kv):
    """context knobs for the duration of a case; the defaults (csrc/common.hpp) come back whatever happens"""
    defaults = {"rank_sort_max": 32, "split_sort_max": 96}
    try:
        for name, v in kv.items():
            ctx.set_option(name, v)
        yield
    finally:
        for name in kv:
            ctx.set_option(name, defaults[name])


# ---- merge --------------------------------------------------------------------------------------------------------------------
MERGE_SIZES = [(1, 1, 1, 1), (1, 2, 1, 1), (3, 4, 250, 1000), (3, 4, 300, 1000), (2, 8, 100, 1000), (256, 2, 40, 64),
               (5, 3, 700, 2000), (1, 8, 2048, 16384)]
MERGE_KINDS = ["shuffled", "all_equal", "ties_at_cut", "specials", "pad_mid", "pad_list", "pad_request", "row_edges"]
SPECIALS = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001,
                     0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32).view(np.float32)


def merge_lists(nq, nlists, per_list, k, kind, seed=0):
    """rows / scores [nq][nlists][per_list], rows distinct within a request (the keys of a merge are distinct: shards are disjoint)
    and below 2^32 - 1; lists are NOT sorted (the merge does not rely on it)"""
    rng = np.random.default_rng([seed, nq, nlists, per_list, k, MERGE_KINDS.index(kind)])
    per_q = nlists * per_list
    rows = np.stack([rng.choice(4_000_000, per_q, replace=False) for _ in range(nq)]).astype(np.uint64) * np.uint64(1000) + np.uint64(7)
    sc = rng.standard_normal((nq, per_q)).astype(np.float32)
    if kind == "all_equal":
        sc[:] = np.float32(0.25)
    elif kind == "ties_at_cut":
        sc = rng.choice(np.array([1.0, 0.5, -2.0], dtype=np.float32), size=(nq, per_q))
    elif kind == "specials":
        hit = rng.random((nq, per_q)) < 0.3
        sc[hit] = rng.choice(SPECIALS, size=int(hit.sum()))
        sc[:, :min(per_q, SPECIALS.shape[0])] = SPECIALS[:per_q]
        sc = rng.permuted(sc, axis=1)
    elif kind == "pad_mid":
        rows[rng.random((nq, per_q)) < 0.2] = PAD
        rows[:, per_q // 2] = PAD
    rows, sc = rows.reshape(nq, nlists, per_list), np.ascontiguousarray(sc).reshape(nq, nlists, per_list)
    if kind == "pad_list":
        rows[:, nlists // 2] = PAD
    elif kind == "pad_request":
        rows[nq // 2] = PAD
    elif kind == "row_edges":
        rows[:, 0, 0] = 0
        rows[:, -1, -1] = 0xFFFFFFFE
    return rows, sc


def run_merge(ctx, api, rows, sc, k, repeat=1):
    """one of the three entry points on query-major inputs → [(rows [nq][k], scores [nq][k])] per repetition"""
    nq, nlists, per_list = rows.shape
    if api == "lists_major":
        rows, sc = rows.transpose(1, 0, 2), sc.transpose(1, 0, 2)
    res = []
    with bufs(ctx) as b:
        d_r, d_s = b.put(rows), b.put(sc)
        for _ in range(repeat):
            d_or, d_os = b.out(nq * k, np.uint64), b.out(nq * k, np.float32)
            if api == "merge":
                rc = ctx.L.pg_topk_merge_dev(ctx.h, d_r, d_s, nq, nlists, per_list, k, d_or, d_os)
            else:
                rc = ctx.L.pg_topk_merge_lists_dev(ctx.h, d_r, d_s, nq, nlists, per_list, int(api == "lists_major"), k, d_or, d_os)
            pa._lib.check(rc)
            out_r, ok_r = b.get(d_or, nq * k, np.uint64)
            out_s, ok_s = b.get(d_os, nq * k, np.float32)
            assert ok_r and ok_s, "%s wrote behind its [nq][k] outputs" % api
            res.append((out_r.reshape(nq, k), out_s.reshape(nq, k)))
    return res


def check_merge(ctx, size, kind, apis=("merge", "lists", "lists_major")):
    nq, nlists, per_list, k = size
    rows, sc = merge_lists(nq, nlists, per_list, k, kind)
    want_r, want_s = sr.merge_ref(rows, sc, k)
    for api in apis:
        runs = run_merge(ctx, api, rows, sc, k, repeat=3 if api == apis[0] else 1)
        for got_r, got_s in runs:
            bad = np.argwhere(got_r != want_r)
            assert bad.shape[0] == 0, "%s %s %s: rows differ first at %s" % (api, size, kind, bad[:3].tolist())
            assert sr.same_bits(got_s, want_s), "%s %s %s: scores differ" % (api, size, kind)
            # (a NaN leaves the merge as THE quiet NaN: the key holds no payload)
            assert np.all(sr.bits(got_s)[np.isnan(got_s)] == 0x7FC00000)
        # the same call three times: the same bits (the atomicAdd order of merge_keys_kernel must not reach the output)
        for got_r, got_s in runs[1:]:
            assert np.array_equal(got_r, runs[0][0]) and np.array_equal(sr.bits(got_s), sr.bits(runs[0][1]))


@pytest.mark.parametrize("kind", MERGE_KINDS)
@pytest.mark.parametrize("size", MERGE_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_merge_entry_points_equal_the_ref(ctx, size, kind):
    """merge_keys_kernel → select_kernel → final_launch through pg_topk_merge_dev and pg_topk_merge_lists_dev (list_major 0 / 1:
    the strides l * row_ls + q * row_qs of merge_keys_kernel) = merge_ref.  Sizes: one entry; k below, at and above the number of
    real entries (select_kernel's M <= K copy path against its radix select; the padded tail of every final kernel); 256 requests;
    k = 16384 > 8192 (final_kernel / the 128 KB LDS of final_rank_kernel).  Contents: unsorted lists; every score equal (lowest rows
    win: the row half of topk_key); ties straddling the k cut (the select's last digit); NaN / inf / signed zeros / denormals
    (f32_ordered_bits, key_score); padding in the middle of lists, a whole padded list, a request with nothing but padding between
    full ones (cnt[q] = 0); rows 0 and 2^32 - 2 (the ends of key_row).  Three calls give the same bits."""
    check_merge(ctx, size, kind)


@pytest.mark.parametrize("kind", ["shuffled", "specials", "pad_mid", "pad_request"])
@pytest.mark.parametrize("size", [(5, 3, 700, 2000), (3, 4, 1100, 5000), (1, 8, 2048, 16384)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kn", [{}, {"rank_sort_max": 0}, {"rank_sort_max": 0, "split_sort_max": 0}],
                         ids=["default", "no_rank", "no_rank_no_split"])
def test_merge_final_branches_on_short_lists(ctx, kn, size, kind):
    """final_launch's branches, each on merged lists short of k (padding, or 4 x 1100 < 5000): final_rank_kernel (default knobs),
    split_sort_launch with FinalSortPolicy::tail (rank_sort_max = 0), final_kernel_reg (also split_sort_max = 0; k <= 8192) and
    final_kernel (k = 16384 with rank_sort_max = 0) — their `i < n ? entry : (UINT64_MAX, -inf)` tails and count clamps."""
    with knobs(ctx, **kn):
        check_merge(ctx, size, kind, apis=("lists_major", "merge"))


def test_merge_refusals_leave_the_context_usable(ctx):
    """the host checks of topk_merge_strided_locked: nq 0 / 257, k 0 / 16385, nlists * per_list = 0 and beyond k + 2^19 — an error
    code each, nothing launched, and the next valid merge on the same context is right"""
    with bufs(ctx) as b:
        d_r, d_s = b.put(np.zeros(64, np.uint64)), b.put(np.zeros(64, np.float32))
        d_or, d_os = b.out(64, np.uint64), b.out(64, np.float32)
        bad = [(0, 2, 4, 4), (257, 2, 4, 4), (1, 2, 4, 0), (1, 2, 4, 16385), (1, 0, 4, 4), (1, 2, 0, 4),
               (1, 1, 4 + (1 << 19) + 1, 4), (1, (1 << 19) + 8, 1, 7)]
        for nq, nlists, per_list, k in bad:
            assert ctx.L.pg_topk_merge_dev(ctx.h, d_r, d_s, nq, nlists, per_list, k, d_or, d_os) != 0, (nq, nlists, per_list, k)
            for lm in (0, 1):
                assert ctx.L.pg_topk_merge_lists_dev(ctx.h, d_r, d_s, nq, nlists, per_list, lm, k, d_or, d_os) != 0
            with pytest.raises(pa._lib.PgError):
                pa._lib.check(ctx.L.pg_topk_merge_dev(ctx.h, d_r, d_s, nq, nlists, per_list, k, d_or, d_os))
        assert b.get(d_or, 64, np.uint64)[1] and np.all(b.get(d_or, 64, np.uint64)[0].view(np.uint8) == SENT)
    check_merge(ctx, (3, 4, 300, 1000), "shuffled")


# ---- owned compaction ------------------------------------------------------------------------------------------------------------
OFF, NROWS = 1000, 500


@pytest.fixture(scope="module")
def shard(ctx):
    """a 500-row, dim-64 shard at row_offset 1000 and its rows on the host (computed once, never changed)"""
    tab = np.random.default_rng(11).standard_normal((NROWS, 64)).astype(np.float32)
    t = pa.Table(ctx, NROWS, 64, row_offset=OFF)
    t.upload(tab)
    yield t, tab
    t.destroy()


def compact_rows(nq, k, kind):
    rng = np.random.default_rng([nq, k, len(kind)])
    edge = np.array([999, 1000, 1499, 1500, 0, 0xFFFFFFFFFFFFFFFF, 1 << 32, (1 << 32) + 1200, (1 << 63) + 1001], dtype=np.uint64)
    if kind == "mixed":
        rows = rng.integers(700, 1800, size=(nq, k)).astype(np.uint64)
        hit = rng.random((nq, k)) < 0.3
        rows[hit] = rng.choice(edge, size=int(hit.sum()))
        rows.reshape(-1)[:min(nq * k, edge.shape[0])] = edge[:nq * k]
    elif kind == "all":
        rows = rng.integers(OFF, OFF + NROWS, size=(nq, k)).astype(np.uint64)
    elif kind == "none":
        rows = rng.choice(edge[[0, 3, 4, 5, 6, 7, 8]], size=(nq, k))
    elif kind == "alternating":
        rows = np.where((np.arange(nq * k).reshape(nq, k) % 2) == 0, np.uint64(1234), np.uint64(1500)).astype(np.uint64)
    elif kind == "last":                       # the only owned entry at j = k - 1
        rows = np.full((nq, k), PAD, dtype=np.uint64)
        rows[:, k - 1] = 1499
    elif kind == "at_1024":                    # ... and at j = 1024, the first entry of owned_fill_kernel's second pass
        rows = np.full((nq, k), 1500, dtype=np.uint64)
        rows[:, 1024] = 1000
    return np.ascontiguousarray(rows)


COMPACT_SIZES = [(1, 1), (1, 1023), (1, 1024), (1, 1025), (3, 2049), (255, 7), (256, 5), (256, 300), (2, 16384)]
COMPACT_CASES = [(nq, k, kind) for nq, k in COMPACT_SIZES for kind in ("mixed", "all", "none", "alternating", "last", "at_1024")
                 if kind != "at_1024" or k > 1024]                             # (an entry j = 1024 needs a list that long)


@pytest.mark.parametrize("nq,k,kind", COMPACT_CASES)
def test_owned_compact_equals_the_ref(ctx, shard, nq, k, kind):
    """owned_count_kernel (256-thread strided count and tree), owned_scan_kernel (t == nq - 1 writes off[nq]; nq = 255 / 256 fill the
    one workgroup) and owned_fill_kernel (1024-entry passes: k = 1023 / 1024 / 1025 / 2049 / 16384 around the pass boundary, `base`
    carried between passes, the only owned entry at j = k - 1 or at j = 1024) = owned_compact_ref.  Ownership: ids 999 / 1000 / 1499 /
    1500 at the ends of [1000, 1500), 0, UINT64_MAX, ids >= 2^32 (r - off must not be truncated before the compare).  All nq + 1
    offsets, local / slot up to the total, nothing behind it."""
    t, _ = shard
    rows = compact_rows(nq, k, kind)
    local, slot, off = sr.owned_compact_ref(rows, OFF, NROWS)
    total = int(off[-1])
    with bufs(ctx) as b:
        d_rows = b.put(rows)
        d_local, d_slot, d_off = b.out(nq * k, np.uint32), b.out(nq * k, np.uint32), b.out(nq + 1, np.uint32)
        pa._lib.check(ctx.L.pg_owned_compact_dev(ctx.h, t.h, d_rows, nq, k, d_local, d_slot, d_off))
        g_off, ok_o = b.get(d_off, nq + 1, np.uint32)
        g_local, ok_l = b.get(d_local, nq * k, np.uint32)
        g_slot, ok_s = b.get(d_slot, nq * k, np.uint32)
    assert ok_o and ok_l and ok_s
    assert np.array_equal(g_off, off), np.argwhere(g_off != off)[:4].tolist()
    assert np.array_equal(g_local[:total], local) and np.array_equal(g_slot[:total], slot)
    assert np.all(g_local[total:].view(np.uint8) == SENT) and np.all(g_slot[total:].view(np.uint8) == SENT)


def test_owned_compact_refusals(ctx, shard):
    """pg_owned_compact_dev's host checks: nq 0 / 257, k 0"""
    t, _ = shard
    with bufs(ctx) as b:
        d_rows = b.put(np.zeros(64, np.uint64))
        d_local, d_slot, d_off = b.out(64, np.uint32), b.out(64, np.uint32), b.out(64, np.uint32)
        for nq, k in ((0, 4), (257, 4), (1, 0)):
            assert ctx.L.pg_owned_compact_dev(ctx.h, t.h, d_rows, nq, k, d_local, d_slot, d_off) != 0
        pa._lib.check(ctx.L.pg_owned_compact_dev(ctx.h, t.h, d_rows, 2, 4, d_local, d_slot, d_off))
        assert b.get(d_off, 64, np.uint32)[0][:3].tolist() == [0, 0, 0]


# ---- scatter -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,total", [(700, 0), (700, 700), (700, 705), (700, 300), (1, 1), (256, 261), (0, 5)])
def test_scatter_f32_equals_the_ref(ctx, cap, total):
    """scatter_scores_kernel: `i < cap && i < *total` with the total read from a device word — 0 (nothing moves), cap, cap + 5 (must
    clip at cap: entries cap … cap + 4 stay where they are); cap = 0 launches nothing.  Values travel as bits (a NaN payload, -0.0)."""
    rng = np.random.default_rng(cap * 1000 + total)
    n_out = 2000
    vals = rng.standard_normal(max(cap, 1) + 8).astype(np.float32)
    vals.view(np.uint32)[:2] = [0x7FC12345, 0x80000000]
    slot = rng.permutation(n_out)[:max(cap, 1) + 8].astype(np.uint32)
    want = sr.scatter_ref(vals, slot, total, cap, sentinel(n_out, np.float32))
    with bufs(ctx) as b:
        d_out = b.out(n_out, np.float32)
        pa._lib.check(ctx.L.pg_scatter_f32_dev(ctx.h, b.put(vals), b.put(slot), b.put(np.array([total], np.uint32)), cap, d_out))
        got, ok = b.get(d_out, n_out, np.float32)
    assert ok and np.array_equal(sr.bits(got), sr.bits(want))
    assert int((sr.bits(got) != sr.bits(sentinel(n_out, np.float32))).sum()) == min(cap, total)


# ---- DPP candidates -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,k,n_cand", [(1, 1, 1), (3, 300, 1), (3, 300, 300), (256, 40, 17), (2, 16384, 8192)])
def test_dpp_candidates_equal_the_ref(ctx, nq, k, n_cand):
    """sorted_head_kernel: c[q * C + j] = x[q * k + order[q * k + j]] — the two strides (k for the lists, C for the head) with C = 1,
    C < k, C = k; every request's order a random permutation (a kernel that read order[j] of the wrong request, or j + 1, shows);
    rows with padding, fused scores with NaN payloads: both travel as bits."""
    rng = np.random.default_rng([nq, k, n_cand])
    order = np.stack([rng.permutation(k) for _ in range(nq)]).astype(np.uint32)
    rows = rng.integers(0, 1 << 40, size=(nq, k)).astype(np.uint64)
    rows[rng.random((nq, k)) < 0.1] = PAD
    fused = rng.standard_normal((nq, k))
    nan = rng.random((nq, k)) < 0.1
    fused.view(np.uint64)[nan] = np.uint64(0x7FF8000000000000) + rng.integers(1, 1 << 30, size=int(nan.sum())).astype(np.uint64)
    want_r, want_f = sr.sorted_head_ref(order, rows, fused, n_cand)
    with bufs(ctx) as b:
        d_cr, d_cf = b.out(nq * n_cand, np.uint64), b.out(nq * n_cand, np.float64)
        pa._lib.check(ctx.L.pg_dpp_candidates_dev(ctx.h, b.put(order), b.put(rows), b.put(fused), nq, k, n_cand, d_cr, d_cf))
        got_r, ok_r = b.get(d_cr, nq * n_cand, np.uint64)
        got_f, ok_f = b.get(d_cf, nq * n_cand, np.float64)
    assert ok_r and ok_f
    assert np.array_equal(got_r, want_r) and np.array_equal(sr.bits(got_f), sr.bits(want_f))


def test_dpp_candidates_refusals(ctx):
    """pg_dpp_candidates_dev's host check: n_cand 0 and k + 1"""
    with bufs(ctx) as b:
        d_o, d_r, d_f = b.put(np.zeros(64, np.uint32)), b.put(np.zeros(64, np.uint64)), b.put(np.zeros(64, np.float64))
        d_cr, d_cf = b.out(64, np.uint64), b.out(64, np.float64)
        for n_cand in (0, 9):
            assert ctx.L.pg_dpp_candidates_dev(ctx.h, d_o, d_r, d_f, 2, 8, n_cand, d_cr, d_cf) != 0
        assert np.all(b.get(d_cr, 64, np.uint64)[0].view(np.uint8) == SENT)
        pa._lib.check(ctx.L.pg_dpp_candidates_dev(ctx.h, d_o, d_r, d_f, 2, 8, 8, d_cr, d_cf))
        assert np.all(b.get(d_cr, 16, np.uint64)[0] == 0)


# ---- owned embedding rows -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dim_tables(ctx):
    out = {}
    for dim in (64, 128, 256):
        tab = np.random.default_rng(dim).standard_normal((300, dim)).astype(np.float32)
        tab.view(np.uint32)[0, :3] = [0x7FC00055, 0x80000000, 0x00000001]        # rows travel as bits
        t = pa.Table(ctx, 300, dim, row_offset=7000)
        t.upload(tab)
        out[dim] = (t, tab)
    yield out
    for t, _ in out.values():
        t.destroy()


@pytest.mark.parametrize("n", [1, 255, 257, 5000])
@pytest.mark.parametrize("dim", [64, 128, 256])
def test_gather_owned_rows_equal_the_ref(ctx, dim_tables, dim, n):
    """gather_global_rows_kernel: thread gid → (entry gid / (dim / 4), float4 gid % (dim / 4)) for dim 64 / 128 / 256, n around the
    256-thread block and beyond; row_offset 7000 (the `r - off` of the source row); duplicates, the ids at both ends of the range and
    just outside, padding and foreign ids.  Owned rows are bit-equal to the table; every other destination row still holds the
    sentinel (the kernel must not zero or touch what it does not own)."""
    t, tab = dim_tables[dim]
    rng = np.random.default_rng([dim, n])
    pool = np.array([6999, 7000, 7000, 7299, 7300, 0, 299, 0xFFFFFFFFFFFFFFFF, (1 << 32) + 7001, 7150, 7150], dtype=np.uint64)
    c_rows = np.where(rng.random(n) < 0.5, rng.integers(6900, 7400, size=n).astype(np.uint64), rng.choice(pool, size=n))
    c_rows[:min(n, pool.shape[0])] = pool[:n]
    c_rows = np.ascontiguousarray(rng.permutation(c_rows))
    want = sr.gather_owned_ref(tab, 7000, c_rows, sentinel(n * dim, np.float32).reshape(n, dim))
    with bufs(ctx) as b:
        d_out = b.out(n * dim, np.float32)
        pa._lib.check(ctx.L.pg_gather_owned_rows_dev(ctx.h, t.h, b.put(c_rows), n, d_out))
        got, ok = b.get(d_out, n * dim, np.float32)
    assert ok and np.array_equal(sr.bits(got.reshape(n, dim)), sr.bits(want))


# ---- rows → local, widening ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_owned", [True, False])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 3000])
def test_rows_to_local_equals_the_ref(ctx, shard, n, with_owned):
    """rows_to_local_kernel: local = r - off for an owned row, 0 for a foreign one or padding (ids 999 / 1000 / 1499 / 1500, 0,
    UINT64_MAX, >= 2^32), the owned byte only when d_owned is given; n = 0 launches nothing, n around the 256-thread block."""
    t, _ = shard
    rng = np.random.default_rng(n)
    edge = np.array([999, 1000, 1499, 1500, 0, 0xFFFFFFFFFFFFFFFF, 1 << 32, (1 << 32) + 1200], dtype=np.uint64)
    rows = np.where(rng.random(max(n, 1)) < 0.6, rng.integers(800, 1700, size=max(n, 1)).astype(np.uint64), rng.choice(edge, size=max(n, 1)))
    rows[:min(n, 8)] = edge[:n]
    rows = np.ascontiguousarray(rows)
    loc, own = sr.rows_to_local_ref(rows[:n], OFF, NROWS)
    with bufs(ctx) as b:
        d_local, d_owned = b.out(n, np.uint32), b.out(n, np.uint8)
        pa._lib.check(ctx.L.pg_rows_to_local_dev(ctx.h, t.h, b.put(rows), n, d_local, d_owned if with_owned else None))
        g_loc, ok_l = b.get(d_local, n, np.uint32)
        g_own, ok_o = b.get(d_owned, n, np.uint8)
    assert ok_l and ok_o and np.array_equal(g_loc, loc)
    assert np.array_equal(g_own, own) if with_owned else np.all(g_own == SENT)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_widen_f32_equals_the_oracle(ctx, n):
    """widen_kernel = o.widen_f32 (the float → double conversion is exact): signed zeros, infinities, NaN, the largest float, the
    smallest normal and the smallest denormal — a kernel built or run with denormals flushed turns 1.4e-45 into 0 and fails here."""
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x80800000,
                        0x00000001, 0x80000001, 0x007FFFFF], dtype=np.uint32).view(np.float32)
    x = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    x[-min(n, special.shape[0]):] = special[:n][::-1] if n < special.shape[0] else special
    if n == 1:
        x[0] = special[9]                                                      # the smallest denormal
    want = o.widen_f32(x)
    with bufs(ctx) as b:
        d_out = b.out(n, np.float64)
        pa._lib.check(ctx.L.pg_widen_f32_dev(ctx.h, b.put(x), n, d_out))
        got, ok = b.get(d_out, n, np.float64)
    assert ok and sr.same_bits(got, want)
    assert np.all(got[x != 0] != 0), "a denormal was flushed to zero"
