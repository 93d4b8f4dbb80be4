"""GPU tests of the recalls with per-request exclusion lists.  The compaction kernel alone on synthetic ordered
inputs; the direct calls, the attached index and the coalescer against tests/exclude_ref.py (the CPU oracle at depth k + n_q,
the listed ids dropped, cut to k, padded): ids, order, score bits, padding and counts must match."""
import ctypes as C
import threading

import numpy as np
import pytest

import exclude_ref as ref
import pairec_amd as pa
from oracle import oracle as o

pytestmark = pytest.mark.gpu

U64MAX = ref.U64MAX
CHUNK, WAVE, SET_SLOTS = 1024, 64, 8192          # exclude.hip: entries per step of the walk, lanes per ballot, slots of the set
HASH_MUL = np.uint64(0x9E3779B97F4A7C15)         # ... and its hash: (id * HASH_MUL) >> 51


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1]))
    assert np.array_equal(np.asarray(got[2], np.uint32), np.asarray(want[2], np.uint32))


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------

def ordered_input(rng, nq, k_in, id_pool=None):
    """[nq][k_in] distinct ids per request with descending scores of arbitrary bits (two equal now and then)"""
    rows = np.empty((nq, k_in), np.uint64)
    for q in range(nq):
        rows[q] = (rng.choice(id_pool, k_in, replace=False) if id_pool is not None
                   else rng.choice(1 << 40, k_in, replace=False).astype(np.uint64) + np.uint64(1 << 33))
    sc = -np.sort(-rng.standard_normal((nq, k_in)).astype(np.float32), axis=1)
    sc[:, 1::7] = sc[:, 0::7][:, :sc[:, 1::7].shape[1]]
    return rows, sc


def compact_ref(rows, sc, lists, k_out, pad):
    nq = rows.shape[0]
    out = (np.empty((nq, k_out), np.uint64), np.empty((nq, k_out), np.float32), np.empty(nq, np.uint32))
    for q in range(nq):
        r, s, c = ref.drop_cut_pad(rows[q], sc[q], lists[q], k_out)
        s[c:] = pad
        out[0][q], out[1][q], out[2][q] = r, s, c
    return out


def check_compact(ctx, rows, sc, lists, k_out, pad=-np.inf):
    got = ctx.exclude_compact(rows, sc, lists, k_out, pad)
    assert_same(got, compact_ref(rows, sc, lists, k_out, pad))
    return got


@pytest.mark.parametrize("k_in", [1, 63, 64, 65, 1000, 16384])
def test_kernel_sizes_and_empty_lists(ctx, k_in):
    rng = np.random.default_rng(k_in)
    rows, sc = ordered_input(rng, 4, k_in)
    some = rng.choice(rows[1], min(4096, max(1, k_in // 3)), replace=False)
    # none / some / the head (all of it up to 4096 entries, the longest list) / every other entry
    lists = [np.zeros(0, np.uint64), some, rows[2][:4096].copy(), rows[3][::2][:4096].copy()]
    for k_out in sorted({1, max(1, k_in // 2), k_in}):
        got = check_compact(ctx, rows, sc, lists, k_out, pad=np.float32(-7.5))
        # an empty list: the head of the input, bit for bit
        assert np.array_equal(got[0][0], rows[0][:k_out]) and np.array_equal(bits(got[1][0]), bits(sc[0][:k_out]))
        if k_in <= 4096:
            assert got[2][2] == 0 and np.all(got[0][2] == U64MAX) and np.all(got[1][2] == np.float32(-7.5))
        else:
            assert got[2][2] == min(k_out, k_in - 4096) and got[0][2][0] == rows[2][4096]
    # every list empty: the lists' pointer may be NULL
    got = check_compact(ctx, rows, sc, [()] * 4, k_in)
    assert np.array_equal(got[0], rows) and np.array_equal(bits(got[1]), bits(sc))


def test_kernel_runs_across_every_chunk_and_wave_boundary(ctx):
    rng = np.random.default_rng(11)
    k_in = 16384
    rows, sc = ordered_input(rng, 3, k_in)
    pos_chunk = np.concatenate([np.arange(b - 3, b + 3) for b in range(CHUNK, k_in, CHUNK)])
    pos_wave = np.concatenate([np.arange(b - 1, b + 1) for b in range(WAVE, k_in, WAVE)])
    pos_tail = np.arange(k_in - 5, k_in)
    lists = [rows[0][pos_chunk], rows[1][pos_wave], rows[2][np.concatenate([np.arange(0, 70), pos_tail])]]
    for k_out in (k_in, k_in - len(pos_chunk), CHUNK, CHUNK + 1, 5000):
        check_compact(ctx, rows, sc, lists, k_out)


def test_kernel_padded_input_duplicates_and_foreign_ids(ctx):
    rng = np.random.default_rng(12)
    k_in = 3000
    rows, sc = ordered_input(rng, 3, k_in)
    rows[0, 2000:], sc[0, 2000:] = U64MAX, -np.inf            # an answer that ends in padding
    rows[1, 1:], sc[1, 1:] = U64MAX, -np.inf
    rows[2, :], sc[2, :] = U64MAX, -np.inf                    # nothing but padding
    dup = rng.choice(rows[0][:2000], 500, replace=False)
    lists = [np.concatenate([dup, dup, dup[:17], [U64MAX, U64MAX, np.uint64(5), np.uint64(1 << 62)]]).astype(np.uint64),
             np.array([U64MAX], np.uint64), np.array([U64MAX, rows[0][0]], np.uint64)]
    for k_out in (3000, 2000, 1499, 1):
        got = check_compact(ctx, rows, sc, lists, k_out)
    assert got[2].tolist() == [1, 1, 0]
    got = check_compact(ctx, rows, sc, lists, 3000)
    assert got[2].tolist() == [1500, 1, 0]


def test_kernel_lists_that_collide_in_the_set(ctx):
    rng = np.random.default_rng(13)
    # 4096 ids equal modulo the set's size, and 4096 ids the implementation's own hash sends to ONE slot
    mod = (np.arange(1, 4097, dtype=np.uint64) * np.uint64(SET_SLOTS))
    target = (np.uint64(1) * HASH_MUL) >> np.uint64(51)
    found, base = [], 1
    while sum(x.size for x in found) < 4096:
        cand = np.arange(base, base + (1 << 22), dtype=np.uint64)
        found.append(cand[((cand * HASH_MUL) >> np.uint64(51)) == target])
        base += 1 << 22
    same = np.concatenate(found)[:4096]
    assert same.size == 4096 and int(target) < SET_SLOTS
    k_in = 6000
    for ids in (mod, same):
        others = rng.choice(1 << 40, k_in, replace=False).astype(np.uint64) + np.uint64(1 << 33)
        pool = np.concatenate([ids, others[:k_in - 4096 + 500]])
        rows, sc = ordered_input(rng, 2, k_in, id_pool=pool)
        lists = [ids, rng.permutation(ids)[:4000]]
        check_compact(ctx, rows, sc, lists, 5000)
        check_compact(ctx, rows, sc, lists, 1500)


def test_kernel_256_requests_of_mixed_lengths(ctx):
    rng = np.random.default_rng(14)
    nq, k_in, k_out = 256, 6000, 5000
    rows, sc = ordered_input(rng, nq, k_in)
    lens = [0, 1, 4096, 64, 300, 4095, 2, 1000]
    lists = []
    for q in range(nq):
        n = lens[q % len(lens)]
        mine = rng.choice(rows[q], min(n, k_in), replace=False)
        lists.append(mine if q % 3 else np.concatenate([mine[: n // 2], rows[(q + 1) % nq][: n - n // 2]]))      # half foreign
    got = check_compact(ctx, rows, sc, lists, k_out)
    assert got[2].min() < k_out and got[2].max() == k_out
    L = ctx.L
    assert L.pg_exclude_compact_dev(ctx.h, 8, 8, 257, 10, 8, 8, 10, 0.0, 8, 8, None) == -1
    assert L.pg_exclude_compact_dev(ctx.h, 8, 8, 1, 10, 8, 8, 11, 0.0, 8, 8, None) == -4
    assert L.pg_exclude_compact_dev(ctx.h, 8, 8, 1, 16385, 8, 8, 10, 0.0, 8, 8, None) == -4
    assert L.pg_exclude_compact_dev(ctx.h, 8, 8, 1, 10, 8, 8, 0, 0.0, 8, 8, None) == -4


# ---- the direct calls ---------------------------------------------------------------------------------------------------------

N1, D1, OFF1 = 120_000, 128, 4_000_000_000
N2, D2 = 20_000, 64


class World:
    pass


@pytest.fixture(scope="module")
def world(ctx):
    w = World()
    rng = np.random.default_rng(0xE0)
    w.tab1 = o.synth_rows(o.SEED_TABLE, 0, N1, D1) * rng.uniform(0.7, 1.3, (N1, 1)).astype(np.float32)
    w.t1 = pa.Table(ctx, N1, D1, row_offset=OFF1)
    w.t1.upload(w.tab1)
    w.q1 = o.synth_rows(o.SEED_QUERY, 0, 64, D1)
    w.tab2 = o.synth_rows(o.SEED_TABLE, 9, N2, D2)
    w.t2 = pa.Table(ctx, N2, D2)
    w.t2.upload(w.tab2)
    w.q2 = o.synth_rows(o.SEED_QUERY, 100, 64, D2)
    w.cols = {"status": rng.integers(0, 2, N1).astype(np.int32), "cat": rng.integers(0, 8, N1).astype(np.int32)}
    w.feats = pa.Features(ctx, N1)
    for name, v in w.cols.items():
        w.feats.set_column(name, pa.F_I32, v)
    w.feats2 = pa.Features(ctx, N2)
    w.feats2.set_column("cat", pa.F_I32, w.cols["cat"][:N2])
    yield w
    w.feats.destroy()
    w.feats2.destroy()
    w.t1.destroy()
    w.t2.destroy()


def biting_lists(rng, tab, q, k, lens, l2, row_offset=0, mask=None):
    """lists of the given lengths, each drawn from its query's own plain top-(k + n) so that it bites"""
    lists = []
    for i, n in enumerate(lens):
        top, _ = ref.plain_top(tab, q[i], k + n, l2, row_offset, mask)
        lists.append(rng.choice(top, min(n, top.size), replace=False) if n else np.zeros(0, np.uint64))
    return lists


SHAPES = [(1, [1]), (1, [4096]), (5, [0, 1, 300, 300, 1]), (64, [0, 1, 300, 4096] * 16)]


@pytest.mark.parametrize("l2", [False, True], ids=["ip", "l2"])
@pytest.mark.parametrize("which", [1, 2], ids=["120000x128", "20000x64"])
@pytest.mark.parametrize("k", [50, 5000])
def test_direct_calls_equal_the_restatement(ctx, world, which, l2, k):
    tab, t, q, off = (world.tab1, world.t1, world.q1, OFF1) if which == 1 else (world.tab2, world.t2, world.q2, 0)
    rng = np.random.default_rng(100 * which + 10 * l2 + k)
    for nq, lens in SHAPES:
        lists = biting_lists(rng, tab, q[:nq], k, lens, l2, off)
        got = t.recall_topk_exclude(q[:nq], k, lists, l2=l2)
        want = ref.recall_exclude(tab, q[:nq], k, lists, l2, off)
        assert_same(got, want)
        assert got[2].tolist() == [k] * nq
        for i in range(nq):
            assert not np.isin(got[0][i], lists[i]).any()


def test_device_form_equals_the_host_form(ctx, world):
    t, q, k, nq = world.t2, world.q2[:5], 50, 5
    rng = np.random.default_rng(3)
    lists = biting_lists(rng, world.tab2, q, k, [0, 1, 300, 300, 7], False)
    want = t.recall_topk_exclude(q, k, lists)
    ids, offs = pa.engine._pack_lists(lists, nq)
    offs = offs + np.uint32(3)                               # offsets need not start at 0
    ids = np.concatenate([np.zeros(3, np.uint64), ids])
    bufs = [ctx.to_device(q), ctx.to_device(ids), ctx.malloc(nq * k * 8), ctx.malloc(nq * k * 4)]
    cnt = np.zeros(nq, np.uint32)
    opts = pa._lib.PgRecallExcludeOpts(0, None, None)
    try:
        pa._lib.check(ctx.L.pg_recall_topk_exclude_dev(ctx.h, t.h, C.c_void_p(bufs[0]), nq, k, C.c_void_p(bufs[1]), offs.ctypes.data,
                                                       C.byref(opts), C.c_void_p(bufs[2]), C.c_void_p(bufs[3]), cnt.ctypes.data))
        rows, sc = np.empty((nq, k), np.uint64), np.empty((nq, k), np.float32)
        ctx.d2h(rows, bufs[2])
        ctx.d2h(sc, bufs[3])
    finally:
        for b in bufs:
            ctx.free(b)
    assert_same((rows, sc, cnt), want)


@pytest.mark.parametrize("l2", [False, True], ids=["ip", "l2"])
def test_compound_clause_and_view(ctx, world, l2):
    rng = np.random.default_rng(21 + l2)
    k, nq = 50, 5
    mask = (world.cols["status"] == 1) & np.isin(world.cols["cat"], [1, 3, 5])
    w = pa.Where("status = 1 AND cat IN (1, 3, 5)")
    try:
        q = world.q1[:nq]
        lists = biting_lists(rng, world.tab1, q, k, [0, 1, 300, 300, 64], l2, OFF1, mask)
        plain, _ = ref.plain_top(world.tab1, q[1], 5, l2, OFF1)             # best rows the clause need not admit: no effect
        lists[1] = np.concatenate([lists[1], plain[~mask[(plain - np.uint64(OFF1)).astype(np.int64)]]]).astype(np.uint64)
        got = world.t1.recall_topk_exclude(q, k, lists, l2=l2, feats=world.feats, where=w)
        assert_same(got, ref.recall_exclude(world.tab1, q, k, lists, l2, OFF1, mask))
        empty = world.t1.recall_topk_exclude(q, k, None, l2=l2, feats=world.feats, where=w)
        assert_same(empty, world.t1.recall_topk_where_ex(world.feats, w, q, k, l2=l2))
    finally:
        w.free()
    # a view: the lists hold the source's ids; fewer rows than k survive
    m2 = world.cols["cat"][:N2] == 3
    view = world.t2.view(world.feats2, "cat", "==", 3)
    try:
        k2, q2 = 5000, world.q2[:nq]
        assert m2.sum() < k2
        lists = biting_lists(rng, world.tab2, q2, 50, [0, 1, 300, 300, 64], l2, 0, m2)
        got = view.recall_topk_exclude(q2, k2, lists, l2=l2)
        assert_same(got, ref.recall_exclude(world.tab2, q2, k2, lists, l2, 0, m2))
        assert got[2].tolist() == [int(m2.sum()) - len(x) for x in lists]
        got = view.recall_topk_exclude(q2, 50, lists, l2=l2)
        assert_same(got, ref.recall_exclude(world.tab2, q2, 50, lists, l2, 0, m2))
    finally:
        view.destroy()


def test_refusals_and_empty_lists(ctx, world):
    t, q = world.t2, world.q2[:3]
    with pytest.raises(pa._lib.PgError) as e:
        t.recall_topk_exclude(q, 16000, [(), np.arange(385, dtype=np.uint64), ()])
    assert e.value.code == -4 and "16000" in str(e.value) and "385" in str(e.value)
    with pytest.raises(pa._lib.PgError) as e:
        t.recall_topk_exclude(q, 10, [(), np.arange(4097, dtype=np.uint64), ()])
    assert e.value.code == -4
    rows, sc, cnt = np.empty((3, 10), np.uint64), np.empty((3, 10), np.float32), np.zeros(3, np.uint32)
    ids = np.arange(8, dtype=np.uint64)
    L = ctx.L

    def call(offs, opts=None, ids_ptr=ids.ctypes.data):
        offs = None if offs is None else np.asarray(offs, np.uint32)
        return L.pg_recall_topk_exclude(ctx.h, t.h, q.ctypes.data, 3, 10, ids_ptr, None if offs is None else offs.ctypes.data,
                                        opts, rows.ctypes.data, sc.ctypes.data, cnt.ctypes.data)

    assert call(None) == -1
    assert call([0, 5, 3, 8]) == -1
    assert call([4, 2, 2, 2]) == -1
    assert call([0, 2, 4, 8], ids_ptr=None) == -1
    assert call([0, 2, 4, 8]) == 0
    assert call([0, 2, 4, 8], C.byref(pa._lib.PgRecallExcludeOpts(2, None, None))) == -1
    assert call([0, 2, 4, 8], C.byref(pa._lib.PgRecallExcludeOpts(0, world.feats2.h, None))) == -1
    # the checks of the call being extended come first
    assert L.pg_recall_topk_exclude(ctx.h, t.h, q.ctypes.data, 3, 0, None, None, None, rows.ctypes.data, sc.ctypes.data, None) == -4
    assert L.pg_recall_topk_exclude(ctx.h, t.h, q.ctypes.data, 257, 10, None, None, None, rows.ctypes.data, sc.ctypes.data, None) == -1
    # every list empty: the plain call bit for bit — at k itself (k = 16384 leaves no room above)
    for l2 in (False, True):
        for k in (50, 16384):
            plain = t.recall_topk_l2(q, k) if l2 else t.recall_topk(q, k)
            assert_same(t.recall_topk_exclude(q, k, None, l2=l2), plain)
            assert_same(t.recall_topk_exclude(q, k, [(), (), ()], l2=l2), plain)


def test_i2i_without_the_trigger(ctx, world):
    t, tab, k = world.t2, world.tab2, 50
    trig = np.array([0, 77, 4096, N2 - 1, 12345], np.uint32)
    plain = t.i2i_recall(trig, k + 1)
    assert np.array_equal(plain[0][:, 0], trig.astype(np.uint64))          # (unit rows: an item is its own best match)
    got = t.i2i_recall(trig, k, exclude_trigger=True)
    assert not (got[0] == trig[:, None].astype(np.uint64)).any()
    assert np.array_equal(got[0], plain[0][:, 1:]) and np.array_equal(bits(got[1]), bits(plain[1][:, 1:]))
    assert got[2].tolist() == [k] * 5
    assert_same(got, ref.recall_exclude(tab, tab[trig], k, [[r] for r in trig], False))
    # lists and the trigger together; lists alone; neither = the plain call
    rng = np.random.default_rng(8)
    lists = biting_lists(rng, tab, tab[trig], k + 1, [0, 1, 300, 17, 4095], False)
    got = t.i2i_recall(trig, k, exclude_trigger=True, lists=lists)
    assert_same(got, ref.recall_exclude(tab, tab[trig], k, [np.append(x, np.uint64(r)) for x, r in zip(lists, trig)], False))
    got = t.i2i_recall(trig, k, lists=lists)
    assert_same(got, ref.recall_exclude(tab, tab[trig], k, lists, False))
    assert_same(t.i2i_recall(trig, k, lists=[()] * 5), t.i2i_recall(trig, k))
    # the trigger table on a global row offset: its own row id is what is excluded
    trig1 = np.array([5, 100_000], np.uint32)
    got = world.t1.i2i_recall(trig1, k, exclude_trigger=True)
    assert_same(got, ref.recall_exclude(world.tab1, world.tab1[trig1], k, [[OFF1 + int(r)] for r in trig1], False, OFF1))
    with pytest.raises(pa._lib.PgError) as e:
        other = pa.Table(ctx, 1000, D2)
        try:
            other.fill_synthetic(3)
            t.i2i_recall(trig[:1], k, trigger_table=other, exclude_trigger=True)
        finally:
            other.destroy()
    assert e.value.code == -1
    with pytest.raises(pa._lib.PgError) as e:
        t.i2i_recall(trig[:1], k, exclude_trigger=True, lists=[np.arange(4096, dtype=np.uint64)])
    assert e.value.code == -4


# ---- through an attached index ------------------------------------------------------------------------------------------------

def test_attached_index_serves_the_inner_recall(ctx):
    n, d, centres, sigma, seed, k = 60_000, 128, 40, 0.1, 0x1DE, 50
    t = pa.Table(ctx, n, d)
    t.fill_mixture(seed, centres, sigma)
    tab = o.synth_mixture_rows(seed, 0, n, d, centres, sigma)
    q = o.synth_mixture_rows(seed, 777, 5, d, centres, sigma, stream=1)
    rng = np.random.default_rng(31)
    ix = None
    try:
        # (the dense rule is calibrated at 100 M rows, DESIGN.md 4.1f: lifted so that the plan serves on this small table)
        ctx.set_option("index_dense_fraction", 1e6)
        cases = []
        for l2 in (False, True):
            lists = biting_lists(rng, tab, q, k, [0, 1, 300, 4096, 300], l2)
            cases.append((l2, lists, t.recall_topk_exclude(q, k, lists, l2=l2)))
            assert_same(cases[-1][2], ref.recall_exclude(tab, q, k, lists, l2))
        ix = pa.Index(ctx, t)
        ix.attach()
        held0 = ix.serving_stats()["plans_held"]
        for l2, lists, before in cases:
            assert_same(t.recall_topk_exclude(q, k, lists, l2=l2), before)
        assert ix.serving_stats()["plans_held"] > held0
    finally:
        ctx.set_option("index_dense_fraction", 0.01)
        if ix is not None:
            try:
                ix.detach()
            except pa._lib.PgError:
                pass
            ix.destroy()
        t.destroy()


# ---- the coalescer ------------------------------------------------------------------------------------------------------------

def test_coalescer_recall_exclude(ctx, world):
    t, tab, k, mx = world.t2, world.tab2, 50, 512
    threads, per = 8, 20
    rng = np.random.default_rng(41)
    lens = [0, 1, 37, 512, 0, 200]
    reqs = []
    for i in range(threads * per):
        qi = i % 64
        n = lens[i % len(lens)]
        top, _ = ref.plain_top(tab, world.q2[qi], k + n, False)
        reqs.append((qi, rng.choice(top, n, replace=False) if n else np.zeros(0, np.uint64)))
    direct = [None] * len(reqs)
    for s in range(0, len(reqs), 64):
        part = reqs[s:s + 64]
        out = t.recall_topk_exclude(world.q2[[qi for qi, _ in part]], k, [x for _, x in part])
        for j in range(len(part)):
            direct[s + j] = (out[0][j], out[1][j], out[2][j])
    plain = t.recall_topk(world.q2, k)
    # created without the option: the entry is refused
    co0 = pa.Coalescer(ctx, t, k, max_wait_us=500)
    try:
        with pytest.raises(pa._lib.PgError) as e:
            co0.recall_exclude(world.q2[0], reqs[1][1])
        assert e.value.code == -4
    finally:
        co0.destroy()
    with pytest.raises(pa._lib.PgError) as e:
        ctx.set_option("coalescer_max_exclude", 4097)
    assert e.value.code == -1
    co = None
    try:
        ctx.set_option("coalescer_max_exclude", 4096)
        with pytest.raises(pa._lib.PgError) as e:
            pa.Coalescer(ctx, t, 13000)
        assert e.value.code == -4
        ctx.set_option("coalescer_max_exclude", mx)
        co = pa.Coalescer(ctx, t, k, max_wait_us=2000)
        ctx.set_option("coalescer_max_exclude", 0)              # (read once, at creation)
        got = [None] * len(reqs)
        got_plain = [None] * threads
        errors = []
        gate = threading.Barrier(threads)

        def worker(w):
            try:
                gate.wait()
                for j in range(per):
                    i = w * per + j
                    got[i] = co.recall_exclude(world.q2[reqs[i][0]], reqs[i][1])
                    if j == per // 2:
                        got_plain[w] = co.recall(world.q2[w])
            except Exception as ex:          # noqa: BLE001
                errors.append(ex)

        th = [threading.Thread(target=worker, args=(w,)) for w in range(threads)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errors, errors
        for i in range(len(reqs)):
            assert np.array_equal(got[i][0], direct[i][0]), i
            assert np.array_equal(bits(got[i][1]), bits(direct[i][1])), i
            assert got[i][2] == direct[i][2] == k
        for w in range(threads):
            assert np.array_equal(got_plain[w][0], plain[0][w]) and np.array_equal(bits(got_plain[w][1]), bits(plain[1][w]))
            assert got_plain[w][2] == k
        st = co.stats()
        assert st.requests[0] == threads * per + threads
        with pytest.raises(pa._lib.PgError) as e:
            co.recall_exclude(world.q2[0], np.arange(mx + 1, dtype=np.uint64))
        assert e.value.code == -4
    finally:
        ctx.set_option("coalescer_max_exclude", 0)
        if co is not None:
            co.destroy()
