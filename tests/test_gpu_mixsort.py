"""GPU tests of MultiRecallMixSort on the device (csrc/mixsort.hip: pg_mix_sort_dev, pg_mix_sort) against
tests/mixsort_ref.py, by bits: every element of out_order and out_count.  List lengths sit on the kernel's edges (S - 1, S, a wave
of 64, the chunk of 1 024, two chunks and one), several lengths travel in one call as ragged counts, and every output carries a
guard region behind it that must stay untouched.  The host statement (pg_mix_sort_host) is held against the same answers."""
import numpy as np
import pytest

import mixsort_ref as ref
import pairec_amd as pa
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

ROWS, OUTSIDE = 600, 40                        # store rows; candidate rows reach OUTSIDE rows past the store
HUGE = np.uint64((1 << 40) + 5)
DTYPES = {"cat": np.int32, "flag": np.int64, "posi": np.int32, "posl": np.int64, "w": np.float32}
F_OF = {np.int32: pa.F_I32, np.int64: pa.F_I64, np.float32: pa.F_F32}
DECL = [(n, F_OF[t]) for n, t in DTYPES.items()]
GUARD = 256


def general(S):
    """four strategies: FIX with duplicate positions and positions beyond S, claimed by a source mask and a condition at once; FIX
    through a position column (values <= 0, duplicates, beyond S) claimed by an item and a user condition; two RANDOM ones that
    overlap the first (a float condition, a source mask)"""
    return [
        {"MixStrategy": "fix_position", "Positions": [3, 1, 3, 7, 200, 12, 1, S, S + 1], "SourceMask": 0b0010,
         "Conditions": [{"Name": "cat", "Operator": "equal", "Type": "int", "Value": 2}]},
        {"MixStrategy": "fix_position", "PositionField": "posi", "Number": 9,
         "Conditions": [{"Name": "flag", "Operator": "equal", "Type": "int64", "Value": 1},
                        {"Name": "age", "Domain": "user", "Operator": "greater", "Type": "int", "Value": 30}]},
        {"MixStrategy": "random_position", "NumberRate": 0.3, "SourceMask": 0b0101},
        {"MixStrategy": "random_position", "Number": 2, "Conditions": [{"Name": "w", "Operator": "greater", "Type": "float", "Value": 0.5}]},
    ]


class World:
    pass


@pytest.fixture(scope="module")
def world(ctx):
    w = World()
    rng = np.random.default_rng(7741)
    w.store = {"cat": rng.integers(0, 6, ROWS).astype(np.int32), "flag": (rng.random(ROWS) < 0.2).astype(np.int64),
               "posi": rng.integers(-3, 24, ROWS).astype(np.int32), "posl": rng.integers(-3, 5000, ROWS).astype(np.int64),
               "w": rng.random(ROWS).astype(np.float32)}
    w.store["posl"][::7] = (1 << 40) + 3                                      # far beyond any page, and beyond int32
    w.store["posl"][3::11] = -(1 << 35)
    w.fs = pa.Features(ctx, ROWS)
    for n, t in DTYPES.items():
        w.fs.set_column(n, F_OF[t], w.store[n], default=1.0)                  # (a default the sort must never read)
    yield w
    w.fs.destroy()


class Guarded:
    """device buffers with a guard behind every output; outputs are pre-filled, so an element the kernel skips shows as well"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def put(self, a):
        if a is None:
            return 0
        p = self.ctx.to_device(np.ascontiguousarray(a))
        self.bufs.append((p, None, 0))
        return p

    def out(self, a):
        p = self.ctx.malloc(a.nbytes + GUARD)
        self.ctx.h2d(p, np.full(a.nbytes + GUARD, 0xA5, np.uint8))
        self.bufs.append((p, a, a.nbytes))
        return p

    def fetch(self):
        self.ctx.synchronize()
        for p, a, nbytes in self.bufs:
            if a is None:
                continue
            raw = np.empty(nbytes + GUARD, np.uint8)
            self.ctx.d2h(raw, p)
            assert np.all(raw[nbytes:] == 0xA5), "a write behind an output"
            a.reshape(-1).view(np.uint8)[:] = raw[:nbytes]

    def free(self):
        for p, _, _ in self.bufs:
            self.ctx.free(p)


def make_case(rng, nq, cap, counts=None, order=True, seed=True, source=True):
    rows = rng.integers(0, ROWS + OUTSIDE, (nq, cap)).astype(np.uint64)       # (about 6 % outside the store)
    rows[rng.random((nq, cap)) < 0.01] = HUGE
    return dict(nq=nq, cap=cap, rows=rows, source=rng.integers(0, 6, (nq, cap)).astype(np.uint8) if source else None,
                order=np.stack([rng.permutation(cap) for _ in range(nq)]).astype(np.uint32) if order else None,
                count=None if counts is None else np.asarray(counts, dtype=np.uint32),
                seed=rng.integers(0, 1 << 63, nq).astype(np.uint64) if seed else None,
                users=[({"age": 25 + 3 * (q % 5)} if q % 4 != 3 else None) for q in range(nq)])


def gathered(w, case):
    """the store's values by element, and which elements are inside"""
    rows = case["rows"]
    inside = rows < ROWS
    idx = np.where(inside, rows, 0).astype(np.int64)
    return {n: np.where(inside, w.store[n][idx], 0).astype(DTYPES[n]) for n in DTYPES}, inside.astype(np.uint8)


def want(w, strategies, size, remain, ctx_size, case):
    cols, inside = gathered(w, case)
    return ref.mix_sort(strategies, size, remain, ctx_size, case["nq"], case["cap"], cols=cols, item_in=inside, source=case["source"],
                        order=case["order"], count=case["count"], seed=case["seed"], users=case["users"])


def run_dev(ctx, w, mix, ctx_size, case, fs="store"):
    nq, cap = case["nq"], case["cap"]
    uv, up = mix.pack_user(case["users"])
    out, cnt = np.empty((nq, cap), np.uint32), np.empty(nq, np.uint32)
    g = Guarded(ctx)
    try:
        d_in = [g.put(a) for a in (case["rows"], case["source"], case["order"], case["count"], case["seed"], uv, up)]
        d_out = [g.out(out), g.out(cnt)]
        ctx.mix_sort_dev(mix, w.fs if fs == "store" else fs, ctx_size, nq, cap, *d_in, *d_out)
        g.fetch()
    finally:
        g.free()
    return out, cnt


def check(ctx, w, strategies, size, remain, ctx_size, case, mix=None):
    own = mix is None
    mix = mix or pa.mix_compile(strategies, DECL, size, remain)
    try:
        w_out, w_cnt = want(w, strategies, size, remain, ctx_size, case)
        cols, inside = gathered(w, case)
        h_out, h_cnt = mix.sort_host(ctx_size, case["nq"], case["cap"], cols=cols, item_in=inside, source=case["source"], order=case["order"],
                                     count=case["count"], seed=case["seed"], users=case["users"])
        assert np.array_equal(h_out, w_out) and np.array_equal(h_cnt, w_cnt)
        out, cnt = run_dev(ctx, w, mix, ctx_size, case)
        assert np.array_equal(cnt, w_cnt)
        bad = np.argwhere(out != w_out)
        assert bad.size == 0, (bad[:5], out[tuple(bad[0])], w_out[tuple(bad[0])])
    finally:
        if own:
            mix.free()
    return w_out, w_cnt


@pytest.mark.parametrize("S,remain,order", [(10, False, True), (10, True, False), (100, True, True), (100, False, False)])
def test_list_lengths_on_the_edges_as_ragged_counts(ctx, world, S, remain, order):
    """S - 1 (identity), S (every entry is in the page: displaced ones return through the remaining-slot fill), a wave, a chunk, two
    chunks and one — in one call, as d_count"""
    ns = [S - 1, S, 63, 64, 65, 1023, 1024, 1025, 2049]
    rng = np.random.default_rng(100 + S + remain)
    case = make_case(rng, len(ns), 2049, counts=ns, order=order)
    w_out, w_cnt = check(ctx, world, general(S), 0, remain, S, case)
    assert w_cnt.tolist() == [n if n < S or remain else S for n in ns] and np.all(w_out[2, 65:] == ref.EMPTY)


def test_cap_16384_permuted_with_the_tail(ctx, world):
    rng = np.random.default_rng(16384)
    case = make_case(rng, 1, 16384)
    check(ctx, world, general(100), 100, True, 20, case)                      # (the config's size is the larger one)


def test_256_requests_of_96_with_ragged_counts_and_no_seed(ctx, world):
    rng = np.random.default_rng(256)
    case = make_case(rng, 256, 96, counts=rng.integers(0, 97, 256), seed=False)
    case["count"][:4] = [96, 10, 9, 0]
    check(ctx, world, general(10), 0, True, 10, case)


def test_page_of_one_slot_and_three_requests(ctx, world):
    st = [{"MixStrategy": "fix_position", "Positions": [1, 1, 2], "SourceMask": 0b0011},
          {"MixStrategy": "random_position", "Number": 1, "SourceMask": 0b1100}]
    rng = np.random.default_rng(1)
    for remain in (False, True):
        check(ctx, world, st, 0, remain, 1, make_case(rng, 3, 65, counts=[65, 1, 0]))
    check(ctx, world, st, 1, False, 0, make_case(rng, 1, 64, order=False))     # nq = 1, the size from the config alone


def test_page_of_4096_slots(ctx, world):
    st = [{"MixStrategy": "fix_position", "Positions": [4096, 1, 2048, 2048, 4097, 64, 65], "SourceMask": 0b0001},
          {"MixStrategy": "fix_position", "PositionField": "posl", "Number": 300, "SourceMask": 0b0010},
          {"MixStrategy": "random_position", "Number": 64, "SourceMask": 0b0100}]
    rng = np.random.default_rng(4096)
    check(ctx, world, st, 0, True, 4096, make_case(rng, 1, 5000))


def test_a_strategy_that_fills_exactly_on_a_chunk_boundary(ctx, world):
    """the 5th member is list entry 1 023 (the walk ends in chunk 0), resp. 1 024 (it needs chunk 1); later members stay out"""
    rng = np.random.default_rng(1023)
    st = [{"MixStrategy": "fix_position", "Positions": [2, 4, 6, 8, 10], "SourceMask": 0b1000000},
          {"MixStrategy": "random_position", "Number": 3, "SourceMask": 0b1000000}]
    case = make_case(rng, 2, 2049, order=False)
    for q, last in enumerate((1023, 1024)):
        case["source"][q, [5, 77, 500, 1000, last, last + 1, last + 300, 2040]] = 6
    w_out, _ = check(ctx, world, st, 0, False, 12, case)
    assert w_out[0, 9] == 1023 and w_out[1, 9] == 1024
    assert set(w_out[0, :12].tolist()) >= {1024, 1323, 2040}                   # the second strategy took the three behind


def test_fewer_members_than_number_and_no_members(ctx, world):
    rng = np.random.default_rng(5)
    st = [{"MixStrategy": "fix_position", "PositionField": "posi", "Number": 5000, "SourceMask": 0b1000000},
          {"MixStrategy": "random_position", "Number": 20, "SourceMask": 0b10000000},
          {"MixStrategy": "fix_position", "Positions": [1, 2, 3], "SourceMask": 1 << 20}]
    case = make_case(rng, 2, 1500, counts=[1500, 700])
    case["source"][:, ::50] = 6
    case["source"][0, 3::400] = 7
    check(ctx, world, st, 0, True, 20, case)


def test_random_with_step_one_and_with_every_slot_taken_by_fix(ctx, world):
    rng = np.random.default_rng(6)
    S = 40
    step1 = [{"MixStrategy": "random_position", "Number": S, "SourceMask": 0b0111}]
    check(ctx, world, step1, 0, False, S, make_case(rng, 2, 300))
    full = [{"MixStrategy": "fix_position", "Positions": list(range(S, 0, -1)), "SourceMask": 0b0011},
            {"MixStrategy": "random_position", "Number": 5, "SourceMask": 0b1100}]
    w_out, w_cnt = check(ctx, world, full, 0, True, S, make_case(rng, 2, 300, counts=[300, S]))
    assert w_cnt.tolist() == [300, S]


def test_rows_outside_the_store_and_user_slots(ctx, world):
    """every row outside: conditions on item columns fail, a position column reads as missing; a user-only condition still holds"""
    rng = np.random.default_rng(8)
    st = [{"MixStrategy": "fix_position", "PositionField": "posi", "Number": 4, "SourceMask": 0b0001},
          {"MixStrategy": "fix_position", "Positions": [2, 5],
           "Conditions": [{"Name": "age", "Domain": "user", "Operator": "greaterThan", "Type": "int", "Value": 31},
                          {"Name": "cat", "Operator": "is_null"}]}]
    case = make_case(rng, 5, 130)
    case["rows"][0:2] = rng.integers(ROWS, ROWS + OUTSIDE, (2, 130)).astype(np.uint64)
    case["rows"][2] = HUGE
    check(ctx, world, st, 0, False, 9, case)


def test_no_strategies_no_source_no_store(ctx, world):
    rng = np.random.default_rng(9)
    mix = pa.mix_compile([], (), 7, True)
    try:
        case = make_case(rng, 3, 70, counts=[70, 7, 6], source=False)
        w_out, w_cnt = want(world, [], 7, True, 0, case)
        out, cnt = run_dev(ctx, world, mix, 0, case, fs=None)
        assert np.array_equal(out, w_out) and np.array_equal(cnt, w_cnt)
        assert np.array_equal(out[0], case["order"][0])                        # the list, then its tail: the list
    finally:
        mix.free()


def test_one_request_entry_and_two_contexts_sharing_a_set(ctx, world):
    rng = np.random.default_rng(10)
    st = general(10)
    st[1] = dict(st[1], Conditions=st[1]["Conditions"][:1])                    # (a second context has no user arrays at hand)
    mix = pa.mix_compile(st, DECL, 0, True)
    other = pa.Context(0)
    fs2 = pa.Features(other, ROWS)
    try:
        for n, t in DTYPES.items():
            fs2.set_column(n, F_OF[t], world.store[n], default=0.0)
        case = make_case(rng, 1, 333)
        w_out, w_cnt = check(ctx, world, st, 0, True, 10, case, mix=mix)
        out, cnt = ctx.mix_sort_one(mix, world.fs, 10, case["rows"][0], case["source"][0], case["order"][0], int(case["seed"][0]), case["users"][0])
        assert cnt == w_cnt[0] and np.array_equal(out, w_out[0])
        out2, cnt2 = other.mix_sort(mix, fs2, 10, case["rows"], case["source"], case["order"], None, case["seed"], case["users"])
        assert np.array_equal(cnt2, w_cnt) and np.array_equal(out2, w_out)
        out, cnt = ctx.mix_sort_one(mix, world.fs, 10, np.empty(0, np.uint64))  # an empty request: an empty answer
        assert cnt == 0 and out.size == 0
    finally:
        fs2.destroy()
        other.close()
        mix.free()


def test_refusals_leave_the_context_usable(ctx, world):
    rng = np.random.default_rng(11)
    case = make_case(rng, 1, 64)
    mix = pa.mix_compile(general(10), DECL)
    bare = pa.Features(ctx, ROWS)
    try:
        bare.set_column("cat", pa.F_I32, world.store["cat"], default=0.0)
        bare.set_column("flag", pa.F_I64, world.store["flag"], default=0.0)
        bare.set_column("w", pa.F_F32, world.store["w"], default=0.0)
        with pytest.raises(PgError) as e:
            run_dev(ctx, world, mix, 10, case, fs=bare)
        assert e.value.code == -1 and "\"posi\"" in str(e.value) and "feature store" in str(e.value)
        with pytest.raises(PgError) as e:
            run_dev(ctx, world, mix, 10, dict(case, source=None))
        assert e.value.code == -1 and "source" in str(e.value)
        with pytest.raises(PgError) as e:
            run_dev(ctx, world, mix, 1, case)                                  # RANDOM Number 2 on a page of one slot
        assert e.value.code == -1 and "number 2" in str(e.value)
        with pytest.raises(PgError) as e:
            run_dev(ctx, world, mix, 4097, case)
        assert e.value.code == -4 and "4097" in str(e.value)
        check(ctx, world, general(10), 0, False, 10, case, mix=mix)
    finally:
        bare.destroy()
        mix.free()


# ---- the host mirror: SortType "MultiRecallMixSort" in pairec_gpu.Sorts -------------------------------------------------------------
import json                 # noqa: E402

import test_mixsort_cpu as cpu      # noqa: E402  (the mirror's config, the golden cases, the library loader)


class Eng:
    pass


@pytest.fixture(scope="module")
def eng():
    e = Eng()
    e.H = cpu.mirror_lib()
    e.h = e.H.ph_engine_create(json.dumps(cpu.MIRROR_CONFIG).encode())
    assert e.h, e.H.ph_last_error()
    user = cpu.o.synth_rows(cpu.o.SEED_QUERY, 3, 1, 128)[0]
    e.H.ph_set_user_vector(e.h, b"u1", " ".join("%d:%s" % (i + 1, repr(float(v))) for i, v in enumerate(user)).encode())
    yield e
    e.H.ph_engine_destroy(e.h)


def mirror_sort(e, name, items, size):
    r = e.H.ph_engine_sort_scored(e.h, name.encode(), json.dumps(items).encode(), b"{}", size)
    return None if r is None else [x["item_id"] for x in json.loads(r)["items"]]


def golden_items(case):
    """the case's items as ItemRankScore leaves them: by score, descending"""
    it = case["items"]
    inv = {v: k for k, v in cpu.GOLDEN["strings"].items() if k in ("man", "woman")}
    items = [{"id": str(i), "score": it["score"][i], "retrieve_id": case["recall_names"][it["source"][i]],
              "properties": {k: inv[v[i]] for k, v in it.get("columns", {}).items() if k == "sex"}} for i in range(len(it["source"]))]
    return sorted(items, key=lambda x: -x["score"])


def test_mirror_fix_config_gives_the_ref_page_and_skips_unknown_strategies(eng):
    case = next(c for c in cpu.GOLDEN["cases"] if c["name"] == "fix_position_by_recall_name")
    items = golden_items(case)
    member = [[x["retrieve_id"] == "r1" for x in items]]
    for size in case["sizes"]:
        want = [items[j]["id"] for j in ref.mix_list(case["config"]["MixSortRules"], size, len(items), member, [None])]
        assert mirror_sort(eng, "fix_r1", items, size) == want and len(want) == size
        assert [want[p - 1] for p in (1, 4, 6, 8, 10)] == ["9", "8", "7", "6", "5"]
        assert mirror_sort(eng, "skips_unknown", items, size) == want
    assert mirror_sort(eng, "fix_r1", [], 10) == []
    many = [{"id": str(i), "score": 1.0, "retrieve_id": "r1"} for i in range(16385)]
    assert mirror_sort(eng, "fix_r1", many, 10) is None and b"MultiRecallMixSort" in eng.H.ph_last_error() and b"16385 items" in eng.H.ph_last_error()


def test_mirror_random_config_holds_the_golden_properties_and_counts_its_calls(eng):
    """RemainItem: the length is the item count; no empty slot; the seed is Seed + the calls this sort has served before"""
    case = next(c for c in cpu.GOLDEN["cases"] if c["name"] == "random_position_by_condition")
    items = golden_items(case)
    rules = [r for s in cpu.MIRROR_SORTS if s["Name"] == "random_man" for r in s["MixSortRules"]]
    member = [[x["properties"]["sex"] == "man" for x in items]]
    for call, size in enumerate((10, 12, 15, 20)):
        got = mirror_sort(eng, "random_man", items, size)
        S = max(size, 12)
        want = [items[j]["id"] for j in ref.mix_list(rules, S, len(items), member, [None], seed=77 + call, remain=True)]
        assert got == want and len(got) == len(items) and len(set(got)) == len(items)
    lacking = [dict(x, properties={}) if x["id"] == "3" else x for x in items]
    assert mirror_sort(eng, "random_man", lacking, 10) is None
    assert b"MultiRecallMixSort" in eng.H.ph_last_error() and b'"sex"' in eng.H.ph_last_error() and b"item 3" in eng.H.ph_last_error()


def test_mirror_scene_with_the_sort_behind_item_rank_score(eng):
    base = [x["item_id"] for x in json.loads(eng.H.ph_recommend(eng.h, b"u1", 300, b"plain"))["items"]]
    assert len(base) == 300
    r = eng.H.ph_recommend(eng.h, b"u1", 40, b"mixed")
    assert r, eng.H.ph_last_error()
    got = [x["item_id"] for x in json.loads(r)["items"]]
    rules = [r for s in cpu.MIRROR_SORTS if s["Name"] == "page_mix" for r in s["MixSortRules"]]
    # every item is the recall's; no item carries a "slot" property: the second strategy takes three and places none
    want = ref.mix_list(rules, 40, 300, [[True] * 300, [True] * 300], [None, [-1] * 300])
    assert got == [base[j] for j in want] and got[:5] == [base[6], base[0], base[7], base[2], base[8]]
