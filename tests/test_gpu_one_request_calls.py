"""GPU tests of the five one-request calls on host arrays — pg_item_state_filter, pg_boost_scores, pg_candidates_classcut,
pg_mix_sort, pg_diversity_rules — each held against its batched device entry at nq = 1, by bits: they share the kernels, so all
that can differ is the staging (what is uploaded where, what comes back, how much).  n sits around a wave of 64 lanes and past
one workgroup's first pass (1, 63, 64, 65, 257), with and without `source`; n = 0 answers without touching an output.  The C
entries are called directly, on host outputs that lie between two 64-byte guard regions.  A last test frees two compiled sets of
each kind in the opposite order from their creation, each after a launch nobody waited for, and uses the context again."""
import ctypes as C

import numpy as np
import pytest

import pairec_amd as pa
from pairec_amd import _lib
from pairec_amd.engine import _div_config

pytestmark = pytest.mark.gpu

S = 300                                           # store rows; candidates' rows reach past them
SIZES = [1, 63, 64, 65, 257]
GUARD = 64
DECL = [("cat", pa.F_I32), ("big", pa.F_I64), ("w", pa.F_F32), ("x", pa.F_F64)]
NP_OF = {pa.F_I32: np.int32, pa.F_I64: np.int64, pa.F_F32: np.float32, pa.F_F64: np.float64}
USER = {"age": 31, "lim": 0.25}
FILTER = [{"Conditions": [{"Name": "cat", "Operator": "less", "Type": "int", "Value": 4},
                          {"Name": "w", "Operator": "greater", "Type": "float", "Value": "user.lim"},
                          {"Name": "age", "Domain": "user", "Operator": "greater", "Type": "int", "Value": "item.cat"}]}]
BOOST = [{"Conditions": [{"Name": "cat", "Operator": "less", "Type": "int", "Value": 3}], "Expression": "score * 2 + x"},
         {"Conditions": [{"Name": "big", "Operator": "greater", "Type": "int64", "Value": 1 << 33}], "Expression": "score - w"},
         {"Conditions": [{"Name": "lim", "Domain": "user", "Operator": "is_not_null"}], "Expression": "round(score, 1) + cat"}]
MIX = [{"MixStrategy": "fix_position", "Positions": [2, 5, 1], "SourceMask": 0b010,
        "Conditions": [{"Name": "cat", "Operator": "equal", "Type": "int", "Value": 2}]},
       {"MixStrategy": "random_position", "Number": 3, "Conditions": [{"Name": "age", "Domain": "user", "Operator": "greater", "Type": "int", "Value": 30}]}]
DIV = {"size": 40, "rules": [{"dims": [0], "interval": 1, "weight": 2}, {"dims": [1, 0], "window": 3, "frequency": 1, "weight": 1}],
       "exclude_source_mask": 0b100}


class Guarded:
    """a host output of `count` elements between two guard regions"""

    def __init__(self, dtype, count):
        self.n = count * np.dtype(dtype).itemsize
        self.raw = np.full(GUARD + self.n + GUARD, 0xA5, np.uint8)
        self.ptr = self.raw.ctypes.data + GUARD
        self.value = self.raw[GUARD:GUARD + self.n].view(dtype)

    def untouched(self):
        return bool(np.all(self.raw[:GUARD] == 0xA5) and np.all(self.raw[GUARD + self.n:] == 0xA5))

    def blank(self):
        return bool(np.all(self.raw == 0xA5))


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def same(one, batched):
    assert one.untouched(), "a write outside a host output"
    assert np.array_equal(bits(one.value), bits(batched)), "the one-request call and the batched entry differ"


class World:
    pass


@pytest.fixture(scope="module")
def world(ctx):
    w = World()
    rng = np.random.default_rng(5150)
    w.L = _lib.load()
    w.store = {"cat": rng.integers(0, 6, S).astype(np.int32), "big": rng.integers(0, 4, S).astype(np.int64) << 32,
               "w": (rng.integers(-4, 5, S) * 0.125).astype(np.float32), "x": rng.integers(-8, 9, S) * 0.5}
    w.fs = pa.Features(ctx, S)
    for name, dt in DECL:
        w.fs.set_column(name, dt, w.store[name])
    w.filt = pa.Cond(FILTER, DECL)
    w.boost = pa.Cond(BOOST, DECL, boost=True)
    w.mix = pa.Mix(MIX, DECL, size=12, remain_item=True)
    w.mix_no_source = pa.Mix([{k: v for k, v in st.items() if k != "SourceMask"} for st in MIX], DECL, size=12, remain_item=True)
    yield w
    for o in (w.filt, w.boost, w.mix, w.mix_no_source):
        o.free()
    w.fs.destroy()


def request(n, seed):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, S + S // 10, n).astype(np.uint64)
    rows[rng.random(n) < 0.05] = np.uint64(0xFFFFFFFFFFFFFFFF)                      # padding anywhere
    score = rng.integers(0, 6, n).astype(np.float64)
    score[rng.random(n) < 0.05] = np.nan
    return rows, score, rng.integers(0, 4, n).astype(np.uint8)


def opt(a):
    return None if a is None else a.ctypes.data


@pytest.mark.parametrize("with_source", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_item_state_filter(ctx, world, n, with_source):
    rows, score, source = request(n, 10 + n)
    source = source if with_source else None
    uv, up = world.filt.pack_user([USER])
    o_r, o_s, o_src, o_n = Guarded(np.uint64, n), Guarded(np.float64, n), Guarded(np.uint8, n), Guarded(np.uint32, 1)
    _lib.check(world.L.pg_item_state_filter(ctx.h, world.filt.h, world.fs.h, n, rows.ctypes.data, score.ctypes.data, opt(source), uv.ctypes.data,
                                            int(up[0]), o_r.ptr, o_s.ptr, o_src.ptr if with_source else None, o_n.ptr))
    b = ctx.item_state_filter(world.filt, world.fs, rows[None], score[None], None if source is None else source[None], users=[USER])
    same(o_r, b[0])
    same(o_s, b[1])
    same(o_n, b[6])
    assert 0 < int(b[6][0]) < n or n < 63
    if with_source:
        same(o_src, b[2])
    else:
        assert o_src.blank()


@pytest.mark.parametrize("with_rule", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_boost_scores(ctx, world, n, with_rule):
    """(this call takes no source: the optional output is the rule ids)"""
    rows, score, _ = request(n, 20 + n)
    rows = np.minimum(rows, np.uint64(S + 5))                # (no padding: the one-request call knows candidates in and outside the store only)
    inside = rows < S
    idx = np.where(inside, rows, 0).astype(np.int64)
    cols = [np.ascontiguousarray(world.store[name][idx]).astype(NP_OF[dt]) for name, dt in DECL]
    ptrs = (C.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
    item_in = inside.astype(np.uint8)
    uv, up = world.boost.pack_user([USER])
    o_s, o_rule = Guarded(np.float64, n), Guarded(np.uint8, n)
    _lib.check(world.L.pg_boost_scores(ctx.h, world.boost.h, 0, n, item_in.ctypes.data, ptrs, uv.ctypes.data, int(up[0]), score.ctypes.data,
                                       o_s.ptr, o_rule.ptr if with_rule else None))
    b_s, b_rule = ctx.boost_scores(world.boost, world.fs, rows[None], score[None], users=[USER])
    same(o_s, b_s)
    if with_rule:
        same(o_rule, b_rule)
    else:
        assert o_rule.blank()


@pytest.mark.parametrize("width", ["one", "n", "some"])
@pytest.mark.parametrize("with_source", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_candidates_classcut(ctx, world, n, with_source, width):
    """width: the rule set's out_cap is 1, n, or in between"""
    rows, score, source = request(n, 30 + n)
    source = source if with_source else None
    name = "recall_name == 'b' || " if with_source else ""
    rules = {"one": [(name + "cat < 3", pa.TRIM_FIX, 1)], "n": [("cat < 3", pa.TRIM_FIX, n), (name + "recall_score >= 2", pa.TRIM_ACCUMULATE, n)],
             "some": [(name + "cat < 3", pa.TRIM_FIX, (n + 3) // 4), ("w > 0", pa.TRIM_ACCUMULATE, (n + 2) // 3)]}[width]
    cc = pa.Classcut(rules, DECL, ["a", "b", "c"])
    w = cc.out_cap(n)
    assert w == {"one": 1, "n": n}.get(width, w)
    o_r, o_s, o_src, o_n = Guarded(np.uint64, w), Guarded(np.float64, w), Guarded(np.uint8, w), Guarded(np.uint32, 1)
    _lib.check(world.L.pg_candidates_classcut(ctx.h, cc.h, world.fs.h, n, rows.ctypes.data, score.ctypes.data, opt(source), o_r.ptr, o_s.ptr,
                                              o_src.ptr if with_source else None, o_n.ptr))
    b = ctx.candidates_classcut(cc, world.fs, rows[None], score[None], None if source is None else source[None])
    cc.free()
    same(o_r, b[0])
    same(o_s, b[1])
    same(o_n, b[6])
    if with_source:
        same(o_src, b[2])
    else:
        assert o_src.blank()


@pytest.mark.parametrize("with_order", [True, False])
@pytest.mark.parametrize("with_source", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_mix_sort(ctx, world, n, with_source, with_order):
    rows, _, source = request(n, 40 + n)
    source = source if with_source else None
    mix = world.mix if with_source else world.mix_no_source           # (a strategy with a source mask needs `source`)
    order = np.random.default_rng(n).permutation(n).astype(np.uint32) if with_order else None
    seed = 0x9E3779B97F4A7C15 + n
    uv, up = mix.pack_user([USER])
    o_o, o_n = Guarded(np.uint32, n), Guarded(np.uint32, 1)
    _lib.check(world.L.pg_mix_sort(ctx.h, mix.h, world.fs.h, 0, n, rows.ctypes.data, opt(source), opt(order), seed, uv.ctypes.data, int(up[0]),
                                   o_o.ptr, C.cast(o_n.ptr, C.POINTER(C.c_uint32))))
    b_o, b_n = ctx.mix_sort(mix, world.fs, 0, rows[None], None if source is None else source[None], None if order is None else order[None],
                            seed=np.array([seed], np.uint64), users=[USER])
    same(o_o, b_o)
    same(o_n, b_n)


@pytest.mark.parametrize("with_source", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_diversity_rules(ctx, world, n, with_source):
    rng = np.random.default_rng(50 + n)
    dims = rng.integers(0, 4, (2, n)).astype(np.int64)
    source = rng.integers(0, 4, n).astype(np.uint8) if with_source else None
    cfg = DIV if with_source else {k: v for k, v in DIV.items() if k != "exclude_source_mask"}
    c, keep = _div_config(cfg, 2)
    o = Guarded(np.uint32, n)
    _lib.check(world.L.pg_diversity_rules(ctx.h, C.byref(c), n, dims.ctypes.data, opt(source), o.ptr))
    del keep
    same(o, ctx.diversity_rules(cfg, dims[:, None, :], source=None if source is None else source[None]))
    assert sorted(o.value.tolist()) == list(range(n))


def test_an_empty_request_touches_no_output(ctx, world):
    """n = 0: every call answers OK, writes a count of 0 where it has one and nothing else"""
    L, e = world.L, np.zeros(1, np.uint64)
    out, out2, src, cnt = Guarded(np.uint64, 4), Guarded(np.float64, 4), Guarded(np.uint8, 4), Guarded(np.uint32, 1)
    uv, up = world.filt.pack_user([USER])
    _lib.check(L.pg_item_state_filter(ctx.h, world.filt.h, world.fs.h, 0, e.ctypes.data, e.ctypes.data, e.ctypes.data, uv.ctypes.data, int(up[0]),
                                      out.ptr, out2.ptr, src.ptr, cnt.ptr))
    assert cnt.value[0] == 0 and cnt.untouched() and out.blank() and out2.blank() and src.blank()
    cc = pa.Classcut([("cat < 3", pa.TRIM_FIX, 2)], DECL)
    cnt = Guarded(np.uint32, 1)
    _lib.check(L.pg_candidates_classcut(ctx.h, cc.h, world.fs.h, 0, e.ctypes.data, e.ctypes.data, e.ctypes.data, out.ptr, out2.ptr, src.ptr, cnt.ptr))
    cc.free()
    assert cnt.value[0] == 0 and cnt.untouched() and out.blank() and out2.blank() and src.blank()
    uv, up = world.mix.pack_user([USER])
    cnt = Guarded(np.uint32, 1)
    _lib.check(L.pg_mix_sort(ctx.h, world.mix.h, world.fs.h, 0, 0, e.ctypes.data, e.ctypes.data, e.ctypes.data, 7, uv.ctypes.data, int(up[0]), out.ptr,
                             C.cast(cnt.ptr, C.POINTER(C.c_uint32))))
    assert cnt.value[0] == 0 and cnt.untouched() and out.blank()
    uv, up = world.boost.pack_user([USER])
    ptrs = (C.c_void_p * len(DECL))(*[e.ctypes.data] * len(DECL))
    _lib.check(L.pg_boost_scores(ctx.h, world.boost.h, 0, 0, e.ctypes.data, ptrs, uv.ctypes.data, int(up[0]), e.ctypes.data, out2.ptr, src.ptr))
    assert out2.blank() and src.blank()
    c, keep = _div_config(DIV, 2)
    _lib.check(L.pg_diversity_rules(ctx.h, C.byref(c), 0, e.ctypes.data, e.ctypes.data, out.ptr))
    del keep
    assert out.blank()
    # a classcut whose every count is 0 keeps nothing of a request that is not empty either
    rows, score, source = request(65, 3)
    cc = pa.Classcut([("cat < 3", pa.TRIM_FIX, 0)], DECL)
    cnt = Guarded(np.uint32, 1)
    _lib.check(L.pg_candidates_classcut(ctx.h, cc.h, world.fs.h, 65, rows.ctypes.data, score.ctypes.data, source.ctypes.data, out.ptr, out2.ptr, src.ptr,
                                        cnt.ptr))
    cc.free()
    assert cnt.value[0] == 0 and cnt.untouched() and out.blank() and out2.blank() and src.blank()


def test_compiled_sets_freed_in_reverse_after_unsynchronised_launches(ctx, world):
    """two sets of each kind, each launched once without a synchronize, freed last-made first: the free waits for the launch that
    may still read the set's table, and the context serves afterwards"""
    nq, cap = 2, 65
    rng = np.random.default_rng(8)
    rows = rng.integers(0, S, (nq, cap)).astype(np.uint64)
    score = rng.integers(0, 6, (nq, cap)).astype(np.float64)
    d = [ctx.to_device(rows), ctx.to_device(score)] + [ctx.malloc(nq * cap * 8) for _ in range(3)]
    d_rows, d_score, d_o1, d_o2, d_o3 = d
    made = []
    try:
        for k in range(2):
            c = pa.Cond([{"Conditions": [{"Name": "cat", "Operator": "in", "Type": "int", "Value": [k, k + 2, 5]}]}], DECL)
            made.append(c)
            ctx.item_state_filter_dev(c, world.fs, nq, cap, d_rows, d_score, 0, 0, 0, 0, 0, 0, 0, 0, 0, d_o1, d_o2, 0, 0, 0, 0, d_o3)
            cc = pa.Classcut([("cat in (%d, 4) || w > 0" % k, pa.TRIM_FIX, 7 + k)], DECL)
            made.append(cc)
            ctx.candidates_classcut_dev(cc, world.fs, nq, cap, d_rows, d_score, 0, 0, 0, 0, 0, 0, 0, d_o1, d_o2, 0, 0, 0, 0, d_o3)
            m = pa.Mix([{"MixStrategy": "fix_position", "Positions": [1 + k, 4], "Conditions": [{"Name": "cat", "Operator": "equal", "Type": "int", "Value": k}]}],
                       DECL, size=8)
            made.append(m)
            ctx.mix_sort_dev(m, world.fs, 0, nq, cap, d_rows, 0, 0, 0, 0, 0, 0, d_o1, d_o3)
        for o in reversed(made):
            o.free()
        made = []
        ctx.synchronize()
        uv_rows, uv_score, _ = request(64, 9)
        got = ctx.item_state_filter_one(world.filt, world.fs, uv_rows, uv_score, user=USER)
        want = ctx.item_state_filter(world.filt, world.fs, uv_rows[None], uv_score[None], users=[USER])
        assert got[3] == int(want[6][0]) and np.array_equal(got[0], want[0][0])
    finally:
        for o in made:
            o.free()
        for p in d:
            ctx.free(p)
