"""GPU tests of ItemStateFilter and BoostScoreSort on the device (csrc/cond.hip: pg_item_state_filter_dev,
pg_boost_scores_dev and the one-request entries) against tests/cond_ref.py: rows, counts, sources, planes and rule ids exactly,
scores as bit patterns (ref.score_bits folds the sign of the default NaN an invalid operation generates, nothing else).  The reference is
computed once over the store's rows — a candidate's answer depends on its row and its request's user properties only — and shared
by all tests.  Sizes sit on the kernels' edges: a wave of 64 lanes, the filter's chunk of 1 024 positions, the boost kernel's
workgroup of 256, the largest cap of 16 384.  Every output buffer carries a guard word behind it."""
import math

import numpy as np
import pytest

import cond_ref as ref
import fanin_ref
import pairec_amd as pa
import trim_ref
from pairec_amd._lib import PgError

pytestmark = pytest.mark.gpu

U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
S, A, J = 2000, 250, 47                       # store rows; rows [0, A) pass whatever the user, [A, 2A) fail; J rows just outside
HUGE = np.uint64((1 << 40) + 5)               # a row far outside
LIST64 = [3 * k for k in range(60)] + [(1 << 31) + 9, (1 << 40) + 3, -(1 << 35), 1 << 62]
BAD_ID = 3
USERS = [{"uf": 2.0, "ui": 7}, {"ui": 7}, {"uf": 2.0}, {}]
DTYPES = {"c0": np.int32, "c1": np.int64, "c2": np.float32, "c3": np.float64, "c4": np.int64, "c5": np.int32, "c6": np.int64, "c7": np.int32,
          "c8": np.int32, "c9": np.int32, "c10": np.float32, "c11": np.float64, "c12": np.int32, "c13": np.int64, "c14": np.float32,
          "c15": np.int32}
F_OF = {np.int32: pa.F_I32, np.int64: pa.F_I64, np.float32: pa.F_F32, np.float64: pa.F_F64}
DECL = [(n, F_OF[t]) for n, t in DTYPES.items()]

FILTER_RULES = [
    {"Conditions": [
        {"Name": "c0", "Operator": "greaterThan", "Type": "int", "Value": "item.c1"},
        {"Name": "c2", "Domain": "item", "Operator": "less", "Type": "float", "Value": "item.c3"},
        {"Name": "c4", "Operator": "in", "Type": "int", "Value": LIST64},
        {"Name": "c5", "Operator": "not_in", "Type": "string", "Value": [BAD_ID]},
        {"Operator": "bool", "Type": "or", "Configs": [
            {"Name": "c6", "Operator": "equal", "Type": "int64", "Value": "item.c7"},
            {"Name": "c8", "Operator": "lessThan", "Type": "float", "Value": "user.uf"}]},
        {"Name": "ui", "Domain": "user", "Operator": "not_equal", "Type": "int", "Value": "item.c9"}]},
    # (the kernel evaluates rule 0; rule 1 brings the set to 16 referenced columns, all of which every lane loads)
    {"Conditions": [
        {"Name": "c10", "Operator": "greater", "Type": "float", "Value": 0.0},
        {"Name": "c11", "Operator": "less", "Type": "float", "Value": 5.0},
        {"Name": "c12", "Operator": "equal", "Type": "int", "Value": 1},
        {"Name": "c13", "Operator": "not_equal", "Type": "int64", "Value": 0},
        {"Name": "c14", "Operator": "lessThan", "Type": "float", "Value": "item.c11"},
        {"Name": "c15", "Operator": "in", "Type": "int", "Value": [2]}]},
]
BOOST_RULES = [
    {"Conditions": [], "Expression": "score * 2 + c12"},
    {"Conditions": [{"Name": "c0", "Operator": "greaterThan", "Type": "int", "Value": "item.c1"}], "Expression": "score - c10 / 4"},
    {"Conditions": [{"Name": "c4", "Operator": "in", "Type": "int", "Value": LIST64}], "Expression": "round(score * c11, 2)"},
    {"Conditions": [{"Name": "uf", "Domain": "user", "Operator": "is_not_null"}], "Expression": "score % 7 + c14"},
    {"Conditions": [{"Name": "c5", "Operator": "not_in", "Type": "string", "Value": [BAD_ID]}], "Expression": "-score ** 2"},
    {"Conditions": [{"Operator": "bool", "Type": "and", "Configs": [
        {"Name": "c2", "Operator": "less", "Type": "float", "Value": "item.c3"},
        {"Name": "c13", "Operator": "greater", "Type": "int64", "Value": (1 << 31) + 1},
        {"Name": "c6", "Operator": "equal", "Type": "int64", "Value": "item.c7"}]}], "Expression": "(score + [c15]) * 0.5"},
    {"Conditions": [{"Name": "c8", "Operator": "lessThan", "Type": "float", "Value": "user.uf"}], "Expression": "score / c9"},
    {"Conditions": [{"Name": "ui", "Domain": "user", "Operator": "not_equal", "Type": "int", "Value": "item.c9"}], "Expression": "round(score) + 1"},
]


def _store(rng):
    c = {}
    c["c1"] = rng.integers(0, 4, S)
    c["c0"] = c["c1"] + rng.integers(0, 3, S)
    c["c2"] = rng.integers(-8, 8, S) * 0.25
    c["c3"] = c["c2"] + 1.0
    c["c4"] = rng.choice(LIST64, S)
    c["c5"] = rng.choice([0, 1, 2, 4, 5], S)
    c["c7"] = rng.integers(0, 50, S)
    c["c6"] = c["c7"].copy()
    c["c8"] = rng.integers(0, 3, S)
    c["c9"] = rng.integers(1, 4, S)
    c["c10"] = rng.integers(1, 9, S) * 0.5
    c["c11"] = rng.integers(1, 17, S) * 0.25
    c["c12"] = rng.integers(0, 3, S)
    c["c13"] = rng.integers(2, 9, S) * (1 << 31)
    c["c14"] = rng.integers(-4, 5, S) * 0.125
    c["c15"] = rng.integers(0, 4, S)
    # rows [A, 2A) fail rule 0 on its first term; the rows behind them fail a random term, or none
    c["c0"][A:2 * A] = c["c1"][A:2 * A] - 1
    for r in range(2 * A, S):
        k = rng.integers(0, 12)
        if k == 0:
            c["c0"][r] = c["c1"][r] - 1
        elif k == 1:
            c["c3"][r] = c["c2"][r]
        elif k == 2:
            c["c4"][r] += 1
        elif k == 3:
            c["c5"][r] = BAD_ID
        elif k == 4:
            c["c6"][r] += 1
            c["c8"][r] = 5
        elif k == 5:
            c["c6"][r] += 1
        elif k == 6:
            c["c9"][r] = 7
        elif k == 7:
            c["c13"][r] = 5
        elif k == 8:
            c["c9"][r] = 0
    return {n: np.ascontiguousarray(c[n]).astype(t) for n, t in DTYPES.items()}


class World:
    pass


@pytest.fixture(scope="module")
def world(ctx):
    w = World()
    rng = np.random.default_rng(4116)
    w.store = _store(rng)
    w.fs = pa.Features(ctx, S)
    for n, t in DTYPES.items():
        w.fs.set_column(n, F_OF[t], w.store[n], default=1.0)           # (a default the filter must never read)
    w.filter = pa.cond_compile(FILTER_RULES, DECL)
    w.boost = pa.cond_compile(BOOST_RULES, DECL, boost=True)
    # the universe: every store row, J rows just outside, one far outside; its index in the tables
    w.universe = np.concatenate([np.arange(S + J, dtype=np.uint64), [HUGE]])
    w.score_of = np.round(rng.standard_normal(w.universe.size) * 4, 3)
    w.score_of[::97] = 0.0
    cols, inside = ref.gather(w.store, S, w.universe)
    w.keep = [np.array([ref.match(FILTER_RULES[0]["Conditions"], i, cols, inside, u) for i in range(w.universe.size)]) for u in USERS]
    w.boosted = {}
    for v in (0, 1):
        for fa in (False, True):
            s, r = ref.boost(BOOST_RULES, fa, w.score_of, cols, inside, USERS[v])
            w.boosted[v, fa] = (s, r)
    # the host statements agree with the tables (the CPU tests hold them against cond_ref on random cases; this is this config)
    for v, u in enumerate(USERS):
        assert np.array_equal(w.filter.match_host(cols, inside, u), w.keep[v])
    for (v, fa), (s, r) in w.boosted.items():
        hs, hr = w.boost.boost_host(w.score_of, cols, inside, USERS[v], fa)
        assert np.array_equal(ref.score_bits(hs), ref.score_bits(s)) and np.array_equal(hr, r)
    assert all(k[:A].all() and not k[A:2 * A].any() and not k[S:].any() for k in w.keep)
    assert 0.2 < w.keep[0][2 * A:S].mean() < 0.8
    yield w
    w.filter.free()
    w.boost.free()
    w.fs.destroy()


def index_of(rows):
    """universe index of candidate rows (padding → 0, never looked at)"""
    r = np.asarray(rows, dtype=np.uint64)
    return np.where(r == HUGE, S + J, np.where(r == U64MAX, 0, r)).astype(np.int64)


def request_rows(rng, cap, flavour):
    """one request's rows and count: mixed (a third outside the store, padding in the middle, count short of cap), all kept, none
    kept, nothing (count 0)"""
    if flavour == "all":
        return rng.integers(0, A, cap).astype(np.uint64), cap
    if flavour == "none":
        return rng.integers(A, 2 * A, cap).astype(np.uint64), cap
    rows = rng.integers(0, S, cap).astype(np.uint64)
    out = rng.random(cap) < 1 / 3
    rows[out] = rng.integers(S, S + J, cap).astype(np.uint64)[out]
    rows[rng.random(cap) < 0.02] = HUGE
    rows[rng.random(cap) < 0.05] = U64MAX
    if flavour == "nothing":
        return rows, 0
    return rows, (cap if flavour == "mixed_full" else max(1, cap - cap // 7))


def make_case(rng, nq, cap, flavours, n64, n32, optional=True):
    rows, count = np.empty((nq, cap), np.uint64), np.empty(nq, np.uint32)
    for q in range(nq):
        rows[q], count[q] = request_rows(rng, cap, flavours[q % len(flavours)])
    score = np.round(rng.standard_normal((nq, cap)), 4)
    score.view(np.uint64)[0, cap // 2] = 0x7FF8000000000123              # a NaN with a payload travels as bits
    if not optional:
        return rows, score, None, count, None, None, None
    return (rows, score, rng.integers(0, 8, (nq, cap)).astype(np.uint8), count, rng.standard_normal((n64, nq, cap)),
            rng.integers(0, 256, (nq, cap)).astype(np.uint32), rng.standard_normal((n32, nq, cap)).astype(np.float32))


GUARD = 256


class Guarded:
    """device buffers with a guard behind every one: outputs are pre-filled, so an element the kernel skips shows as well"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def put(self, a):
        if a is None:
            return 0
        p = self.ctx.to_device(np.ascontiguousarray(a))
        self.bufs.append((p, None, 0))
        return p

    def out(self, a):
        if a is None:
            return 0
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


def run_filter(ctx, w, case, users, cond=None):
    rows, score, source, count, p64, mask, p32 = case
    nq, cap = rows.shape
    cond = cond or w.filter
    uv, up = cond.pack_user(users)
    outs = [np.empty((nq, cap), np.uint64), np.empty((nq, cap), np.float64), None if source is None else np.empty((nq, cap), np.uint8),
            None if p64 is None else np.empty(p64.shape, np.float64), None if mask is None else np.empty((nq, cap), np.uint32),
            None if p32 is None else np.empty(p32.shape, np.float32), np.empty(nq, np.uint32)]
    g = Guarded(ctx)
    try:
        d_in = [g.put(a) for a in (rows, score, source, count, p64, mask, p32, uv, up)]
        d_out = [g.out(a) for a in outs]
        ctx.item_state_filter_dev(cond, w.fs, nq, cap, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], 0 if p64 is None else p64.shape[0], d_in[5],
                                  d_in[6], 0 if p32 is None else p32.shape[0], d_in[7], d_in[8], *d_out)
        g.fetch()
    finally:
        g.free()
    return tuple(outs)


def want_filter(w, case, variants):
    rows, score, source, count, p64, mask, p32 = case
    idx = index_of(rows)
    keep = np.stack([w.keep[v][idx[q]] for q, v in enumerate(variants)])
    return ref.item_state_filter(None, None, S, rows, score, source, count, p64, mask, p32, keep=keep)


def run_boost(ctx, w, rows, score, count, users, filter_all, want_rule=True):
    nq, cap = rows.shape
    uv, up = w.boost.pack_user(users)
    out, rule = np.empty((nq, cap), np.float64), (np.empty((nq, cap), np.uint8) if want_rule else None)
    g = Guarded(ctx)
    try:
        d = [g.put(a) for a in (rows, score, count, uv, up)]
        ctx.boost_scores_dev(w.boost, w.fs, filter_all, nq, cap, d[0], d[1], d[2], d[3], d[4], g.out(out), g.out(rule))
        g.fetch()
    finally:
        g.free()
    return out, rule


def want_boost(w, rows, score, count, variants, filter_all):
    """scores here are the universe's score of the row, so the tables hold the answers; padding keeps its bits and gets 0xFF"""
    nq, cap = rows.shape
    idx = index_of(rows)
    out, rule = score.copy(), np.full((nq, cap), 0xFF, np.uint8)
    for q, v in enumerate(variants):
        s, r = w.boosted[v, filter_all]
        live = (np.arange(cap) < (cap if count is None else count[q])) & (rows[q] != U64MAX)
        out[q, live], rule[q, live] = s[idx[q, live]], r[idx[q, live]]
    return out, rule


def boost_case(w, rng, nq, cap, flavours):
    rows, count = np.empty((nq, cap), np.uint64), np.empty(nq, np.uint32)
    for q in range(nq):
        rows[q], count[q] = request_rows(rng, cap, flavours[q % len(flavours)])
    score = w.score_of[index_of(rows)].copy()
    pad = rows == U64MAX
    score[pad] = rng.standard_normal(int(pad.sum()))                        # padding: any bits, kept
    if pad.any():
        score.view(np.uint64)[tuple(np.argwhere(pad)[0])] = 0x7FF8000000000123
    return rows, score, count


CAPS = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 16384)


# ---- the filter -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", CAPS)
def test_filter_sizes(ctx, world, cap):
    rng = np.random.default_rng(cap)
    flavours = ("mixed", "all", "none" if cap % 2 else "nothing")
    case = make_case(rng, 3, cap, flavours, n64=1 + cap % 8, n32=1 + cap % 3)
    got = run_filter(ctx, world, case, [USERS[0]] * 3)
    want = want_filter(world, case, [0, 0, 0])
    trim_ref.same(got, want)
    assert got[6][1] == cap and got[6][2] == 0
    if cap in (65, 1025):                                                  # every optional array absent
        bare = (case[0], case[1], None, case[3], None, None, None)
        trim_ref.same(run_filter(ctx, world, bare, [USERS[0]] * 3), want_filter(world, bare, [0, 0, 0]))
        full = (case[0], case[1], case[2], None, case[4], case[5], case[6])     # no counts: cap entries each
        trim_ref.same(run_filter(ctx, world, full, [USERS[0]] * 3), want_filter(world, full, [0, 0, 0]))


@pytest.mark.parametrize("cap", (65, 1025))
def test_filter_optional_arrays_one_at_a_time(ctx, world, cap):
    """every optional array absent, then each present alone, at one lane past a wave and one position past a chunk: what binds the
    ABI's pointers decides per array what the kernel carries and pads"""
    rng = np.random.default_rng(7000 + cap)
    rows, score, source, count, p64, mask, p32 = make_case(rng, 3, cap, ("mixed", "all", "none"), n64=2, n32=3)
    users = [USERS[0]] * 3
    for case in ((rows, score, None, None, None, None, None), (rows, score, source, None, None, None, None),
                 (rows, score, None, count, None, None, None), (rows, score, None, None, p64, None, None),
                 (rows, score, None, None, None, mask, None), (rows, score, None, None, None, None, p32)):
        got = run_filter(ctx, world, case, users)
        trim_ref.same(got, want_filter(world, case, [0, 0, 0]))
        assert 0 < got[6][0] < cap and got[6][1] == cap and got[6][2] == 0


def test_filter_256_requests_users_and_flavours(ctx, world):
    rng = np.random.default_rng(256)
    nq, cap = 256, 65
    flavours = ("mixed", "all", "none", "nothing", "mixed_full")
    case = make_case(rng, nq, cap, flavours, n64=8, n32=8)
    variants = [q % 4 for q in range(nq)]                                  # a request with a user slot absent, with both, with none
    got = run_filter(ctx, world, case, [USERS[v] for v in variants])
    trim_ref.same(got, want_filter(world, case, variants))
    kept = got[6].astype(np.int64)
    assert kept[1] == cap and kept[2] == 0 and kept[3] == 0 and 0 < kept[0] < cap
    # the users matter: the same rows under another user keep another set
    assert any(not np.array_equal(world.keep[0], world.keep[v]) for v in (1, 2, 3))


def test_filter_table_is_the_sequential_reference(ctx, world):
    """the shared table against cond_ref's own walk over the candidates, rows gathered from the store, on one small request set"""
    rng = np.random.default_rng(5)
    case = make_case(rng, 4, 130, ("mixed", "mixed_full", "all", "none"), n64=2, n32=1)
    variants = [0, 1, 2, 3]
    direct = ref.item_state_filter(FILTER_RULES[0]["Conditions"], world.store, S, *case, users=[USERS[v] for v in variants])
    trim_ref.same(want_filter(world, case, variants), direct)
    trim_ref.same(run_filter(ctx, world, case, [USERS[v] for v in variants]), direct)
    got = ctx.item_state_filter(world.filter, world.fs, *case, users=[USERS[v] for v in variants])
    trim_ref.same(got, direct)


def test_filter_in_lists_of_one_and_sixty_four(ctx, world):
    rng = np.random.default_rng(9)
    case = make_case(rng, 2, 300, ("mixed_full",), n64=1, n32=1, optional=False)
    for values in ([(1 << 40) + 3], LIST64, [(1 << 31) + 9, -(1 << 35)]):
        for op in ("in", "not_in"):
            conds = [{"Name": "c4", "Operator": op, "Type": "int", "Value": values}]
            cond = pa.cond_compile([{"Conditions": conds}], DECL)
            try:
                want = ref.item_state_filter(conds, world.store, S, *case)
                trim_ref.same(run_filter(ctx, world, case, [None, None], cond=cond), want)
                if op == "in" and len(values) == 1:
                    assert 0 < want[6].sum() < 40
            finally:
                cond.free()


def test_filter_refusals_leave_the_context_usable(ctx, world):
    case = make_case(np.random.default_rng(1), 1, 16, ("mixed_full",), n64=1, n32=1, optional=False)
    with pytest.raises(PgError) as ei:
        run_filter(ctx, world, case, [None], cond=world.boost)
    assert ei.value.code == -1 and "boost rule set" in str(ei.value)
    other = pa.cond_compile([{"Conditions": [{"Name": "c0", "Operator": "equal", "Type": "int", "Value": 1}]}], [("c0", pa.F_I64)])
    try:
        with pytest.raises(PgError) as ei:
            run_filter(ctx, world, case, [None], cond=other)
        assert ei.value.code == -1 and '"c0"' in str(ei.value) and "dtype" in str(ei.value)
    finally:
        other.free()
    with pytest.raises(PgError) as ei:
        ctx.item_state_filter_dev(world.filter, world.fs, 1, 16385, 8, 8, 0, 0, 0, 0, 0, 0, 0, 8, 8, 16, 16, 0, 0, 0, 0, 16)
    assert ei.value.code == -4 and "cap=16385" in str(ei.value)
    with pytest.raises(PgError) as ei:
        ctx.item_state_filter_dev(world.filter, world.fs, 1, 16, 4096, 8192, 0, 0, 0, 0, 0, 0, 0, 8, 8, 4096 + 64, 16384, 0, 0, 0, 0, 32768)
    assert ei.value.code == -1 and "overlaps" in str(ei.value)
    # what the checks of the candidate lists answer, code and text (recorded from the build before cand_lists.hpp stated them once);
    # every address is made up: the calls are refused before anything reaches the stream
    d = 1 << 16

    def call(nq=1, cap=16, **kw):
        a = dict(d_rows=d, d_score=2 * d, d_source=3 * d, d_count=0, d_planes_f64=0, n_f64=0, d_source_mask=0, d_planes_f32=0, n_f32=0,
                 d_user_vals=8, d_user_present=8, d_out_rows=4 * d, d_out_score=5 * d, d_out_source=6 * d, d_out_planes_f64=0,
                 d_out_source_mask=0, d_out_planes_f32=0, d_out_count=7 * d)
        a.update(kw)
        ctx.item_state_filter_dev(world.filter, world.fs, nq, cap, **a)

    for kw, code, text in ((dict(d_out_source=0), -1, "d_source / d_source_mask and their outputs come in pairs"),
                           (dict(d_source_mask=8 * d), -1, "d_source / d_source_mask and their outputs come in pairs"),
                           (dict(d_planes_f64=8 * d, n_f64=1), -1, "a carried plane set and its output come in pairs"),
                           (dict(d_planes_f64=8 * d, d_out_planes_f64=9 * d, n_f64=0), -1, "a carried plane set holds 1..8 planes"),
                           (dict(d_planes_f64=8 * d, d_out_planes_f64=9 * d, n_f64=9), -1, "a carried plane set holds 1..8 planes"),
                           (dict(d_rows=0), -1, "NULL argument"), (dict(nq=0), -1, "nq=0 must be in [1,256]"),
                           (dict(cap=0), -4, "cap=0 unsupported (1..16384)")):
        with pytest.raises(PgError) as ei:
            call(**kw)
        assert ei.value.code == code and str(ei.value).endswith(": pg_item_state_filter_dev: " + text), kw
    trim_ref.same(run_filter(ctx, world, case, [USERS[0]]), want_filter(world, case, [0]))


# ---- the boost ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", CAPS)
def test_boost_sizes(ctx, world, cap):
    rng = np.random.default_rng(7 * cap)
    rows, score, count = boost_case(world, rng, 3, cap, ("mixed", "all", "none" if cap % 2 else "nothing"))
    for fa in (False, True):
        got_s, got_r = run_boost(ctx, world, rows, score, count, [USERS[0], USERS[1], USERS[0]], fa)
        want_s, want_r = want_boost(world, rows, score, count, [0, 1, 0], fa)
        assert np.array_equal(got_r, want_r), np.argwhere(got_r != want_r)[:4].tolist()
        assert np.array_equal(ref.score_bits(got_s), ref.score_bits(want_s)), np.argwhere(ref.score_bits(got_s) != ref.score_bits(want_s))[:4].tolist()
        untouched = want_r == 0xFF                                          # padding and entries no rule matched: the very bits
        assert np.array_equal(got_s.view(np.uint64)[untouched], score.view(np.uint64)[untouched])


def test_boost_eight_rules_chain_and_errors_still_match(ctx, world):
    s_all, r_all = world.boosted[0, True]
    s_first, r_first = world.boosted[0, False]
    # rows [0, A) match every rule under the full user: with filter_all the last rule applied is rule 7 and the score went through
    # all eight expressions; without it rule 0 alone
    assert np.all(r_all[:A] == 7) and np.all(r_first[:A] == 0)
    inside = np.ones(A, dtype=bool)
    cols = {n: a[:A] for n, a in world.store.items()}
    chained = world.score_of[:A].copy()
    for k, ru in enumerate(BOOST_RULES):
        chained = ref.boost([{"Conditions": [], "Expression": ru["Expression"]}], False, chained, cols, inside, {})[0]
    assert np.array_equal(ref.score_bits(chained), ref.score_bits(s_all[:A]))
    # a row outside the store: rule 0 (no conditions) matches, its expression names a column and errors, the score stays, and
    # without filter_all the walk still ends there
    assert np.all(r_first[S:] == 0) and np.array_equal(s_first[S:].view(np.uint64), world.score_of[S:].view(np.uint64))
    rows = np.concatenate([np.arange(A, dtype=np.uint64), np.arange(S, S + J, dtype=np.uint64), [HUGE]])[None, :]
    score = world.score_of[index_of(rows)].copy()
    for fa in (False, True):
        got_s, got_r = run_boost(ctx, world, rows, score, None, [USERS[0]], fa)
        want_s, want_r = want_boost(world, rows, score, None, [0], fa)
        assert np.array_equal(got_r, want_r) and np.array_equal(ref.score_bits(got_s), ref.score_bits(want_s))
    # the rule plane is optional
    got_s, none = run_boost(ctx, world, rows, score, None, [USERS[0]], True, want_rule=False)
    assert none is None and np.array_equal(ref.score_bits(got_s), ref.score_bits(want_boost(world, rows, score, None, [0], True)[0]))


def test_boost_256_requests(ctx, world):
    rng = np.random.default_rng(65)
    nq, cap = 256, 65
    rows, score, count = boost_case(world, rng, nq, cap, ("mixed", "all", "none", "nothing", "mixed_full"))
    variants = [q % 2 for q in range(nq)]
    got_s, got_r = run_boost(ctx, world, rows, score, count, [USERS[v] for v in variants], True)
    want_s, want_r = want_boost(world, rows, score, count, variants, True)
    assert np.array_equal(got_r, want_r) and np.array_equal(ref.score_bits(got_s), ref.score_bits(want_s))
    got_s2, got_r2 = ctx.boost_scores(world.boost, world.fs, rows, score, count, [USERS[v] for v in variants], True)
    assert np.array_equal(got_r2, got_r) and np.array_equal(got_s2.view(np.uint64), got_s.view(np.uint64))


def test_boost_fractional_power_within_the_device_pow(ctx, world):
    """`**` with a fractional exponent goes through pow(): compared as the expression tests compare OP_POW, within the device
    pow's last ulp, not by bits"""
    cond = pa.cond_compile([{"Conditions": [], "Expression": "(score * score + c11) ** 0.3"}], DECL, boost=True)
    try:
        rows = np.arange(512, dtype=np.uint64)[None, :]
        score = world.score_of[:512][None, :].copy()
        uv, up = cond.pack_user([None])
        got = ctx.boost_scores(cond, world.fs, rows, score, None, [None], False)[0]
        want = np.array([math.pow(s * s + c, 0.3) for s, c in zip(score[0], world.store["c11"][:512])])
        assert np.allclose(got[0], want, rtol=4e-16, atol=0.0)
    finally:
        cond.free()


# ---- one request on host arrays; the chain ----------------------------------------------------------------------------------------

def test_one_request_entries_equal_the_dev_ones(ctx, world):
    rng = np.random.default_rng(77)
    for cap in (1, 700, 2049):
        rows, n = request_rows(rng, cap, "mixed_full")
        score = world.score_of[index_of(rows)].copy()
        source = rng.integers(0, 8, cap).astype(np.uint8)
        case = (rows[None, :], score[None, :], source[None, :], None, None, None, None)
        dev = run_filter(ctx, world, case, [USERS[1]])
        o_r, o_s, o_src, cnt = ctx.item_state_filter_one(world.filter, world.fs, rows, score, source, USERS[1])
        assert cnt == dev[6][0] and np.array_equal(o_r, dev[0][0]) and np.array_equal(o_s.view(np.uint64), dev[1][0].view(np.uint64))
        assert np.array_equal(o_src, dev[2][0])
        # pg_boost_scores takes the candidates' own values: the store's rows gathered on the host (padding has none: left out)
        live = rows != U64MAX
        cols, inside = ref.gather(world.store, S, rows[live])
        for fa in (False, True):
            d_s, d_r = run_boost(ctx, world, rows[None, :], score[None, :], None, [USERS[0]], fa)
            h_s, h_r = ctx.boost_scores_one(world.boost, score[live], cols, inside, USERS[0], fa)
            assert np.array_equal(h_r, d_r[0][live]) and np.array_equal(h_s.view(np.uint64), d_s[0][live].view(np.uint64))


def test_fanin_then_filter_then_trim(ctx, world):
    """pg_fanin_merge_dev → pg_item_state_filter_dev → pg_candidates_trim_dev: each stage takes the one before it as it is, and the
    page equals the three references composed"""
    rng = np.random.default_rng(31)
    nq, ks = 3, (300, 200, 120)
    src = []
    for i, k in enumerate(ks):
        rows = np.stack([rng.choice(S + J, k, replace=False).astype(np.uint64) for _ in range(nq)])
        sc = rng.standard_normal((nq, k))
        src.append((rows, sc if i == 1 else sc.astype(np.float32)))
    m = ctx.fanin_merge(src)                                             # rows, score, source, planes, mask, count
    wm = fanin_ref.merge(src)
    users = [USERS[0], USERS[1], USERS[3]]
    f = ctx.item_state_filter(world.filter, world.fs, m[0], m[1], m[2], m[5], m[3], m[4], None, users)
    keep = np.stack([world.keep[v][index_of(wm[0][q])] for q, v in enumerate((0, 1, 3))])
    wf = ref.item_state_filter(None, None, S, wm[0], wm[1], wm[2], wm[5], wm[3], wm[4], None, keep=keep)
    trim_ref.same(f, wf)
    assert np.all(f[6] > 0) and np.all(f[6] < m[5])
    rules = [(0, pa.TRIM_FIX, 40), (1, pa.TRIM_ACCUMULATE, 90), (2, pa.TRIM_ACCUMULATE, 120)]
    t = ctx.candidates_trim(rules, f[0], f[1], f[2], f[6], f[3], f[4])
    trim_ref.same(t, trim_ref.trim(rules, wf[0], wf[1], wf[2], wf[6], wf[3], wf[4]))


def test_boost_in_place_and_empty_requests(ctx, world):
    """d_out_score may be d_score itself; the one-request entries answer an empty request with an empty answer"""
    rng = np.random.default_rng(8)
    rows, score, count = boost_case(world, rng, 2, 1500, ("mixed", "all"))
    uv, up = world.boost.pack_user([USERS[0], USERS[1]])
    bufs = [ctx.to_device(a) for a in (rows, score, count, uv, up)]
    d_rule = ctx.malloc(rows.size)
    try:
        ctx.boost_scores_dev(world.boost, world.fs, True, 2, 1500, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], bufs[1], d_rule)
        ctx.synchronize()
        got_s, got_r = np.empty_like(score), np.empty(rows.shape, np.uint8)
        ctx.d2h(got_s, bufs[1])
        ctx.d2h(got_r, d_rule)
    finally:
        for b in bufs + [d_rule]:
            ctx.free(b)
    want_s, want_r = want_boost(world, rows, score, count, [0, 1], True)
    assert np.array_equal(got_r, want_r) and np.array_equal(ref.score_bits(got_s), ref.score_bits(want_s))
    none = np.zeros(0, np.uint64)
    o_r, o_s, o_src, cnt = ctx.item_state_filter_one(world.filter, world.fs, none, np.zeros(0), None, USERS[0])
    assert cnt == 0 and o_r.size == 0 and o_s.size == 0 and o_src is None
    s, r = ctx.boost_scores_one(world.boost, np.zeros(0), {n: np.zeros(0, t) for n, t in DTYPES.items()}, None, USERS[0])
    assert s.size == 0 and r.size == 0
