"""expr_eval_kernel (expr.hip) on hostile values and at its limits, against the references of the three front ends and against
pg_expr_eval_host: the cases of tests/expr_cases.py — the CPU test test_expr_hostile_cpu.py settles, without a device, that the
host statement and the references agree on them bit for bit, so whatever differs here is the device's.  Then the paths around
the kernel: item counts on either side of a block with a guard word behind the outputs, the arithmetic flag, the program and
stack limits, pg_fuse_scores_dev with strided planes and rewrites, pg_features_eval_dev over typed columns."""
import ctypes as C

import numpy as np
import pytest

import expr_cases as xc
import features_ref as fr
import pairec_amd as pa
from oracle import oracle as o
from pairec_amd._lib import PgError, check

pytestmark = pytest.mark.gpu

MAX_POW_ULP = 2          # a fractional `^` on the device is within 2 ulp of libm's


def _hex(x):
    return float(x).hex()


# ---- the operator table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fe,src", xc.table_cases(), ids=lambda p: str(p))
def test_operator_table_on_the_device(ctx, fe, src):
    """All 37 x 37 ordered pairs.  Pairs whose reference evaluation stays on go_pow's exact branches: the device's verdict and bits
    are the oracle's and the host statement's.  Pairs that reach libm's pow (a fractional exponent on a finite non-zero base): same
    class and sign, finite results within 2 representable doubles."""
    ok, val, lib = xc.table_reference(fe, src)
    e = fe.compile(src)
    vmat = xc.bind(e, {"a": xc.PAIRS[0], "b": xc.PAIRS[1]}, xc.PAIRS.shape[1])
    hok, host = xc.eval_items(e.eval_host, vmat, ok)
    gok, got = xc.eval_items(lambda v: e.eval(ctx, v), vmat, ok)
    e.free()
    bad, worst = [], (0, None)
    for i in range(ok.size):
        where = "%s %s (%s, %s): oracle %s host %s device %s" % (
            fe, src, _hex(xc.PAIRS[0, i]), _hex(xc.PAIRS[1, i]), _hex(val[i]) if ok[i] else "error",
            _hex(host[i]) if hok[i] else "error", _hex(got[i]) if gok[i] else "error")
        if gok[i] != ok[i] or gok[i] != hok[i]:
            bad.append("verdict " + where)
        elif not ok[i]:
            continue
        elif not lib[i]:
            if not (xc.same_bits(got[i], val[i]) and xc.same_bits(got[i], host[i])):
                bad.append("bits " + where)
        elif xc.klass(got[i]) != xc.klass(val[i]):
            bad.append("class " + where)
        elif np.isfinite(val[i]):
            d = xc.ulp_distance(got[i], val[i])
            if d > worst[0]:
                worst = (d, where)
            if d > MAX_POW_ULP:
                bad.append("%d ulp " % d + where)
    print("\n[expr table] %s %s: %d libm-branch pairs, largest distance %d ulp%s" % (
        fe, src, int(np.count_nonzero(lib)), worst[0], " at " + worst[1] if worst[1] else ""))
    assert not bad, "%d pairs differ:\n%s" % (len(bad), "\n".join(bad[:12]))


# ---- random expressions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fe", xc.FRONT_ENDS, ids=str)
def test_random_expressions_on_the_device(ctx, fe):
    """The CPU test's 150 x 64 items.  An item whose reference evaluation never reached libm's pow: same verdict, same bits.  The
    others: relative 1e-11; only an item the reference itself marks ulp-sensitive (test_expr_hostile_cpu.py bounds their share)
    may instead be explained by moving the reference's pow results by up to 2 ulp."""
    bad, explained, n_pow = [], 0, 0
    for c in xc.random_cases(fe):
        e = fe.compile(c.src)
        vmat = xc.bind(e, c.cols, xc.N_ITEMS)
        gok, got = xc.eval_items(lambda v: e.eval(ctx, v), vmat, c.ok)
        e.free()
        for i in range(xc.N_ITEMS):
            where = "%s %r item %d %r: oracle %s device %s" % (fe, c.src, i, c.env(i), _hex(c.val[i]) if c.ok[i] else "error",
                                                              _hex(got[i]) if gok[i] else "error")
            if c.n_libm[i] == 0:
                if gok[i] != c.ok[i] or (c.ok[i] and not xc.same_bits(got[i], c.val[i])):
                    bad.append("exact class: " + where)
                continue
            n_pow += 1
            if gok[i] == c.ok[i] and (not c.ok[i] or xc.close(got[i], c.val[i], 1e-11)):
                continue
            if not c.sensitive[i]:
                bad.append("pow class: " + where)
                continue
            env = c.env(i)
            if xc.nudge_explains(fe, c.ast, env, int(c.n_libm[i]), bool(gok[i]), float(got[i])) or (
                    fe is xc.DEFAULT and gok[i] and c.ok[i]
                    and o.pow_last_ulp_explains(lambda: o.expr_eval(c.ast, env.get), float(got[i]))):
                explained += 1
            else:
                bad.append("ulp-sensitive, unexplained: " + where)
    print("\n[expr random] %s: %d pow-class items, %d explained by pow's last ulps" % (fe, n_pow, explained))
    assert not bad, "%d items differ:\n%s" % (len(bad), "\n".join(bad[:12]))


# ---- item counts around a 256-thread block, with a guard word behind the outputs ---------------------------------------------------
GUARD = 0xDEADBEEFCAFEF00D


def _eval_dev_guarded(ctx, e, vmat, n):
    """pg_expr_eval_dev into n + 1 doubles of the guard pattern → the n + 1 words after the call"""
    d_v = ctx.to_device(vmat)
    d_o = ctx.to_device(np.full(n + 1, GUARD, dtype=np.uint64))
    out = np.zeros(n + 1, dtype=np.uint64)
    try:
        check(ctx.L.pg_expr_eval_dev(ctx.h, e.h, C.c_void_p(d_v), n, C.c_void_p(d_o)))
        ctx.d2h(out, d_o)
    finally:
        ctx.free(d_v)
        ctx.free(d_o)
    return out


@pytest.mark.parametrize("n", [1, 255, 256, 257, 511, 513])
def test_item_counts_around_a_block(ctx, n):
    src = "${a}*2+${b}#1"
    rng = np.random.default_rng(n)
    a = np.floor(rng.standard_normal(n) * 1000.0)
    b = np.where(rng.random(n) < 0.4, 0.0, np.floor(rng.standard_normal(n) * 50.0))
    b[-1] = 0.0                                                 # (the last item takes `#`'s right side)
    ast = o.expr_parse(src)
    want = np.array([o.expr_eval(ast, {"a": a[i], "b": b[i]}.get) for i in range(n)])
    e = pa.Expr(src)
    assert e.var_names == ["a", "b"]
    out = _eval_dev_guarded(ctx, e, np.stack([a, b]), n)
    assert np.array_equal(out[:n], want.view(np.uint64))
    assert out[n] == GUARD
    assert np.array_equal(e.eval(ctx, np.stack([a, b])).view(np.uint64), want.view(np.uint64))
    e.free()


# ---- the arithmetic flag -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [0, 255, 256, 512])
def test_one_zero_divisor_fails_the_call_and_the_next_call_is_clean(ctx, at):
    n = 513
    a = np.arange(1.0, n + 1.0)
    b = np.full(n, 4.0)
    b[at] = 0.0
    for src in ("${a}/${b}", "${a}%${b}"):
        e = pa.Expr(src)
        with pytest.raises(PgError) as ei:
            e.eval(ctx, np.stack([a, b]))
        assert ei.value.code == xc.ARITH and "'%s'" % src in str(ei.value)
        clean = e.eval(ctx, np.stack([a, np.full(n, 4.0)]))          # the flag does not outlive the call
        assert np.array_equal(clean, a / 4.0 if "/" in src else np.fmod(a, 4.0))
        e.free()
    # antlr's `/`, govaluate's `/` and `%` are Go's float operations: a zero divisor is a value, never an error
    for fe, src in ((xc.ANTLR, "${a}/${b}"), (xc.GOVALUATE, "a / b"), (xc.GOVALUATE, "a % b")):
        e = fe.compile(src)
        got = e.eval(ctx, np.stack([a, b]))
        ast = fe.parse(src)
        want = np.array([fe.ref(ast, {"a": a[i], "b": b[i]})[1] for i in range(n)])
        assert all(xc.same_bits(got[i], want[i]) for i in range(n))
        assert (np.isinf(got[at]) if "/" in src else np.isnan(got[at])) and np.isfinite(np.delete(got, at)).all()
        e.free()


# ---- programs at the limits: 32 stack slots, 127 and 128 operations ----------------------------------------------------------------
@pytest.mark.parametrize("fe", xc.FRONT_ENDS, ids=str)
def test_programs_at_the_stack_and_length_limits(ctx, fe):
    n = 257
    vals = xc.limit_values(64, n)
    total = lambda k: sum(vals["v%d" % j] for j in range(1, k + 1))
    cases = [(xc.nest_source(fe, 32), total(32)), (xc.chain_source(fe, 64), total(64))]
    if fe is not xc.DEFAULT:                                    # (a default-grammar program has an odd length: 127 is its limit)
        cases.append((xc.chain_source(fe, 64, negate_first=True), total(64) - 2.0 * vals["v1"]))
    for k, (src, want) in enumerate(cases):
        e = fe.compile(src)
        vmat = xc.bind(e, vals, n)
        got = e.eval(ctx, vmat)
        assert np.array_equal(got.view(np.uint64), e.eval_host(vmat).view(np.uint64))
        assert np.array_equal(got, want)
        # the last operand pushed — slot 31 of the stack in the nest, operation 127 in the chains — decides the answer
        last = e.var_names.index("v32" if k == 0 else "v64")
        vmat[last] += np.arange(1.0, n + 1.0)
        assert np.array_equal(e.eval(ctx, vmat), want + np.arange(1.0, n + 1.0))
        e.free()
    with pytest.raises(PgError) as ei:
        fe.compile(xc.nest_source(fe, 33))
    assert ei.value.code == xc.UNSUPPORTED


# ---- pg_fuse_scores_dev: strided planes, rewrites, the variable limit --------------------------------------------------------------
F32_DENORMAL, F32_MAX = np.float32(1e-45), np.float32(3.4028235e38)
GAP = np.float32(-12345.0)


def _fuse(ctx, ex, names, planes, stride, rec):
    """pg_fuse_scores_dev over planes [P][stride] (only the first n entries of a plane are items) → fused [n]"""
    n = rec.size
    arr = (C.c_char_p * len(names))(*[nm.encode() for nm in names])
    d_rank, d_rec, d_out = ctx.to_device(planes), ctx.to_device(rec), ctx.malloc(n * 8)
    out = np.zeros(n, dtype=np.float64)
    try:
        check(ctx.L.pg_fuse_scores_dev(ctx.h, ex.h, arr, len(names), C.c_void_p(d_rank), stride, C.c_void_p(d_rec), n, C.c_void_p(d_out)))
        ctx.d2h(out, d_out)
    finally:
        for p in (d_rank, d_rec, d_out):
            ctx.free(p)
    return out


def _planes(n_planes, n, seed):
    """planes [P][n + 7] f32 with the gap pattern behind every plane's n items and fp32's edge values among the items; recall [n]"""
    rng = np.random.default_rng(seed)
    stride = n + 7
    planes = np.full((n_planes, stride), GAP, dtype=np.float32)
    planes[:, :n] = rng.standard_normal((n_planes, n)).astype(np.float32)
    rec = rng.random(n).astype(np.float32)
    for p in range(n_planes):
        planes[p, 3 * p] = F32_DENORMAL
        planes[p, 3 * p + 1] = F32_MAX
        planes[p, 3 * p + 2] = np.float32(-0.0)
        planes[p, n - 1 - p] = -F32_MAX
    rec[n - 40], rec[n - 41], rec[n - 42] = F32_DENORMAL, np.float32(-0.0), F32_MAX
    return planes, stride, rec


def _fuse_oracle(src, rewrites, names, planes, rec):
    out = np.empty(rec.size, dtype=np.float64)
    for i in range(rec.size):
        it = o.OracleItem(str(i), float(rec[i]))
        for p, nm in enumerate(names):
            it.add_algo_score(nm, float(planes[p, i]))
        o.fuse_scores(src, [it], score_rewrite=rewrites)
        out[i] = it.score
    return out


def _check_fuse(ctx, src, rewrites, names, planes, stride, rec, n_vars):
    ex = pa.Expr(src)
    assert len(ex.var_names) == n_vars
    if rewrites:
        ex.set_score_rewrites(rewrites)
    got = _fuse(ctx, ex, names, planes, stride, rec)
    ex.free()
    want = _fuse_oracle(src, rewrites, names, planes, rec)
    diff = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert diff.size == 0, [(int(i), _hex(got[i]), _hex(want[i])) for i in diff[:8]]
    return got


def test_fuse_scores_dev_with_strided_planes_and_rewrites(ctx):
    """Three planes rank_stride = n + 7 apart.  The RankScore holds 32 operand references — 30 to the planes in turn, current_score
    and a rewrite's source — and a 33rd to a source whose expression does not compile (it scores 0).  (Variables are bound by
    NAME: these are 6 of them.  The most a scene can bind is 12 planes + current_score + 8 rewrite sources = 21: second case.)
    No `^` anywhere: d_fused equals oracle.fuse_scores bit for bit."""
    n = 300
    names = ["p0", "p1", "p2"]
    planes, stride, rec = _planes(3, n, 11)
    # (53 operands, 105 operations: 30 references with a coefficient each would not fit the 128-operation program)
    terms = ["${p%d}%s" % (j % 3, "*%s" % ((j + 1) * 0.25) if j % 3 != 2 else "") for j in range(30)]
    src = "".join(("+" if j % 2 == 0 else "-") + t for j, t in enumerate(terms))[1:] + "+${current_score}+${rw1}+${bad}"
    rewrites = {"rw1": "${p0}*0.5+${current_score}/(${p1}*${p1}+1)#3", "bad": "${p0} @ 1"}
    _check_fuse(ctx, src, rewrites, names, planes, stride, rec, 6)

    # the fp32 → fp64 widening alone: every plane and current_score as they are, edge values included
    for p, nm in enumerate(names + ["current_score"]):
        got = _check_fuse(ctx, "${%s}" % nm, None, names, planes, stride, rec, 1)
        src32 = rec if nm == "current_score" else planes[p, :n]
        assert np.array_equal(got.view(np.uint64), src32.astype(np.float64).view(np.uint64))
        if nm != "current_score":
            assert got[3 * p] == 2.0 ** -149 and got[3 * p + 1] == float(F32_MAX) and _hex(got[3 * p + 2]) == "-0x0.0p+0"

    # as many variables as a scene can bind: 12 planes, current_score, 8 rewrite sources
    names = ["q%d" % p for p in range(12)]
    planes, stride, rec = _planes(12, n, 12)
    rewrites = {"s%d" % r: "${q%d}*2-${q%d}#${current_score}+%d" % (r, r + 4, r) for r in range(8)}
    src = "+".join("${q%d}*%s" % (p, (p + 1) * 0.5) for p in range(12)) + "-${current_score}" + "".join("+${s%d}/%d" % (r, r + 2) for r in range(8))
    _check_fuse(ctx, src, rewrites, names, planes, stride, rec, 21)


def test_fuse_scores_dev_refusals(ctx):
    n = 300
    names = ["p0", "p1", "p2"]
    planes, stride, rec = _planes(3, n, 13)
    ex = pa.Expr("+".join("${x%d}" % j for j in range(33)))
    with pytest.raises(PgError) as ei:
        _fuse(ctx, ex, names, planes, stride, rec)
    assert ei.value.code == xc.UNSUPPORTED and "33 variables (at most 32)" in str(ei.value)
    ex.free()
    # a division by zero inside a rewrite is the call's arithmetic error; one item is enough, and the next call is clean
    ex = pa.Expr("${p0}+${boost}")
    ex.set_score_rewrites({"boost": "1/(${p1}-${p2})"})
    planes[2, 256] = planes[1, 256]
    with pytest.raises(PgError) as ei:
        _fuse(ctx, ex, names, planes, stride, rec)
    assert ei.value.code == xc.ARITH
    planes[2, 256] = planes[1, 256] + np.float32(1.0)
    got = _fuse(ctx, ex, names, planes, stride, rec)
    ex.free()
    want = _fuse_oracle("${p0}+${boost}", {"boost": "1/(${p1}-${p2})"}, names, planes, rec)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


# ---- pg_features_eval_dev: the same hostile numbers as typed columns ----------------------------------------------------------------
def test_features_eval_dev_over_typed_columns(ctx):
    rows, n = 96, 257
    rng = np.random.default_rng(21)
    i64 = np.iinfo(np.int64)
    hostile = {
        pa.F_I32: [-(1 << 31), (1 << 31) - 1, -1, 0],
        pa.F_I64: [i64.min, i64.max, (1 << 53) + 1, -1, -((1 << 53) + 1), (1 << 62) + 1],
        pa.F_F32: [np.nan, np.inf, -np.inf, -0.0, 1e-45, 3.4028235e38],
        pa.F_F64: [np.nan, np.inf, -np.inf, -0.0, 5e-324, 1e308, 2.0 ** 63],
    }
    np_type = {pa.F_I32: np.int32, pa.F_I64: np.int64, pa.F_F32: np.float32, pa.F_F64: np.float64}
    fs = pa.Features(ctx, rows)
    cols, defaults = {}, {}
    for c, (kind, dtype) in enumerate((k, d) for k in range(4) for d in (("i32", pa.F_I32), ("i64", pa.F_I64), ("f32", pa.F_F32), ("f64", pa.F_F64))):
        name = "%s_%d" % (dtype[0], kind)
        if dtype[1] in (pa.F_I32, pa.F_I64):
            v = rng.integers(-1000, 1000, rows).astype(np_type[dtype[1]])
        else:
            v = (rng.standard_normal(rows) * 10.0).astype(np_type[dtype[1]])
        for t, h in enumerate(hostile[dtype[1]]):               # (each column's edge values on rows of its own: few items are all-NaN)
            v[(7 * c + t) % rows] = h
        default = -0.0 if c == 15 else -1.5 * (c + 1)
        fs.set_column(name, dtype[1], v, default=default)
        # what a row outside the store reads: the default rounded to the column's dtype (pairec_gpu.h, THE STORED DEFAULT) — an
        # integer column given -1.5 stores -1
        cols[name], defaults[name] = v, float(fr.stored_default(dtype[1], default))
    assert defaults["i32_0"] == -1.0 and defaults["f32_0"] == -4.5 and defaults["f64_3"] == 0.0 and np.signbit(defaults["f64_3"])
    names = list(cols)
    assert len(names) == 16
    r = np.concatenate([rng.permutation(rows), rng.integers(0, rows, n - rows)]).astype(np.uint32)
    r[[100, 101, 255, 256]] = [0xFFFFFFFF, rows, rows, 0xFFFFFFFF]          # outside the store: the column defaults
    inside = r < rows
    # what the kernel must bind: numpy's own conversion of every typed value to float64 (int64: round to nearest even)
    gathered = {nm: np.where(inside, cols[nm][np.minimum(r, rows - 1)].astype(np.float64), defaults[nm]) for nm in names}
    assert gathered["i64_0"].max() == 2.0 ** 63 and 2.0 ** 53 in gathered["i64_0"]

    def want_of(src):
        ast = o.expr_parse(src)
        return np.array([o.expr_eval(ast, {nm: gathered[nm][i] for nm in names}.get) for i in range(n)])

    def same(got, want):
        return all(xc.same_bits(got[i], want[i]) for i in range(n))

    src = "-".join("(${i32_%d}#${f64_%d})*(${f32_%d}#2)+${i64_%d}%%1000" % (k, k, k, k) for k in range(4))
    e = pa.Expr(src)
    assert sorted(e.var_names) == sorted(names)
    got = fs.eval_expr(e, r)
    e.free()
    want = want_of(src)
    assert same(got, want) and np.count_nonzero(np.isfinite(want)) > n // 2
    for nm in names:                                            # every column by itself: the conversion, value for value
        e = pa.Expr("${%s}" % nm)
        got = fs.eval_expr(e, r)
        e.free()
        assert same(got, gathered[nm]), nm
    e = pa.Expr("+".join("${%s}" % nm for nm in names) + "+${one_more}")
    with pytest.raises(PgError) as ei:
        fs.eval_expr(e, r)
    assert "17 variables (at most 16" in str(ei.value)
    e.free()
    fs.destroy()
