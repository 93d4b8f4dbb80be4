"""pg_expr_eval_host — the host statement of what expr_eval_kernel computes (expr.hip: expr_run_host over the shared expr_binop /
go_pow of expr_prog.hpp) — against the references of the three front ends on hostile values and at the compiler's limits
(cases: tests/expr_cases.py; the GPU counterpart, on the same cases, is test_gpu_expr.py).  Host and references share one libm,
so every comparison here is verdict for verdict and bit for bit, `^` included."""
import numpy as np
import pytest

import expr_cases as xc
from pairec_amd._lib import PgError


def _mismatches(fe, src, vmat, ok, val, gok, got, limit=8):
    bad = [i for i in range(len(ok)) if gok[i] != ok[i] or (ok[i] and not xc.same_bits(got[i], val[i]))]
    return ["%s %s item %d %r: reference %s, library %s" % (fe, src, i, [float(x).hex() for x in vmat[:, i]],
                                                            float(val[i]).hex() if ok[i] else "error",
                                                            float(got[i]).hex() if gok[i] else "error") for i in bad[:limit]], len(bad)


@pytest.mark.parametrize("fe,src", xc.table_cases(), ids=lambda p: str(p))
def test_operator_table_on_the_hostile_grid(fe, src):
    """one expression per operator over all 37 x 37 ordered pairs: same verdict, same bits, no exception for `^`"""
    ok, val, _ = xc.table_reference(fe, src)
    e = fe.compile(src)
    vmat = xc.bind(e, {"a": xc.PAIRS[0], "b": xc.PAIRS[1]}, xc.PAIRS.shape[1])
    gok, got = xc.eval_items(e.eval_host, vmat, ok)
    e.free()
    lines, n_bad = _mismatches(fe, src, vmat, ok, val, gok, got)
    assert n_bad == 0, "\n".join(lines)
    if fe is xc.DEFAULT and src[4] in "/%":
        assert not ok.all()                                     # (the zero divisors of the grid did raise, one call each)
    else:
        assert ok.all()                                         # antlr's `/`, govaluate's `/` and `%` never raise


@pytest.mark.parametrize("fe", xc.FRONT_ENDS, ids=str)
def test_random_expressions(fe):
    """150 seeded expressions x 64 items: same verdict, same bits on every item.  Also settled here, from the references alone: at
    least half of the items never reach libm's pow, and at most 5 % of those that do sit in front of a discontinuity — the two
    conditions under which the GPU test's looser comparison of the pow class cannot hide a failure."""
    total, exact, powc, sensitive = xc.random_census(fe)
    assert total == xc.N_RANDOM * xc.N_ITEMS
    assert 2 * exact >= total, (exact, total)
    assert powc > 0 and 20 * sensitive <= powc, (sensitive, powc)
    report, n_bad = [], 0
    for c in xc.random_cases(fe):
        e = fe.compile(c.src)
        vmat = xc.bind(e, c.cols, xc.N_ITEMS)
        gok, got = xc.eval_items(e.eval_host, vmat, c.ok)
        e.free()
        lines, k = _mismatches(fe, c.src, vmat, c.ok, c.val, gok, got, 2)
        report += lines
        n_bad += k
    assert n_bad == 0, "\n".join(report[:20])


@pytest.mark.parametrize("fe", xc.FRONT_ENDS, ids=str)
def test_compiler_limits(fe):
    """32 stack slots and 128 operations are served in full, one more of either is refused"""
    n = 5
    vals = xc.limit_values(65, n)
    total = lambda k: sum(vals["v%d" % j] for j in range(1, k + 1))

    e = fe.compile(xc.nest_source(fe, 32))
    assert len(e.var_names) == 32
    assert np.array_equal(e.eval_host(xc.bind(e, vals, n)), total(32))
    e.free()
    e = fe.compile(xc.nest_source(fe, 32, constants=(1, 32)))                  # (constants on slots 0 and 31)
    assert np.array_equal(e.eval_host(xc.bind(e, vals, n)), total(32) - vals["v1"] - vals["v32"] + 33.0)
    e.free()
    with pytest.raises(PgError) as ei:
        fe.compile(xc.nest_source(fe, 33))
    assert ei.value.code == xc.UNSUPPORTED and "depth 33" in str(ei.value)

    e = fe.compile(xc.chain_source(fe, 64))                     # 64 operands + 63 additions = 127 operations
    assert np.array_equal(e.eval_host(xc.bind(e, vals, n)), total(64))
    e.free()
    with pytest.raises(PgError) as ei:
        fe.compile(xc.chain_source(fe, 65))                     # 129
    assert ei.value.code == xc.UNSUPPORTED and "129" in str(ei.value)

    if fe is xc.DEFAULT:
        # every program of the default grammar is a binary tree — an odd number of operations: 127 is its largest, and a prefix
        # minus (read as 0 - v1: two operations more) on 64 terms is already 129
        with pytest.raises(PgError) as ei:
            fe.compile(xc.chain_source(fe, 64, negate_first=True))
        assert ei.value.code == xc.UNSUPPORTED and "129" in str(ei.value)
    else:
        e = fe.compile(xc.chain_source(fe, 64, negate_first=True))   # 128 operations: ExprDev's whole program array
        assert np.array_equal(e.eval_host(xc.bind(e, vals, n)), total(64) - 2.0 * vals["v1"])
        e.free()
        with pytest.raises(PgError) as ei:
            fe.compile("-(" + xc.chain_source(fe, 64) + ")+" + fe.var("v65"))       # 130
        assert ei.value.code == xc.UNSUPPORTED
