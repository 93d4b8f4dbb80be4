"""Cases for the expression evaluator's hostile-value tests (test_expr_hostile_cpu.py on pg_expr_eval_host, test_gpu_expr.py on
expr_eval_kernel): the 37-value grid, one expression per operator of each front end, seeded random expressions with their
items, the programs at the compiler's limits, and the comparisons.  Everything a test expects comes from the references —
oracle.expr_eval (default grammar), oracle.antlr_result (antlr), cond_ref.expr_eval (govaluate) — never from the library, so
the CPU and the GPU test see identical inputs and identical expectations."""
import contextlib
import functools
import itertools
import math
import struct

import numpy as np

import cond_ref
import pairec_amd as pa
from oracle import oracle as o
from pairec_amd._lib import PgError

ARITH, UNSUPPORTED = -5, -4
INF, NAN = math.inf, math.nan

GRID = (0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 3.0, -3.0, 0.1,
        7.0, -7.0, 7.9, -7.9,
        1e308, -1e308, 5e-324, -5e-324, 2.2250738585072014e-308,
        2.0 ** 63, -2.0 ** 63, 2.0 ** 62, 2.0 ** 53 + 2.0, 1e15 + 0.5,
        1024.0, 1025.0, -1025.0, 4097.0,
        1e19, -1e19,
        INF, -INF, NAN,
        400.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53)
assert len(GRID) == 37
# all ordered pairs: item i * 37 + j is (GRID[i], GRID[j])
PAIRS = np.array([[a for a in GRID for _ in GRID], [b for _ in GRID for b in GRID]], dtype=np.float64)


# ---- the three front ends ------------------------------------------------------------------------------------------------------
class FrontEnd:
    def __init__(self, name, var_fmt, pow_op, binary, table):
        self.name, self.var_fmt, self.pow_op, self.binary, self.table = name, var_fmt, pow_op, binary, table

    def __repr__(self):
        return self.name

    def var(self, name):
        return self.var_fmt % name

    def compile(self, src):
        if self.name == "govaluate":
            return pa.Expr(src, govaluate=True)
        return pa.Expr(src, "antlr" if self.name == "antlr" else "")

    def parse(self, src):
        if self.name == "default":
            return o.expr_parse(src)
        if self.name == "antlr":
            return o.antlr_parse(src)
        return cond_ref.expr_parse(src)

    def ref(self, ast, env):
        """(ok, value): ok False where the reference panics (a zero divisor of the default grammar's `/` and `%`)"""
        if self.name == "default":
            try:
                return True, float(o.expr_eval(ast, env.get))
            except o.ExprError:
                return False, NAN
        if self.name == "antlr":
            return True, float(o.antlr_result(ast, env))
        with np.errstate(all="ignore"):
            return True, float(cond_ref.expr_eval(ast, env))


DEFAULT = FrontEnd("default", "${%s}", "^", "+-*/%^#",
                   ["${a}%s${b}" % op for op in "+-*/%^#"])
ANTLR = FrontEnd("antlr", "${%s}", "^", "+-*/^",
                 ["${a}%s${b}" % op for op in "+-*/^"] + ["-${a}", "-(${a}^${b})"])
GOVALUATE = FrontEnd("govaluate", "%s", "**", ["+", "-", "*", "/", "%", "**"],
                     ["a %s b" % op for op in ("+", "-", "*", "/", "%", "**")] + ["-a", "round(a)", "round(a, b)"])
FRONT_ENDS = (DEFAULT, ANTLR, GOVALUATE)


# ---- go_pow's libm branch: recorded, and nudged, from the reference alone -------------------------------------------------------
def took_libm(x, y):
    """oracle.go_pow(x, y) ends in libm's pow on a finite non-zero base: a fractional exponent other than Go's exact +-0.5 case.
    There the device's pow may differ in the last ulps; everywhere else go_pow is exact branches only."""
    return math.isfinite(x) and x != 0.0 and math.isfinite(y) and y != math.trunc(y) and abs(y) != 0.5


@contextlib.contextmanager
def pow_hook(shifts=()):
    """Every go_pow call of the references inside the block is logged (True: the libm branch); the result of the k-th libm-branch
    call moves by shifts[k] representable doubles (all three references reach go_pow through the oracle module's global)."""
    orig, log = o.go_pow, []

    def hooked(x, y):
        r = orig(x, y)
        lib = took_libm(x, y)
        if lib:
            k = sum(log)
            s = shifts[k] if k < len(shifts) else 0
            if s and math.isfinite(r) and r != 0.0:
                for _ in range(abs(s)):
                    r = math.nextafter(r, INF if s > 0 else -INF)
        log.append(lib)
        return r
    o.go_pow = hooked
    try:
        yield log
    finally:
        o.go_pow = orig


def ref_item(fe, ast, env, shifts=()):
    """(ok, value, number of libm-branch pow calls) of one item by the front end's reference"""
    with pow_hook(shifts) as log:
        ok, v = fe.ref(ast, env)
    return ok, v, sum(log)


# ---- comparisons -----------------------------------------------------------------------------------------------------------------
def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def same_bits(a, b):
    """bit for bit; a NaN matches a NaN of any payload or sign; -0.0 is not +0.0"""
    return (a != a and b != b) or bits(a) == bits(b)


def klass(x):
    if x != x:
        return "nan"
    s = "-" if math.copysign(1.0, x) < 0 else "+"
    return s + ("inf" if math.isinf(x) else "0" if x == 0.0 else "finite")


def ulp_distance(a, b):
    """representable doubles between two finite values (by bit pattern: subnormal results are judged as fairly as normal ones)"""
    def key(x):
        u = bits(x)
        return -(u & 0x7FFFFFFFFFFFFFFF) if u >> 63 else u
    return abs(key(a) - key(b))


def close(a, b, rel):
    if a != a or b != b:
        return a != a and b != b
    if a == b:
        return True
    return math.isfinite(a) and math.isfinite(b) and abs(a - b) <= rel * max(abs(b), 1e-300)


def ulp_sensitive(fe, ast, env, ok, val, n_libm):
    """the reference's own answer moves by more than 1e-11 relative (or changes its verdict) when one of its first three libm-branch
    pow results is nudged by 1 or 2 ulp: a power in front of something discontinuous or ill-conditioned"""
    for j in range(min(n_libm, 3)):
        for s in (-2, -1, 1, 2):
            ok2, v2, _ = ref_item(fe, ast, env, (0,) * j + (s,))
            if ok2 != ok or (ok and not close(v2, val, 1e-11)):
                return True
    return False


def nudge_explains(fe, ast, env, n_libm, got_ok, got):
    """the library's verdict and value are reproduced by the reference with its first three libm-branch pow results moved by up to
    2 ulp each, independently (oracle.pow_last_ulp_explains for any of the three references, verdicts included)"""
    for shifts in itertools.product((0, -1, 1, -2, 2), repeat=min(n_libm, 3)):
        ok2, v2, _ = ref_item(fe, ast, env, shifts)
        if ok2 == got_ok and (not got_ok or close(v2, got, 1e-10)):
            return True
    return False


# ---- running a library evaluation item by item -----------------------------------------------------------------------------------
def eval_items(run, vmat, ref_ok):
    """run(vmat) → values, or PgError -5 for the whole call when one item divides by zero.  The items the reference evaluates go
    in one call, every item it refuses in a call of its own (and every item singly if the one call is refused)
    → (ok [n] bool, values [n])"""
    n = vmat.shape[1]
    got, gok = np.full(n, NAN), np.zeros(n, dtype=bool)
    good = np.flatnonzero(ref_ok)
    singles = list(np.flatnonzero(~np.asarray(ref_ok)))
    if good.size:
        try:
            got[good] = run(np.ascontiguousarray(vmat[:, good]))
            gok[good] = True
        except PgError as ex:
            assert ex.code == ARITH, ex
            singles += list(good)
    for i in singles:
        try:
            got[i] = run(np.ascontiguousarray(vmat[:, i:i + 1]))[0]
            gok[i] = True
        except PgError as ex:
            assert ex.code == ARITH, ex
    return gok, got


def bind(e, cols, n):
    """the [n_vars][n] matrix of a compiled expression from named columns"""
    return np.stack([cols[nm] for nm in e.var_names]) if e.var_names else np.zeros((0, n))


# ---- the operator table ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table_reference(fe, src):
    """→ (ok [1369] bool, value [1369], libm [1369] bool) of `src` over PAIRS by the reference"""
    ast = fe.parse(src)
    n = PAIRS.shape[1]
    ok, val, lib = np.zeros(n, dtype=bool), np.full(n, NAN), np.zeros(n, dtype=bool)
    for i in range(n):
        ok[i], val[i], k = ref_item(fe, ast, {"a": PAIRS[0, i], "b": PAIRS[1, i]})
        lib[i] = k > 0
    return ok, val, lib


def table_cases():
    return [(fe, src) for fe in FRONT_ENDS for src in fe.table]


# ---- random expressions ----------------------------------------------------------------------------------------------------------
NAMES = ("ctr", "cvr", "price", "current_score", "a_b", "x1")
N_RANDOM, N_ITEMS = 150, 64
_SEED = 20240917


def gen(fe, rng, names, depth=0):
    """a random expression of the front end: depth <= 4, its operators, the given variables (after scripts/soak_expr.py's gen; the
    exponent of a power is a constant four times out of five — a small integer or a half, go_pow's exact branches, or a fraction, its
    libm branch — so that both classes of items are well populated)"""
    r = rng.random()
    if depth >= 4 or r < 0.3:
        k = int(rng.integers(0, 7))
        if k <= 2:
            return fe.var(names[int(rng.integers(0, len(names)))])
        if k == 3:
            return str(int(rng.integers(0, 1000)))
        if k == 4:
            return "%.3f" % (rng.random() * 10)
        if k == 5:
            return ("%de%d" % (int(rng.integers(1, 9)), int(rng.integers(0, 4)))) if fe is DEFAULT else str(int(rng.integers(1, 9)))
        return "0"
    if r < 0.4:
        return "(" + gen(fe, rng, names, depth + 1) + ")"
    if r < 0.45:
        # the default grammar reads "-x" as 0 - x; the other two bind a prefix minus their own way against a power: parenthesised
        return "-" + gen(fe, rng, names, depth + 1) if fe is DEFAULT else "(-(" + gen(fe, rng, names, depth + 1) + "))"
    if fe is GOVALUATE and r < 0.52:
        x = gen(fe, rng, names, depth + 1)
        return "round(%s)" % x if rng.random() < 0.5 else "round(%s, %d)" % (x, int(rng.integers(0, 4)))
    op = fe.binary[int(rng.integers(0, len(fe.binary)))]
    lhs = gen(fe, rng, names, depth + 1)
    if op == fe.pow_op:
        t = rng.random()
        if t < 0.45:
            rhs = ("2", "3", "0.5", "4", "1", "0")[int(rng.integers(0, 6))]
        elif t < 0.8:
            rhs = ("0.1", "1.5", "2.5", "0.333", "0.75", "3.862")[int(rng.integers(0, 6))]
        else:
            rhs = gen(fe, rng, names, depth + 1)
        if fe is DEFAULT:
            return lhs + op + rhs
        return "((" + lhs + ")" + op + "(" + rhs + "))"      # (a chained power and -a ^ b are refused by both sides: see expr.hip)
    sp = " " if rng.random() < 0.3 else ""
    return lhs + sp + op + sp + gen(fe, rng, names, depth + 1)


def draw(rng, n):
    """one variable's items: normal x {1e-3, 1, 50, 1e6}; non-negative integers; 30 % zeros; grid values"""
    kind = int(rng.integers(0, 4))
    v = rng.standard_normal(n) * float(rng.choice([1e-3, 1.0, 50.0, 1e6]))
    if kind == 1:
        v = np.floor(np.abs(v))
    elif kind == 2:
        v[rng.random(n) < 0.3] = 0.0
    elif kind == 3:
        v = np.array(GRID)[rng.integers(0, len(GRID), n)]
    return v


class RandomCase:
    """src, ast, cols {name: [64]}, and per item by the reference: ok, val, n_libm (libm-branch pow calls), sensitive"""


@functools.lru_cache(maxsize=None)
def random_cases(fe):
    rng = np.random.default_rng([_SEED, FRONT_ENDS.index(fe)])
    out = []
    while len(out) < N_RANDOM:
        names = NAMES[:int(rng.integers(1, 7))]
        c = RandomCase()
        c.src = gen(fe, rng, names)
        c.ast = fe.parse(c.src)
        c.cols = {nm: draw(rng, N_ITEMS) for nm in names}
        c.ok, c.val = np.zeros(N_ITEMS, dtype=bool), np.full(N_ITEMS, NAN)
        c.n_libm, c.sensitive = np.zeros(N_ITEMS, dtype=np.int64), np.zeros(N_ITEMS, dtype=bool)
        for i in range(N_ITEMS):
            env = c.env(i)
            c.ok[i], c.val[i], c.n_libm[i] = ref_item(fe, c.ast, env)
            if c.n_libm[i]:
                c.sensitive[i] = ulp_sensitive(fe, c.ast, env, c.ok[i], c.val[i], c.n_libm[i])
        out.append(c)
    return out


def _env(self, i):
    return {nm: float(v[i]) for nm, v in self.cols.items()}


RandomCase.env = _env


def random_census(fe):
    """(items, items in the exact class, items in the pow class, ulp-sensitive items) over the front end's random cases"""
    cs = random_cases(fe)
    total = sum(c.ok.size for c in cs)
    powc = sum(int(np.count_nonzero(c.n_libm)) for c in cs)
    return total, total - powc, powc, sum(int(np.count_nonzero(c.sensitive)) for c in cs)


# ---- programs at the compiler's limits: 32 stack slots (kMaxStack), 128 operations (kMaxProg) -----------------------------------
def nest_source(fe, k, constants=()):
    """v1 + (v2 + (… + vk)): k operands on the stack at once, the innermost on top; operand j in `constants` is the number j"""
    return "+(".join(str(j) if j in constants else fe.var("v%d" % j) for j in range(1, k + 1)) + ")" * (k - 1)


def chain_source(fe, k, negate_first=False):
    """v1 + v2 + … + vk: 2k - 1 operations; one more with a prefix minus on the first term (antlr, govaluate)"""
    return ("-" if negate_first else "") + "+".join(fe.var("v%d" % j) for j in range(1, k + 1))


def limit_values(k, n):
    """k distinct integer-valued variables over n items: every sum of them is exact, and every variable shows in it"""
    return {"v%d" % j: np.array([float(1000 * j + ((7 * i + j) % 911)) for i in range(n)]) for j in range(1, k + 1)}
