"""numpy restatement of the bf16-shadow recall screen (csrc/recall.hip: screen_kernel with I8 = false, screen_prep_kernel,
screen_thr_kernel; csrc/recall_table.hip: table_shadow_kernel), read off the code, and the fixtures that the CPU tests
(test_screen_bf16_cpu.py) and the GPU tests (test_gpu_screen_bf16.py) share, so that both see the same bytes.

The screen keeps a (row, query) pair when !(acc < cut):

    acc  = sum_k bf16(x_k) bf16(q_k)                       v_mfma_f32_32x32x16_bf16, fp32 accumulation in the pipe's own order
    cut  = round_down(thr_screen_q - eps_unit_q * nb)      nb = max(sqrtf(blk_norm2[block]), 1e-16) * 1.0002f
    eps_unit_q = 0.008 ||q|| 1.0001 + 1e-30                (kScreenEps; ||q|| in fp64)
    thr_screen_q = thr_q, or -inf where the bound cannot be trusted (non-finite or huge magnitudes)

Every function is vectorised numpy; nothing here imports the GPU package."""
import numpy as np

F = np.float32
BLK = 32                            # kPieceRows
SCREEN_EPS = F(0.008)               # kScreenEps
NB_INFLATE = F(1.0002)
NORM_FLOOR = F(1e-16)               # kScreenNormFloor: the least block norm the cutoff is computed with
OUTLIER = 4.0e4                     # one element of this size sends a dim-128 table from the int8 to the bf16 shadow


def bf16_rne(x):
    """fp32 -> bf16, round to nearest even, as fp32 values.  NaN as screen_prep_kernel's rne (quiet bit set, payload cut); the
    table side (table_shadow_kernel) uses the hardware conversion, which agrees on every non-NaN value."""
    b = np.ascontiguousarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    r = np.where(nan, (b >> 16) | 0x40, r)
    return (r.astype(np.uint32) << np.uint32(16)).view(F)


def blocks_of(rows):
    return (rows + BLK - 1) // BLK


def blk_norm2(tab):
    """The largest row sum of squares of every 32-row block, as fp32.  The squares are fp32 products (so they underflow where the
    device's do); their sum is taken in fp64 and then put at the LOW end of what an fp32 sum in any order can give (relative
    1e-5 >= (dim + 1) 2^-24 at dim 128), so that an inequality shown with this value holds for the device's."""
    x = np.ascontiguousarray(tab, dtype=F)
    ss = (x * x).astype(np.float64).sum(axis=1)
    nb = blocks_of(len(x))
    pad = np.zeros(nb * BLK)
    pad[:len(x)] = ss
    return (pad.reshape(nb, BLK).max(axis=1) * (1.0 - 1e-5)).astype(F)


def max_norm_of(norm2):
    """TableDerived::max_norm: sqrtf(largest row sum of squares) * 1.0001f"""
    m = F(norm2.max()) if norm2.size else F(0)
    return F(np.sqrt(m, dtype=F) * F(1.0001))


def eps_unit(q):
    """screen_prep_kernel: (float)(sqrt(sum q^2) * (double)kScreenEps * 1.0001) + 1e-30f, the sum in fp64"""
    q = np.atleast_2d(np.asarray(q, dtype=F))
    with np.errstate(over="ignore", invalid="ignore"):
        ss = (q.astype(np.float64) ** 2).sum(axis=1)
        e = (np.sqrt(ss) * float(SCREEN_EPS) * 1.0001).astype(F)
        return (e + F(1e-30)).astype(F)


def stands_aside(thr, eps, max_norm):
    """screen_thr_kernel's four conditions: e is NaN, e > 1e28, thr is NaN, !(e * max_norm < 1e35) (an fp32 product)"""
    thr, eps = np.asarray(thr, dtype=F), np.asarray(eps, dtype=F)
    with np.errstate(over="ignore", invalid="ignore"):
        prod = (eps * F(max_norm)).astype(F)
    return np.isnan(eps) | (eps > F(1e28)) | np.isnan(thr) | ~(prod < F(1e35))


def thr_screen(thr, eps, max_norm):
    return np.where(stands_aside(thr, eps, max_norm), F(-np.inf), np.asarray(thr, dtype=F)).astype(F)


def norm_used(norm2, floor=True):
    """nb = fmaxf(sqrtf(blk_norm2), kScreenNormFloor) * 1.0002f.  floor=False is the rule without the floor: like the neighbour-norm
    variants below it exists only to prove a fixture sharp."""
    n = np.sqrt(np.asarray(norm2, dtype=F), dtype=F)
    return ((np.maximum(n, NORM_FLOOR) if floor else n) * NB_INFLATE).astype(F)


def cut_of(thr_s, eu, norm2, floor=True):
    """The cutoff of one query for every block: v = fmaf(-eu, nb, thr_s); cut = v - fmaf(min(|v|, 3e38), 1.2e-7, 1e-37).
    (The fma is taken in fp64 and rounded once: the product of two fp32 values is exact there.)"""
    with np.errstate(over="ignore", invalid="ignore"):
        nb = norm_used(norm2, floor)
        v = (float(thr_s) - float(eu) * nb.astype(np.float64)).astype(F)
        down = (np.minimum(np.abs(v), F(3.0e38)).astype(np.float64) * float(F(1.2e-7)) + float(F(1e-37))).astype(F)
        return (v - down).astype(F)


def block_norm_used(norm2, variant=0):
    """variant 0: every block's own norm — the kernel's rule.  variant -1 / +1: the norm of block b - 1 / b + 1 (the edge block keeps
    its own).  The variants are index slips nobody should ship; they exist to prove a fixture sharp."""
    if variant == 0:
        return norm2
    idx = np.clip(np.arange(len(norm2)) + variant, 0, len(norm2) - 1)
    return norm2[idx]


def acc_f64(xh, qh):
    """x^ . q^ of every row for one query, in fp64 (x^, q^ the bf16 values)"""
    return xh.astype(np.float64) @ qh.astype(np.float64)


def keep(acc, thr_s, eu, norm2, variant=0, floor=True):
    """The keep rule !(acc < cut) for every row against one query; acc as the fp32 the pipe hands over"""
    cut = np.repeat(cut_of(thr_s, eu, block_norm_used(norm2, variant), floor), BLK)[:len(acc)]
    with np.errstate(over="ignore", invalid="ignore"):
        return ~(np.asarray(acc).astype(F) < cut)


def gamma(d):
    """the relative error of an fp32 sum of d terms in any order"""
    u = d * 2.0 ** -24
    return u / (1.0 - u)


def grow_schedule(rows, k, growth=2.0):
    """[begin, end) rows of the growing-chunk plan's launches (next_chunk_blocks, recall_plan_math.hpp): the first chunk goes
    through the exact scan, every later one is screened against the K-th best score of the rows before it"""
    nb, out, rb = blocks_of(rows), [], 0
    while rb < nb:
        if rb == 0:
            c = 1
            while c < 8 * k:
                c <<= 1
            c = max(c, 2048)
            if c > 32768 or c < k:
                c = 32768
        else:
            c = int(rb * BLK * (growth - 1.0))
        cb = min(c // BLK, nb - rb)
        out.append((rb * BLK, min((rb + cb) * BLK, rows)))
        rb += cb
    return out


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _loud_rows(rng, n, norm, along, u, away):
    """n rows of the given norm orthogonal to every direction of `away` (orthonormal rows, fp64), plus u along `along`"""
    w = rng.standard_normal((n, away.shape[1]))
    w -= (w @ away.T) @ away
    return norm * _unit(w) + np.asarray(u)[:, None] * along[None, :]


class Sharp:
    """Fixture (a): block norms that differ.  Blocks b = 0, 1 (mod 3) are loud, b = 2 (mod 3) quiet (1e-3 N(0, I)).  A loud block's rows
    have norm 10, 100 or 1000 (drawn per block) orthogonal to both sharp queries, plus U(0, 0.2) along the unit vector of the block's
    own sharp query: q[0] for b = 0, q[1] for b = 1 (mod 3).  The K = 300 best rows of a sharp query all sit in its loud blocks, within
    0.003 ||q|| of the K-th score, where the bf16 error of a norm-1000 row is ~0.2 ||q||: only the block's own norm keeps them.  A
    sharp query's loud blocks have a quiet neighbour on one side and a loud block of an unrelated norm on the other.  The other
    queries are Gaussian.  last_member: the table's last row scores highest for the sharp query that owns the last block (last_owner)."""
    K = 300
    SHARP = (0, 1)

    def __init__(self, dim, rows=64_000, seed=7, nq=256, outlier=None, last_member=True):
        rng = np.random.default_rng(1000 * seed + dim)
        nb = blocks_of(rows)
        q = rng.standard_normal((nq, dim))
        q[1] -= (q[1] @ q[0]) / (q[0] @ q[0]) * q[0]
        away = np.stack([_unit(q[0]), _unit(q[1])])
        tab = 1e-3 * rng.standard_normal((nb * BLK, dim))
        self.block_norm = np.zeros(nb)
        for b in range(nb):
            if b % 3 == 2:
                continue
            self.block_norm[b] = 10.0 ** rng.integers(1, 4)
            tab[b * BLK:(b + 1) * BLK] = _loud_rows(rng, BLK, self.block_norm[b], away[b % 3], rng.uniform(0.0, 0.2, BLK), away)
        if last_member:
            self.last_owner = (nb - 1) % 3
            assert self.last_owner != 2, "the last block must be a loud one"
            tab[rows - 1] = _loud_rows(rng, 1, self.block_norm[nb - 1], away[self.last_owner], [0.25], away)[0]
        if outlier is None:
            outlier = dim == 128
        self.outlier_row = None
        if outlier:
            # (row 5 of block 0: one element of 4e4, orthogonal to the sharp queries like every loud row)
            e = np.zeros(dim)
            e[17] = OUTLIER
            tab[5] = e - (e @ away.T) @ away
            self.outlier_row = 5
        self.dim, self.rows = dim, rows
        self.tab = np.ascontiguousarray(tab[:rows], dtype=F)
        self.q = np.ascontiguousarray(q, dtype=F)
        # a flag column that admits every other loud block (fixture h)
        blk = np.arange(rows) // BLK
        self.flag = ((blk % 3 != 2) & ((blk // 3) % 2 == 0)).astype(np.int32)

    def loud_row(self, seed, norm, u, sharp=0):
        """one more loud row for sharp query `sharp`, with u along its unit vector (fixture c)"""
        rng = np.random.default_rng(seed)
        q = self.q.astype(np.float64)
        away = np.stack([_unit(q[0]), _unit(q[1])])
        return _loud_rows(rng, 1, norm, away[sharp], [u], away)[0].astype(F)


def ragged_rows(tail):
    """fixture (b): 1998 whole blocks and a last one of `tail` rows (32: whole); block 1998 is one of q[0]'s"""
    return 1998 * BLK + tail


PLANT_ROWS = 40_000


def planted(dim):
    """Fixture (d), the construction of test_gpu_screen_wide.planted() on a bf16 table: for each of 256 queries j a planted row
    1.5-1.8 x q[j] sits at each of the 32 positions p of a block.  dim 128: q[:, 0] > 0 for every query and one row holds -4e4 in
    column 0 (it leaves the int8 shadow and scores below everything)."""
    rng = np.random.default_rng(1601 + dim)
    tab = _unit(rng.uniform(-1, 1, (PLANT_ROWS, dim))).astype(F)
    q = _unit(rng.uniform(-1, 1, (256, dim))).astype(F)
    if dim == 128:
        q[:, 0] = np.abs(q[:, 0]) + F(1e-3)
    plants = []
    for j in range(256):
        for p in range(BLK):
            r = ((7 * j + 41 * p) % (PLANT_ROWS // BLK)) * BLK + p
            tab[r] = q[j] * F(1.5 + 0.01 * p)
            plants.append((j, r))
    if dim == 128:
        taken = {r for _, r in plants}
        r = next(r for r in range(100, PLANT_ROWS) if r not in taken)
        tab[r, 0] = F(-OUTLIER)
    return tab, q, plants


TINY_SHARP = 4                      # the query of hostile() that meets the 1e-32 rows right at its K-th score


def hostile(dim, nq):
    """Fixture (f): 60 003 rows of 0.05 N(0, I) whose column 1 is made >= 0.05, with
      rows 5000-5399   near-duplicates of one row, 1e-6 relative apart (below bf16 resolution); q[2] along them, q[3] against
      rows 7000-7063   exact copies of rows 8000-8063 (ties by row)
      rows 3008-3103   zero rows; -0.0 components in rows 9000-9031
      rows 2016-2655   scaled by 1e-30 (twenty whole blocks: their fp32 sums of squares underflow to zero)
      rows 1024-1273   v0 = g (1 - 2^-11) in column 1 and zeros elsewhere, g the bf16 nearest 1e-32: v0 rounds UP to g in bf16
      rows 50016-50079 (two whole blocks) the same with column 1 a few ulps below v0: still g in bf16
      q[0] zero, q[1] one dominant component (the outlier's column at dim 128); q[4] = -e_1: every ordinary row scores below
      -0.05, the zero rows 0, the v0 rows -v0 exactly (250 ties) and the late rows a little above that — they are members, the
      K-th score stays -v0, and their bf16 scores are -g, 5e-4 relative BELOW it: only a margin keeps them, and their blocks'
      fp32 sums of squares are zero.  Under the growing-chunk plan the late rows are screened against exactly -v0.
      q[7], q[10] = -e_1 + noise; every third of the other queries is against a row."""
    rng = np.random.default_rng(23 + dim)
    n = 60_003
    tab = (rng.standard_normal((n, dim)) * 0.05).astype(F)
    tab[:, 1] = np.abs(tab[:, 1]) + F(0.05)
    near = tab[5000].copy()
    tab[5000:5400] = near * (F(1.0) + F(1e-6) * np.arange(400, dtype=F)[:, None])
    tab[7000:7064] = tab[8000:8064]
    tab[3008:3104] = 0.0
    tab[9000:9032, ::5] = F(-0.0)
    tab[2016:2656] *= F(1e-30)
    g = bf16_rne(np.array([1e-32], dtype=F))[0]
    v0 = F(g * F(1.0 - 2.0 ** -11))
    late = (np.array([v0]).view(np.uint32)[0] - np.uint32(4) * np.arange(1, 65, dtype=np.uint32)).view(F)
    assert float(v0) == float(g) * (1.0 - 2.0 ** -11) and np.all(bf16_rne(np.append(late, v0)) == g) and np.all(late < v0)
    tab[1024:1274] = 0.0
    tab[1024:1274, 1] = v0
    tab[50_016:50_080] = 0.0
    tab[50_016:50_080, 1] = late
    if dim == 128:
        tab[1234, 17] = F(OUTLIER)
    q = rng.standard_normal((nq, dim)).astype(F)
    q[5::3] = -tab[rng.integers(10_000, 50_000, len(q[5::3]))] + F(0.01) * q[5::3]      # negative best scores are rare; these lean against a row
    q[0] = 0.0
    q[1] = 0.0
    q[1, 17] = 1.0
    q[2] = near
    q[3] = -near
    for i in (7, 10):
        q[i] = F(0.001) * q[i]
        q[i, 1] = -1.0
    q[TINY_SHARP] = 0.0
    q[TINY_SHARP, 1] = -1.0
    return tab, q


GUARD_ROWS = 40_000


def guard_tables(dim):
    """Fixture (g): (unit-norm rows, the same with one row of norm 1e10 in every fifth block — which leaves the int8 shadow by
    itself), and for each the queries: ordinary
    ones with, at 3 and 9, the largest norm the guards of screen_thr_kernel still screen and, at 6 and 12, twice that."""
    rng = np.random.default_rng(77 + dim)
    unit = _unit(rng.standard_normal((GUARD_ROWS, dim))).astype(F)
    big = unit.copy()
    if dim == 128:
        unit[1234, 17] = F(OUTLIER)              # (leaves the int8 shadow; eps_unit x max_norm = 3.2e32 stays far from its guard)
    big[7::5 * BLK] *= F(1e10)
    out = []
    for tab, active, aside in ((unit, 1e30, 2e30), (big, 1e27, 2e27)):
        q = rng.standard_normal((16, dim))
        for i, s in ((3, active), (9, active), (6, aside), (12, aside)):
            q[i] = _unit(q[i]) * s
        out.append((tab, q.astype(F), (3, 9), (6, 12)))
    return out


SUBNORMAL_ROWS = 20_000
SUBNORMAL_M = {"subnormal": 11, "smallest_normal": 130}      # 11 x 2^-133 = 1.01e-39 (fp32 subnormal), 130 x 2^-133 = 1.19e-38 (normal)


def subnormal(dim, m):
    """Fixture (i): 0.05 N(0, I) rows whose column 0 is >= 0.05, and rows that hold one tiny component in column 0 and zeros elsewhere.
    In units of 2^-149, the fp32 subnormal step: rows 100-115 hold -(65536 m + 20000), rows 16000-16031 (block 500) hold
    -(65536 m + 20000 + j), j = 1 .. 32.  A bf16 keeps multiples of 2^-133 = 65536 units there, so every one of them rounds to
    -65536 m: an absolute error of 2^-134, 3 % at m = 11, where the bound counts on a relative 2^-9.  Query 0 is -2^90 e_0
    (exact in bf16): those 48 rows' scores are the only positive ones, all exact, and the K = 16 best are rows 16016-16031.
    Under the growing-chunk plan block 500 is screened against the score of rows 100-115 — which its own bf16 scores do not
    reach.  The fp32 sum of squares of the block is zero.  The other queries are Gaussian."""
    rng = np.random.default_rng(55 + dim)
    tab = (rng.standard_normal((SUBNORMAL_ROWS, dim)) * 0.05).astype(F)
    tab[:, 0] = np.abs(tab[:, 0]) + F(0.05)
    unit = 2.0 ** -149
    base = 65536 * m + 20000
    tab[100:116] = 0.0
    tab[100:116, 0] = F(-base * unit)
    tab[16000:16032] = 0.0
    tab[16000:16032, 0] = (-(base + np.arange(1, 33)) * unit).astype(F)
    if dim == 128:
        tab[1234, 17] = F(OUTLIER)
    q = rng.standard_normal((8, dim)).astype(F)
    q[0] = 0.0
    q[0, 0] = F(-2.0 ** 90)
    return tab, q
