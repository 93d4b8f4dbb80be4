"""pg_index_refresh restated in numpy: the assignment rule (index_build.hip: assign_kernel, through the oracle's
fmaf chains), the index arrays the build's steps 3-5 give for a set of centroids and rows, and the matrix-pipe screen of
index_assign.hip with its bound e(x, L).  Shared by tests/test_index_refresh_cpu.py (the bound dominates |screen - rule| inside
its range, the survivor counts of the GPU tests' tables) and tests/test_gpu_index_refresh.py (the device's arrays equal the rule)."""
import numpy as np

from oracle import oracle as o

RANGE_LO, RANGE_HI = 2.0 ** -40, 2.0 ** 48          # ||.||^2 (fp32 chain) the bound is proven for
SLOTS = 4

# the tables tests/test_gpu_index_refresh.py refreshes on the matrix pipe: (seed, rows, dim, centres, sigma)
GPU_TABLES = ((31, 200_000, 64, 100, 0.1), (0x1F0128, 200_000, 128, 100, 0.1))


def default_lists(n):
    """pg_index_build's default list count"""
    return max(1, min(int(round(4.0 * np.sqrt(n))), 65536, n // 64))


def chain_norm2(v):
    """the k-ascending fp32 fmaf chain of v.v per row (cnorm2_kernel)"""
    v = np.ascontiguousarray(v, np.float32)
    out = np.empty(v.shape[0], np.float32)
    for a in range(0, v.shape[0], 2048):
        out[a:a + 2048] = np.diagonal(o.dot_scores(v[a:a + 2048], v[a:a + 2048]))
    return out


def rule_dist(rows, cent, cn2=None):
    """d[r][L] = fl(cn2[L] - 2 acc), acc the fmaf chain of x.c_L from 0"""
    cn2 = chain_norm2(cent) if cn2 is None else cn2
    with np.errstate(all="ignore"):
        return cn2[None, :] - np.float32(2.0) * o.dot_scores(cent, rows)


def rule_lists(rows, cent):
    """the rule's list of every row: smallest d, ties to the lower list, a row without a comparable distance to list 0"""
    cn2 = chain_norm2(cent)
    out = np.empty(rows.shape[0], np.uint32)
    for a in range(0, rows.shape[0], 16384):
        d = rule_dist(rows[a:a + 16384], cent, cn2)
        d = np.where(np.isnan(d), np.inf, d)             # (`d < best` is false for a NaN; +inf never beats the initial +inf)
        out[a:a + 16384] = np.argmin(d, axis=1)
    return out


def rule_index(rows, cent):
    """offsets, perm (ascending within a list) and the fp64 maximum distance of every list's rows for the rule's lists"""
    lists = rule_lists(rows, cent)
    nl = cent.shape[0]
    perm = np.argsort(lists, kind="stable").astype(np.uint32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(lists, minlength=nl))]).astype(np.uint32)
    with np.errstate(all="ignore"):
        dist = np.sqrt(np.sum((rows.astype(np.float64) - cent[lists].astype(np.float64)) ** 2, axis=1))
    far = np.zeros(nl, np.float64)
    np.fmax.at(far, lists, dist)                        # (fmax: a NaN row's distance does not count, as atomicMax of its bits ...)
    return lists, offsets, perm, far


# ---- the screen ------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16
    return b.astype(np.uint32).view(np.float32)


def split(x):
    hi = bf16_rne(x)
    return hi, bf16_rne(np.asarray(x, np.float32) - hi)


def screen_consts(dim):
    """A, B, eta of e(x, L) = A ||x|| ||c_L|| + B cn2[L] + eta (index_assign.hip: screen_bound_consts)"""
    u, d = 2.0 ** -24, float(dim)

    def gam(n):
        return n * u / (1 - n * u)
    E = gam(d) + 1.01 * gam(d + 2) + 2.0 ** -7 * gam(2 * d) + 3.02 * 2.0 ** -18
    return (np.float32((2 * E + 4.04 * u) * (1 + 2.0 ** -10)), np.float32(2 * u * (1 + 2.0 ** -10)), np.float32(2.0 ** -90))


def in_range(v):
    """per row: every element finite and the fp32 chain of ||v||^2 inside the range the bound is proven for"""
    v = np.ascontiguousarray(v, np.float32)
    with np.errstate(all="ignore"):
        n2 = chain_norm2(v)
    return np.all(np.isfinite(v), axis=1) & (n2 >= RANGE_LO) & (n2 <= RANGE_HI)


def bound(rows, cent, cn2=None, chain=True):
    """e[r][L], evaluated as the kernel does (fp32, ||x|| from the fp32 chain with its 2^-10 margin, ||c|| rounded up);
    chain=False: ||x||^2 summed in fp64 instead (2^-17 from the chain's, inside that margin; for large tables)"""
    A, B, eta = screen_consts(rows.shape[1])
    cn2 = chain_norm2(cent) if cn2 is None else cn2
    n2 = chain_norm2(rows) if chain else np.sum(rows.astype(np.float64) ** 2, axis=1).astype(np.float32)
    nx = np.sqrt(n2) * np.float32(1 + 2.0 ** -10)
    cn = np.sqrt(np.sum(cent.astype(np.float64) ** 2, axis=1)) * (1 + 2.0 ** -40)
    cnf = cn.astype(np.float32)
    cnf = np.where(cnf.astype(np.float64) < cn, np.nextafter(cnf, np.float32(np.inf)), cnf)
    return (A * nx)[:, None] * cnf[None, :] + (B * cn2 + eta)[None, :]


def screen_value(rows, cent, cn2=None):
    """s[r][L] = fl(cn2[L] - 2 fl(hh + cross)): the hi.hi products and the two cross products accumulated in fp32, one rounding
    per addition, k ascending (one admissible order of the MFMA's accumulation; the bound holds for every order)"""
    cn2 = chain_norm2(cent) if cn2 is None else cn2
    xh, xl = split(rows)
    ch, cl = split(cent)
    hh = np.zeros((rows.shape[0], cent.shape[0]), np.float32)
    cr = np.zeros_like(hh)
    for k in range(rows.shape[1]):
        hh = hh + xh[:, k:k + 1] * ch[None, :, k]
        cr = cr + xh[:, k:k + 1] * cl[None, :, k]
        cr = cr + xl[:, k:k + 1] * ch[None, :, k]
    return cn2[None, :] - np.float32(2.0) * (hh + cr)


def kmeans(rows, nl, iters, seed):
    """a few Lloyd iterations over a sample (fp32 matrix products: only the list count and the clustering matter here)"""
    rng = np.random.default_rng(seed)
    s = rows[rng.choice(rows.shape[0], min(rows.shape[0], 32 * nl), replace=False)]
    c = s[:nl].copy()
    for _ in range(iters):
        a = np.argmin(np.sum(c * c, axis=1)[None, :] - 2.0 * (s @ c.T), axis=1)
        cnt = np.bincount(a, minlength=nl)
        acc = np.zeros((nl, rows.shape[1]), np.float64)
        np.add.at(acc, a, s)
        c = np.where(cnt[:, None] > 0, acc / np.maximum(cnt, 1)[:, None], c).astype(np.float32)
    return c


def survivors_per_row(rows, cent):
    """lists the screen cannot discard, per row: those within the bound of the nearest one, the bound applied to both distances
    compared, d_L - e_L <= min_M (d_M + e_M) (d from fp32 matrix products: their error is far below e)"""
    cn2 = np.sum(cent.astype(np.float64) ** 2, axis=1).astype(np.float32)
    out = np.empty(rows.shape[0], np.int64)
    for a in range(0, rows.shape[0], 8192):
        x = rows[a:a + 8192]
        d = cn2[None, :] - 2.0 * (x @ cent.T)
        e = bound(x, cent, cn2, chain=False)
        out[a:a + 8192] = np.sum(d - e <= np.min(d + e, axis=1, keepdims=True), axis=1)
    return out
