"""numpy restatement of what the table pass derives from a table's rows (recall_table.hip, recall_i4.hip, recall_r2.hip; read back
through pg_table_derived_info / pg_table_derived_read), in two layers:

  exact layer   np.float32 in the kernels' operation order (the library is built with -ffp-contract=off, so numpy's fp32
                multiply, divide and rint agree with the device): the scales, every shadow, |x|^2 and its block minima
  bound layer   np.float64 from the arrays the DEVICE returned: the claim under test is "the number bounds the error of the
                shadow that is actually streamed"

check(table, info, arrays) holds every comparison; the GPU tests (test_gpu_table_derived.py) and the CPU sensitivity test
(test_table_derived_ref_cpu.py) both call it.  model(table) is a numpy stand-in for the device (exact layer + the padded bounds),
used by the sensitivity test as the answer that check must accept, and as the base of its mutations."""
import numpy as np

from oracle import oracle as o

PAD = 64                    # padding rows behind every per-row array
BLK = 32                    # rows per block (kPieceRows)
SCREEN_EPS = 0.008          # kScreenEps: the int8 / bf16 routing rule of ensure_table_stats
PRED_WORDS = 128 + 128 * 128 + 10
F = np.float32
ARRAYS = ("i8", "bf16", "blknorm2", "i4", "i4s", "i8r", "nx", "nxmin", "pred")
STATS, I4, R2, NX, PRED = 1, 2, 4, 8, 16
ALL = 31

# tightness caps (the issue's table): value <= mul x fp64 value + add x N, N the fp64 max norm (R_r: + 1e-29 absolute)
CAPS = {"max_norm": (1.0002, 0.0), "resid8": (1.01, 2e-6), "dnorm2": (1.0 + 1e-5, 0.0), "R_r": (1.02, 1e-29),
        "rmax4": (1.001, 2e-6), "resid2": (1.02, 2e-7)}


# ---- exact layer ------------------------------------------------------------------------------------------------
def bf16_up(f):
    """the smallest bf16 value >= f (f finite, >= 0), as fp32"""
    b = np.asarray(f, F).view(np.uint32).astype(np.uint64)
    r = np.where(b & 0xffff, (b | 0xffff) + 1, b)
    return r.astype(np.uint32).view(F)


def bf16_nearest(f):
    return o.f32_to_bf16_round(np.asarray(f, F))


def scale8(x):
    amax = F(np.max(np.abs(x))) if x.size else F(0)
    return np.maximum(amax / F(127.0), F(1e-30)).astype(F)


def quant(x, s, lim):
    """clip(rint(x * (1 / s)), +-lim) in fp32; s a scalar or a column of row scales"""
    inv = (F(1.0) / np.asarray(s, F)).astype(F)
    return np.clip(np.rint((x * inv).astype(F)), -lim, lim).astype(np.int32)


def fma_resid(x, s, X):
    """fmaf(-s, X, x): the product of a 24-bit and a 7-bit number and its difference from x are exact in fp64"""
    return (x.astype(np.float64) - np.asarray(s, F).astype(np.float64) * X.astype(np.float64)).astype(F)


def row_scale4(x):
    amax = np.max(np.abs(x), axis=1).astype(F)
    return bf16_up(np.maximum(amax / F(7.0), F(1e-30)).astype(F))


def pack4(X4):
    """[rows][128] in [-7, 7] -> [rows][16] u32: byte b of dword w holds dims 8w + b (low nibble) and 8w + 4 + b (high nibble)"""
    v = (X4 + 8).astype(np.uint32).reshape(X4.shape[0], 16, 8)
    w = np.zeros(v.shape[:2], np.uint32)
    for i in range(8):
        w |= v[:, :, i] << np.uint32(8 * (i & 3) + 4 * (i >> 2))
    return w


def unpack4(words, nrows):
    b = np.ascontiguousarray(words, np.uint32).reshape(nrows, 16).view(np.uint8).reshape(nrows, 16, 4)
    return np.concatenate([(b & 15).astype(np.int32) - 8, (b >> 4).astype(np.int32) - 8], axis=2).reshape(nrows, 128)


def nxmin_of(nx, rows):
    """min over the block's rows inside the table, 0 where that is NaN (a NaN norm: no help from this block)"""
    nb = (rows + BLK - 1) // BLK
    v = np.full(nb * BLK, np.inf, F)
    v[:rows] = nx[:rows]
    with np.errstate(invalid="ignore"):
        m = np.min(v.reshape(nb, BLK), axis=1)          # (np.min hands a NaN on)
    return np.where(np.isnan(m), F(0), m).astype(F)


def pred_sample_rows(rows):
    n = min(rows, 1 << 20)
    stride = rows // n
    return n, stride, np.minimum(np.arange(n, dtype=np.int64) * stride, rows - 1)


def is_finite_table(x):
    with np.errstate(over="ignore", invalid="ignore"):
        ss = np.sum(x.astype(np.float64) ** 2, axis=1)
    return bool(np.all(ss < 3.0e38))                    # (NaN compares false)


def route(x):
    """which main shadow ensure_table_stats chooses: 0 none, 1 int8, 2 bf16; None where the rule is within 1e-3 of its
    threshold (its fp32 sum of squares is an atomic sum: either side is right there)"""
    rows, dim = x.shape
    if dim not in (64, 128) or not is_finite_table(x):
        return 0
    if dim == 64:
        return 2
    rms = np.sqrt(np.sum(x.astype(np.float64) ** 2) / rows)
    ratio = float(scale8(x)) * np.sqrt(dim / 12.0) / max(4.0 * SCREEN_EPS * rms, 1e-300)
    return 2 if ratio > 1.001 else (1 if ratio < 0.999 else None)


def padded(a, fill=0):
    out = np.full((a.shape[0] + PAD,) + a.shape[1:], fill, a.dtype)
    out[:a.shape[0]] = a
    return out


# ---- a numpy stand-in for the device ------------------------------------------------------------------------------
def _max_without(v, leave_out):
    v = np.asarray(v, np.float64)
    if leave_out and v.size > 1:
        v = np.delete(v, int(np.argmax(v)))
    return float(np.max(v)) if v.size else 0.0


def model(table, leave_out=None):
    """(info, arrays) as a device that computes the exact layer and the documented padded bounds would answer.  leave_out names
    one maximum ("absmax", "max_norm", "resid8", "rmax4", "resid2") from which the row that decides it is left out."""
    x = np.ascontiguousarray(table, F)
    rows, dim = x.shape
    x64 = x.astype(np.float64)
    info = {k: 0 for k in ("elem_bytes", "all_finite", "i4_ok", "r2_ok", "nx_valid", "pred_model", "pred_n_sample", "pred_stride")}
    info.update({k: 0.0 for k in ("max_norm", "s8", "resid8", "rho4", "rmax4", "lam4", "s8r", "resid2", "l2_slack")})
    arr = {}
    fin = is_finite_table(x)
    info["all_finite"] = int(fin and dim in (64, 128))
    if dim in (64, 128):
        nx = o.row_norm2(x)
        arr["nx"] = padded(nx)
        arr["nxmin"] = nxmin_of(nx, rows)
        info["nx_valid"] = 1
        info["l2_slack"] = float(F(l2_slack_ref(arr["nx"], arr["nxmin"], rows, dim)))
    if not fin or dim not in (64, 128):
        return info, arr
    norm = np.sqrt(np.sum(x64 ** 2, axis=1))
    info["max_norm"] = float(F(F(_max_without(norm, leave_out == "max_norm")) * F(1.0001)))
    N = F(info["max_norm"])
    eb = route(x) or 1
    info["elem_bytes"] = eb
    if eb == 1:
        xs = x
        if leave_out == "absmax":
            xs = np.delete(x, int(np.argmax(np.max(np.abs(x), axis=1))), axis=0)
        s8 = scale8(xs)
        X8 = quant(x, s8, 127)
        r = fma_resid(x, s8, X8)
        res = np.sqrt(np.sum(r.astype(np.float64) ** 2, axis=1))
        info["s8"] = float(s8)
        info["resid8"] = float(F(F(_max_without(res, leave_out == "resid8")) * F(1.001) + F(1e-6) * N))
        arr["i8"] = padded(X8.astype(np.int8)).reshape(-1)
    else:
        arr["bf16"] = padded((bf16_nearest(x).view(np.uint32) >> 16).astype(np.uint16)).reshape(-1)
        nb = (rows + BLK - 1) // BLK
        n2 = np.zeros(nb * BLK)
        n2[:rows] = norm ** 2
        arr["blknorm2"] = np.max(n2.reshape(nb, BLK), axis=1).astype(F)
        arr["blknorm2"] = np.nextafter(arr["blknorm2"], F(np.inf))          # (rounded to nearest above: never below the fp64 value)
    if dim != 128:
        return info, arr
    s_r = row_scale4(x)
    X4 = quant(x, s_r[:, None], 7)
    r4 = fma_resid(x, s_r[:, None], X4)
    res4 = np.sqrt(np.sum(r4.astype(np.float64) ** 2, axis=1))
    R = bf16_up((res4.astype(F) * F(1.001) + F(1e-30)).astype(F))
    arr["i4"] = padded(pack4(X4), 0x88888888).reshape(-1)
    arr["i4s"] = padded((s_r.view(np.uint32) >> 16) | (R.view(np.uint32) & np.uint32(0xffff0000)))
    info["i4_ok"] = 1
    info["rmax4"] = float(F(F(_max_without(R, leave_out == "rmax4")) * F(1.000001) + F(1e-6) * N))
    info["rho4"], info["lam4"] = (float(F(v)) for v in i4_stats_ref(x64, s_r, X4, R))
    if eb != 1:
        return info, arr
    s8r = (s8 / F(254.0)).astype(F)
    Xr = quant(r, s8r, 127)
    e2 = fma_resid(r, s8r, Xr)
    res2 = np.sqrt(np.sum(e2.astype(np.float64) ** 2, axis=1))
    arr["i8r"] = padded(Xr.astype(np.int8)).reshape(-1)
    info["r2_ok"] = 1
    info["s8r"] = float(s8r)
    info["resid2"] = float(F(F(_max_without(res2, leave_out == "resid2")) * F(1.01) + F(1e-7) * N))
    n, stride, srows = pred_sample_rows(rows)
    mean, cov = pred_ref(x64[srows])
    words = np.zeros(PRED_WORDS, np.uint32)
    words[:128] = mean.astype(F).view(np.uint32)
    words[128:128 + 128 * 128] = cov.astype(F).reshape(-1).view(np.uint32)
    words[128 + 128 * 128:].view(np.float64)[3] = 1e300
    arr["pred"] = words
    info.update(pred_model=1, pred_n_sample=n, pred_stride=stride)
    return info, arr


# ---- statistics in fp64 -------------------------------------------------------------------------------------------
def l2_slack_ref(nx_dev, nxmin_dev, rows, dim):
    nx = np.asarray(nx_dev[:rows], np.float64)
    m = np.repeat(np.asarray(nxmin_dev, np.float64), BLK)[:rows]
    with np.errstate(invalid="ignore"):
        ok = (nx == nx) & (nx < 1e30)
    total = float(np.sum(nx[ok]))
    if not total > 0.0:
        return 0.0
    slack = float(np.sum(nx[ok] - m[ok]))
    return (slack / rows) * 0.5 / ((total / rows) / np.sqrt(dim))


def i4_stats_ref(x64, s_r, X4, R):
    """(rho4, lam4) from the scales, nibbles and residual bounds given"""
    rows = x64.shape[0]
    s = s_r.astype(np.float64)
    res2 = np.sum((x64 - s[:, None] * X4) ** 2, axis=1)
    rho2 = np.where(s > 1e-18, res2 / (s * s * 128.0), 0.0)
    ss = np.sum(x64 ** 2, axis=1)
    cnt = ss.astype(F) > 0                                   # (the kernel's fp32 sum of squares: tiny rows underflow to 0 and do not count)
    lam = float(np.sum(R.astype(np.float64)[cnt] / np.sqrt(ss[cnt]))) / rows * np.sqrt(128.0)
    return float(np.sqrt(np.max(rho2))) if rows else 0.0, lam


def pred_ref(xs64):
    n = xs64.shape[0]
    mean = np.sum(xs64, axis=0) / n
    return mean, xs64.T @ xs64 / n - np.outer(mean, mean)


# ---- the comparisons ----------------------------------------------------------------------------------------------
def _bits(v):
    return int(np.asarray(v, F).view(np.uint32))


def _first_diff(f, name, got, want, ncols=1):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.shape != want.shape:
        f.append("%s: %d elements, expected %d" % (name, got.size, want.size))
        return
    both_nan = False
    if got.dtype.kind == "f":
        both_nan = np.isnan(got) & np.isnan(want)           # (a NaN's sign and payload are nobody's specification)
        got, want = got.view(np.uint32), want.view(np.uint32)
    bad = np.flatnonzero((got != want) & ~both_nan)
    if bad.size:
        i = int(bad[0])
        f.append("%s differs at row %d column %d: device %r, expected %r (%d elements differ)"
                 % (name, i // ncols, i % ncols, got[i], want[i], bad.size))


def _upper(f, name, got, exact, cap, N, where=""):
    """soundness with no slack, tightness against the cap; returns got / fp64 value (what the cap's factor limits)"""
    mul, add = CAPS[cap]
    lim = mul * exact + (add if cap == "R_r" else add * N)
    if not got >= exact:
        f.append("%s%s = %.9g is BELOW the fp64 value %.9g: not an upper bound" % (name, where, got, exact))
    if not got <= lim:
        f.append("%s%s = %.9g exceeds its cap %.9g (fp64 value %.9g)" % (name, where, got, lim, exact))
    return got / exact if exact > 0 else 0.0


def check(table, info, arrays, parts=ALL, ratios=None):
    """every comparison of a device answer (info: pg_table_derived_info's dict, arrays: name -> pg_table_derived_read's full
    array, padding included; an array that is not built is absent) with the restatement -> list of findings (strings; empty:
    all is well).  `parts`: what info was asked to build.  `ratios` (a dict) collects, per tightness cap, the largest value / fp64
    value seen (R_r: over the rows whose residual is above 1e-20, where the cap's absolute term plays no part)."""
    f = []
    x = np.ascontiguousarray(table, F)
    rows, dim = x.shape
    x64 = x.astype(np.float64)
    ratios = {} if ratios is None else ratios

    def note(cap, r):
        ratios[cap] = max(ratios.get(cap, 0.0), float(r))

    def need(name, n):
        a = arrays.get(name)
        if a is None:
            f.append("array %s is not built" % name)
        elif a.size != n:
            f.append("array %s: %d elements, expected %d" % (name, a.size, n))
            a = None
        return a

    fin = is_finite_table(x)
    want_eb = route(x)
    eb = info["elem_bytes"]
    if want_eb is not None and eb != want_eb:
        f.append("elem_bytes = %d, expected %d" % (eb, want_eb))
    if info["all_finite"] != int(fin and dim in (64, 128)):
        f.append("all_finite = %d, expected %d" % (info["all_finite"], int(fin and dim in (64, 128))))
    for name, have in (("i8", eb == 1), ("bf16", eb == 2), ("blknorm2", eb == 2)):
        if not have and name in arrays:
            f.append("array %s is built but elem_bytes = %d" % (name, eb))
    with np.errstate(over="ignore", invalid="ignore"):
        norm = np.sqrt(np.sum(x64 ** 2, axis=1))
    N = float(np.max(norm)) if fin else 0.0

    # -- |x|^2 and its block minima: built for non-finite tables too
    if parts & NX:
        if info["nx_valid"] != int(dim in (64, 128)):
            f.append("nx_valid = %d, expected %d" % (info["nx_valid"], int(dim in (64, 128))))
        if info["nx_valid"]:
            nx, nxmin = need("nx", rows + PAD), need("nxmin", (rows + BLK - 1) // BLK)
            if nx is not None:
                _first_diff(f, "nx", nx, padded(o.row_norm2(x)))
            if nx is not None and nxmin is not None:
                _first_diff(f, "nxmin", nxmin, nxmin_of(nx, rows))
                want = l2_slack_ref(nx, nxmin, rows, dim)
                if not np.isfinite(info["l2_slack"]) or abs(info["l2_slack"] - want) > 1e-3 * abs(want) + 1e-30:
                    f.append("l2_slack = %.9g, fp64 %.9g" % (info["l2_slack"], want))
    if eb == 0:
        for k in ("i4_ok", "r2_ok", "pred_model"):
            if info[k]:
                f.append("%s is set on a table without a main shadow" % k)
        return f

    # -- the main shadow and its statistics
    note("max_norm", _upper(f, "max_norm", info["max_norm"], N, "max_norm", N))
    s8 = None
    if eb == 1:
        s8 = scale8(x)
        if _bits(info["s8"]) != _bits(s8):
            f.append("s8 = %.9g (0x%08x), expected %.9g (0x%08x)" % (info["s8"], _bits(info["s8"]), s8, _bits(s8)))
        d8 = need("i8", (rows + PAD) * dim)
        if d8 is not None:
            d8 = d8.reshape(rows + PAD, dim)
            _first_diff(f, "X8", d8[:rows], quant(x, s8, 127).astype(np.int8), dim)
            _first_diff(f, "X8 padding", d8[rows:], np.zeros((PAD, dim), np.int8), dim)
            res = np.sqrt(np.sum((x64 - float(F(info["s8"])) * d8[:rows].astype(np.float64)) ** 2, axis=1))
            note("resid8", _upper(f, "resid8", info["resid8"], float(np.max(res)), "resid8", N, " (row %d)" % int(np.argmax(res))))
    else:
        d16 = need("bf16", (rows + PAD) * dim)
        if d16 is not None:
            d16 = d16.reshape(rows + PAD, dim)
            _first_diff(f, "bf16 shadow", d16[:rows], (bf16_nearest(x).view(np.uint32) >> 16).astype(np.uint16), dim)
            _first_diff(f, "bf16 padding", d16[rows:], np.zeros((PAD, dim), np.uint16), dim)
        bn = need("blknorm2", (rows + BLK - 1) // BLK)
        if bn is not None:
            used = np.repeat((np.sqrt(bn.astype(F)) * F(1.0002)).astype(np.float64), BLK)[:rows]   # (as the screen uses the value)
            bad = np.flatnonzero(~(used >= norm))
            if bad.size:
                r = int(bad[0])
                f.append("sqrt(dnorm2[%d]) * 1.0002 = %.9g is BELOW ||x|| = %.9g of row %d" % (r // BLK, used[r], norm[r], r))
            n2 = np.zeros(bn.size * BLK)
            n2[:rows] = norm ** 2
            top = np.max(n2.reshape(-1, BLK), axis=1)
            lim = CAPS["dnorm2"][0] * top
            bad = np.flatnonzero(~(bn.astype(np.float64) <= lim))
            if bad.size:
                b = int(bad[0])
                f.append("dnorm2[%d] = %.9g exceeds its cap %.9g" % (b, bn[b], lim[b]))
            with np.errstate(divide="ignore", invalid="ignore"):
                note("dnorm2", np.nanmax(np.where(top > 0, bn / top, 0.0)))

    # -- the 4-bit shadow
    if parts & I4:
        if info["i4_ok"] != int(dim == 128):
            f.append("i4_ok = %d, expected %d" % (info["i4_ok"], int(dim == 128)))
        d4, d4s = (need("i4", (rows + PAD) * 16), need("i4s", rows + PAD)) if info["i4_ok"] else (None, None)
        if d4 is not None and d4s is not None:
            s_r = row_scale4(x)
            X4 = quant(x, s_r[:, None], 7)
            d4 = d4.reshape(rows + PAD, 16)
            _first_diff(f, "s_r (bf16 bits)", d4s[:rows] & 0xffff, s_r.view(np.uint32) >> 16)
            _first_diff(f, "nibbles", unpack4(d4[:rows], rows), X4, 128)
            _first_diff(f, "nibble padding", d4[rows:], np.full((PAD, 16), 0x88888888, np.uint32), 16)
            _first_diff(f, "scale word padding", d4s[rows:], np.zeros(PAD, np.uint32))
            s_dev = ((d4s[:rows] & 0xffff) << 16).astype(np.uint32).view(F)
            R = (d4s[:rows] & np.uint32(0xffff0000)).view(F)
            X_dev = unpack4(d4[:rows], rows)
            res4 = np.sqrt(np.sum((x64 - s_dev.astype(np.float64)[:, None] * X_dev) ** 2, axis=1))
            mul, add = CAPS["R_r"]
            bad = np.flatnonzero(~(R.astype(np.float64) >= res4))
            if bad.size:
                r = int(bad[0])
                f.append("R_r = %.9g of row %d is BELOW ||x - s_r X4|| = %.9g: not an upper bound (%d rows)" % (R[r], r, res4[r], bad.size))
            bad = np.flatnonzero(~(R.astype(np.float64) <= mul * res4 + add))
            if bad.size:
                r = int(bad[0])
                f.append("R_r = %.9g of row %d exceeds its cap %.9g (%d rows)" % (R[r], r, mul * res4[r] + add, bad.size))
            big = res4 > 1e-20
            if big.any():
                note("R_r", np.max(R.astype(np.float64)[big] / res4[big]))
            note("rmax4", _upper(f, "rmax4", info["rmax4"], float(np.max(R)), "rmax4", N))
            rho, lam = i4_stats_ref(x64, s_dev, X_dev, R)
            for k, want in (("rho4", rho), ("lam4", lam)):
                if abs(info[k] - want) > 1e-3 * abs(want) + 1e-30:
                    f.append("%s = %.9g, fp64 %.9g" % (k, info[k], want))

    # -- the residual shadow
    if parts & R2:
        if info["r2_ok"] != int(dim == 128 and eb == 1):
            f.append("r2_ok = %d, expected %d" % (info["r2_ok"], int(dim == 128 and eb == 1)))
        d8r = need("i8r", (rows + PAD) * 128) if info["r2_ok"] else None
        d8 = arrays.get("i8")
        if d8r is not None and s8 is not None and d8 is not None and d8.size == (rows + PAD) * dim:
            s8r = (s8 / F(254.0)).astype(F)
            if _bits(info["s8r"]) != _bits(s8r):
                f.append("s8r = %.9g, expected %.9g" % (info["s8r"], s8r))
            d8r = d8r.reshape(rows + PAD, 128)
            r = fma_resid(x, s8, quant(x, s8, 127))
            _first_diff(f, "Xr", d8r[:rows], quant(r, s8r, 127).astype(np.int8), 128)
            _first_diff(f, "Xr padding", d8r[rows:], np.zeros((PAD, 128), np.int8), 128)
            e2 = x64 - float(F(info["s8"])) * d8.reshape(rows + PAD, dim)[:rows].astype(np.float64) \
                - float(F(info["s8r"])) * d8r[:rows].astype(np.float64)
            res2 = np.sqrt(np.sum(e2 ** 2, axis=1))
            note("resid2", _upper(f, "resid2", info["resid2"], float(np.max(res2)), "resid2", N, " (row %d)" % int(np.argmax(res2))))

    # -- the threshold model's moments
    if parts & PRED:
        if info["pred_model"] != int(dim == 128 and eb == 1):
            f.append("pred_model = %d, expected %d" % (info["pred_model"], int(dim == 128 and eb == 1)))
        words = need("pred", PRED_WORDS) if info["pred_model"] else None
        if words is not None:
            n, stride, srows = pred_sample_rows(rows)
            if (info["pred_n_sample"], info["pred_stride"]) != (n, stride):
                f.append("pred sample (%d, stride %d), expected (%d, %d)" % (info["pred_n_sample"], info["pred_stride"], n, stride))
            xs = x64[srows]
            mean, cov = pred_ref(xs)
            unit = 2.0 * (n + 16) * 2.0 ** -24
            got_m = words[:128].view(F).astype(np.float64)
            got_c = words[128:128 + 128 * 128].view(F).astype(np.float64).reshape(128, 128)
            tol_m = unit * np.mean(np.abs(xs), axis=0) + 1e-37
            tol_c = unit * (np.abs(xs).T @ np.abs(xs) / n + np.outer(np.abs(mean), np.abs(mean))) + 1e-37
            bad = np.flatnonzero(~(np.abs(got_m - mean) <= tol_m))
            if bad.size:
                f.append("pred mean[%d] = %.9g, fp64 %.9g (tolerance %.3g)" % (bad[0], got_m[bad[0]], mean[bad[0]], tol_m[bad[0]]))
            bad = np.flatnonzero(~(np.abs(got_c - cov) <= tol_c).reshape(-1))
            if bad.size:
                i, j = divmod(int(bad[0]), 128)
                f.append("pred covariance[%d][%d] = %.9g, fp64 %.9g (tolerance %.3g; %d entries)"
                         % (i, j, got_c[i, j], cov[i, j], tol_c[i, j], bad.size))
            obs = np.ascontiguousarray(words[128 + 128 * 128:]).view(np.float64)
            if not (obs[0] == 0 and obs[1] == 0 and obs[2] == 0 and obs[3] == 1e300):
                f.append("pred observation block reads %r, expected n = sum = sum2 = 0 and min z = 1e300" % (obs.tolist(),))
    return f


# ---- the table family ---------------------------------------------------------------------------------------------
def gaussian(rows, dim, seed, sigma=0.05):
    return (np.random.default_rng(seed).standard_normal((rows, dim)) * sigma).astype(F)


def witness_table(rows, dim, seed, r_abs=None, c_abs=0, r_norm=None, r_res=None, r_res2=None, base=None):
    """Gaussian rows of sigma 0.05 with one row that alone decides each maximum, so that a reduction which misses that row
    gives a value far outside every cap:
      r_abs   (dim 128) a small row with one element 0.5 at column c_abs: max |x|, hence s8 (0.5 keeps the int8 shadow)
      r_norm  a row of norm 1.0 with elements below 0.35: the max norm
      r_res   (dim 128) x = s8 (m + 0.4999), m the integers of a Gaussian row: the largest ||x - s8 X8||
      r_res2  (dim 128) x = s8 m + s8r (k + 0.49): the largest ||x - s8 X8 - s8r Xr||
    Returns (table, {name: (witness value, runner-up)}) for the gaps the caller asserts."""
    rng = np.random.default_rng(seed + 7919)
    x = gaussian(rows, dim, seed) if base is None else base.copy()          # (base: Gaussian rows made once for a large table)
    if r_abs is not None:
        x[r_abs] = (x[r_abs] * F(0.1)).astype(F)
        x[r_abs, c_abs] = F(0.5)
    if r_norm is not None:
        v = np.clip(rng.standard_normal(dim), -2.5, 2.5)
        x[r_norm] = (v / np.sqrt(np.sum(v * v))).astype(F)
    s8 = scale8(x)
    if r_res is not None:
        m = np.rint(rng.standard_normal(dim) * 0.05 / float(s8))
        x[r_res] = (float(s8) * (m + 0.4999)).astype(F)
    if r_res2 is not None:
        s8r = (s8 / F(254.0)).astype(F)
        m = np.rint(rng.standard_normal(dim) * 0.05 / float(s8))
        k = rng.integers(-100, 101, dim)
        x[r_res2] = (float(s8) * m + float(s8r) * (k + 0.49)).astype(F)
    return x, witness_gaps(x, r_abs is not None, r_res is not None, r_res2 is not None)


def hostile_table():
    """dim 128, int8: s8 = 2^-8 exactly (max |x| = 127 / 256), so that half-steps are exact ties"""
    x = gaussian(70, 128, 11)
    x[3] = (x[3] * F(0.1)).astype(F)
    x[3, 5], x[3, 77] = F(127.0 / 256.0), F(-127.0 / 256.0)          # exactly +-absmax
    s8 = scale8(x)
    assert float(s8) == 2.0 ** -8
    x[10] = 0.0
    x[11] = F(1e-38)
    x[12] = F(5e-31)
    x[13] = F(-0.0)
    x[14, ::2] *= F(-0.0)                                              # signed zeros among ordinary values
    x[15] = np.tile(np.array([2.5, 3.5, -2.5, -3.5, 0.5, -0.5, 1.5, -1.5], F) * s8, 16)
    x[16] = np.tile(np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 7.0, -7.0], F) * F(2.0 ** -6), 16)   # s_r = 2^-6: ties of the 4-bit shadow
    x[40] = x[20]                                                      # a row identical to another
    return x


def witness_gaps(x, with_abs=True, with_res=True, with_res2=True):
    """{maximum: (largest, second largest over the rows)} in fp64 for the maxima that have a witness"""
    def top2(v):
        v = np.sort(np.asarray(v, np.float64))
        return (float(v[-1]), float(v[-2]) if v.size > 1 else 0.0)
    x64 = x.astype(np.float64)
    out = {"max_norm": top2(np.sqrt(np.sum(x64 ** 2, axis=1)))}
    if with_abs:
        out["absmax"] = top2(np.max(np.abs(x64), axis=1))
    if with_res or with_res2:
        s8 = scale8(x)
        X8 = quant(x, s8, 127)
        r = fma_resid(x, s8, X8)
        if with_res:
            out["resid8"] = top2(np.sqrt(np.sum(r.astype(np.float64) ** 2, axis=1)))
        if with_res2:
            s8r = (s8 / F(254.0)).astype(F)
            e2 = fma_resid(r, s8r, quant(r, s8r, 127))
            out["resid2"] = top2(np.sqrt(np.sum(e2.astype(np.float64) ** 2, axis=1)))
    return out
