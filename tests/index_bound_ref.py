"""The exact IVF index's bound, restated in numpy (index_build.hip: radius_kernel, cnorm_kernel; index_search.hip: bound_kernel; all fp64, every
table-side input rounded up to fp32 first), and adversarial lists to test it on.  Shared by tests/test_index_cpu.py (the formula
dominates every chain score) and tests/test_gpu_index_bounds.py (the device's state equals the formula)."""
import numpy as np


def _up32(v):
    """the smallest float32 >= v (elementwise, v float64)"""
    f = np.asarray(v, dtype=np.float64).astype(np.float32)
    low = f.astype(np.float64) < v
    return np.where(low, np.nextafter(f, np.float32(np.inf)), f)


def _cnorm(c):
    """||c_L|| as the build measures it (index_build.hip: cnorm_kernel): fp64, a 2^-40 relative margin, rounded up to fp32"""
    return float(_up32(np.sqrt(np.sum(c.astype(np.float64) ** 2)) * (1 + 2.0 ** -40)))


def _list_side(x, c):
    """r_L and ||c_L|| as the build measures them: fp64, a 2^-40 relative margin, rounded up to fp32"""
    d = x.astype(np.float64) - c.astype(np.float64)
    r = _up32(np.sqrt(np.max(np.sum(d * d, axis=1))) * (1 + 2.0 ** -40))
    return float(r), _cnorm(c)


def _bound_ip(q, c, r, cn):
    dim = q.shape[1]
    u = 2.0 ** -24
    gam = dim * u / (1 - dim * u)
    qn = np.sqrt(np.sum(q.astype(np.float64) ** 2, axis=1)) * (1 + 2.0 ** -40)
    cq = q.astype(np.float64) @ c.astype(np.float64)
    a = (cn + r) * qn
    slack = gam * a * (1 + 2.0 ** -20) + 2.0 ** -40 * a + dim * 2.0 ** -148
    out = _up32(cq + r * qn + slack)
    return np.where(a * (1 + gam) * 2 < 2.0 ** 127, out, np.inf)


def _bound_neg_l2(q, c, r, cn):
    """upper bound of -d (the search ranks squared Euclidean recalls by -d)"""
    dim = q.shape[1]
    u = 2.0 ** -24
    gam = (dim + 3) * u / (1 - (dim + 3) * u)
    qn = np.sqrt(np.sum(q.astype(np.float64) ** 2, axis=1)) * (1 + 2.0 ** -40)
    s = np.sqrt(np.sum((q.astype(np.float64) - c.astype(np.float64)) ** 2, axis=1)) * (1 - 2.0 ** -40)
    lb = np.maximum(s - r, 0.0)
    lb2 = lb * lb * (1 - 2.0 ** -40)
    b = cn + r + qn
    err = gam * b * b * (1 + 2.0 ** -20) + 2.0 ** -40 * b * b + dim * 2.0 ** -146
    out = _up32(err - lb2)
    return np.where(b * b * 2 < 2.0 ** 126, out, np.inf)


def _adversarial(dim, scale, rng):
    """a list: centroid c and rows around it — some exactly on the sphere of the measured radius, sign patterns that line up
    every term of the chain (maximal rounding), near-duplicates of the centroid; queries: aligned, opposite, one-hot, zero,
    sign-matched"""
    c = (rng.standard_normal(dim) * scale).astype(np.float32)
    signs = np.sign(rng.standard_normal((8, dim))).astype(np.float32)
    dirs = rng.standard_normal((24, dim))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rad = 0.3 * np.linalg.norm(c.astype(np.float64)) + 1e-30
    on_sphere = (c.astype(np.float64) + rad * dirs).astype(np.float32)        # rows at (about) the measured radius
    aligned = (c.astype(np.float64) + rad * signs / np.sqrt(dim)).astype(np.float32)
    near = (c + np.float32(scale) * np.float32(1e-6) * signs[:2]).astype(np.float32)
    x = np.concatenate([on_sphere, aligned, near, c[None, :]]).astype(np.float32)
    onehot = np.zeros((2, dim), dtype=np.float32)
    onehot[0, 0] = 1.0
    onehot[1, dim - 1] = -np.float32(scale)
    q = np.concatenate([
        c[None, :], -c[None, :], signs[:3] * np.float32(scale), aligned[:2], onehot, np.zeros((1, dim), np.float32),
        (rng.standard_normal((3, dim)) * scale).astype(np.float32),
    ]).astype(np.float32)
    return x, c, q
