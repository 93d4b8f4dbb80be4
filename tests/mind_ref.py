"""The PG_MODEL_MIND specification (include/pairec_gpu.h) in plain numpy, written the naive way, and the cases test_mind_cpu.py and
test_gpu_mind.py share.  mind_interests(..., dtype=np.float64) is the reference; with dtype=np.float32 it is the same formula with
every value and every operation in float32: the CPU figure a case's bar is 4 x of (the project's convention for an fp32 kernel
whose summation order differs from numpy's).

BARS holds, per case, 4 x the largest |float32 - float64| over the interest components as measured on the CPU, rounded UP to two
digits.  Measured (the figure itself, before the 4 x): edges 5.73e-07, wide 1.62e-07, one 8.19e-08, single-pass 6.70e-07, holes
1.25e-07, neighbours 5.80e-07, steep 4.86e-07, tiny 6.37e-07, long 1.04e-07 — the normalised cases' interests are about 0.1 a
component, the others' about 1.  No case needed a wider margin."""
import functools

import numpy as np

MAX_SEQ = 256
ROWS = 2000           # rows of the sequence table
HOLE = 0xFFFFFFFF

# name: (K, n_iter, d_out, h1, d_user, normalize, row scale, [(sequence entries, how many of them past the table)])
CASES = {
    # the edges of the 16-position tile and of the maximum
    "edges": (3, 3, 64, 128, 7, 0, 1.0, [(0, 0), (1, 0), (15, 0), (16, 0), (17, 0), (33, 0), (256, 0)]),
    "wide": (8, 3, 128, 256, 130, 1, 1.0, [(0, 0), (1, 0), (15, 0), (16, 0), (17, 0), (33, 0), (256, 0)]),
    "one": (1, 3, 64, 128, 1, 1, 1.0, [(17, 0), (256, 0), (0, 0)]),
    "single-pass": (3, 1, 128, 128, 7, 0, 1.0, [(33, 0), (16, 0)]),
    # entries past the table interleaved; one sequence with nothing else
    "holes": (3, 3, 64, 256, 130, 1, 1.0, [(40, 13), (20, 20), (256, 100), (17, 1)]),
    # an empty sequence between two full ones: a request must not see its neighbour's LDS
    "neighbours": (8, 3, 64, 128, 7, 0, 1.0, [(256, 0), (0, 0), (256, 0)]),
    # the two ends of the squash: |z|^2 >> 1 (and routing logits of tens), |z| -> 0
    "steep": (3, 3, 64, 128, 7, 0, 30.0, [(33, 0), (256, 0), (16, 0)]),
    "tiny": (8, 3, 128, 256, 7, 0, 1e-6, [(33, 0), (256, 0)]),
    # 300 entries: the device form uses the first MAX_SEQ (the host form refuses the call)
    "long": (3, 3, 64, 128, 7, 1, 1.0, [(300, 40)]),
}
BARS = {"edges": 2.3e-06, "wide": 6.5e-07, "one": 3.3e-07, "single-pass": 2.7e-06, "holes": 5.0e-07, "neighbours": 2.4e-06, "steep": 2.0e-06,
        "tiny": 2.6e-06, "long": 4.2e-07}


@functools.lru_cache(maxsize=None)
def table(scale=1.0):
    """ROWS rows of dim 64, norm about `scale`"""
    return (np.random.default_rng(11).standard_normal((ROWS, 64)) * (scale / 8.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def weights(K, d_out, h1, d_user):
    """S, b0, Wc, Wu, b1, W2, b2: u^ of about the rows' norm, routing logits N(0, 1) as MIND initialises them, interests O(1)"""
    rng = np.random.default_rng(1000 * K + d_out + h1 + d_user)
    u = lambda shape, fan, g=1.0: (rng.uniform(-1, 1, shape) * (g * np.sqrt(3.0 / fan))).astype(np.float32)   # noqa: E731
    return (u((64, 64), 64), rng.standard_normal((K, MAX_SEQ)).astype(np.float32), u((64, h1), 64, 2.0), u((d_user, h1), d_user), u((h1,), h1),
            u((h1, d_out), h1), u((d_out,), h1))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(user vectors [n_req][d_user], the sequences) of a case"""
    K, _, _, _, d_user, _, _, lens = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    seqs = []
    for n, holes in lens:
        s = rng.integers(0, ROWS, n).astype(np.uint32)
        s[rng.permutation(n)[:holes]] = [ROWS, HOLE, ROWS + 5][holes % 3]
        seqs.append(s)
    return rng.standard_normal((len(lens), d_user)).astype(np.float32), seqs


def mind_interests(w, tab, users, seqs, n_iter, normalize, dtype=np.float64):
    """interests [n_req][K][d_out] in `dtype`"""
    S, b0, Wc, Wu, b1, W2, b2 = (np.asarray(a, dtype=dtype) for a in w)
    tab, one = np.asarray(tab, dtype=dtype), dtype(1)
    out = np.zeros((len(seqs), b0.shape[0], W2.shape[1]), dtype=dtype)
    for r, seq in enumerate(seqs):
        s = np.asarray(seq[:MAX_SEQ], dtype=np.int64)
        uh = tab[s[s < tab.shape[0]]] @ S                                   # [n][64]
        b = b0[:, :uh.shape[0]].copy()
        for it in range(1, n_iter + 1):
            e = np.exp(b - b.max(axis=0))
            z = (e / e.sum(axis=0)) @ uh                                    # [K][64]
            q = (z * z).sum(axis=1, keepdims=True)
            v = z * q / ((one + q) * np.sqrt(q + dtype(1e-9)))
            if it < n_iter:
                b = b + v @ uh.T
        h = np.maximum(v @ Wc + np.asarray(users[r], dtype=dtype) @ Wu + b1, dtype(0))
        o = h @ W2 + b2
        if normalize:
            o = o / np.sqrt((o * o).sum(axis=1, keepdims=True) + dtype(1e-12))
        out[r] = o
    return out


@functools.lru_cache(maxsize=None)
def reference(name, dtype=np.float64):
    K, n_iter, d_out, h1, d_user, normalize, scale, _ = CASES[name]
    return mind_interests(weights(K, d_out, h1, d_user), table(scale), *inputs(name), n_iter, normalize, dtype)
