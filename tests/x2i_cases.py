"""The X table and the requests that tests/test_gpu_x2i.py runs on the device, tests/test_x2i_cpu.py through pg_x2i_recall_host and
tests/x2i_check.cpp (from the files write_grid leaves) through csrc/x2i_host.hpp alone.  An item table of 70 001 rows — just past
65 536 — with a nonzero row_offset and 4 200 X values: a random body, crafted regions behind it, and a band of rows and of X that is
never uploaded."""
import numpy as np

ROWS, N_X, ROW_OFFSET = 70001, 4200, 1 << 20
ROW_BAND, X_BAND = (65000, 66000), (4030, 4090)      # never uploaded
LDS_SLOTS, LDS_MAX_PAIRS, KNOB_DEFAULT = 10240, 5120, 6144    # x2i.hip: the LDS tier's table and its limit; cf_lds_max_pairs' default
X_SLOTS = 4096                                       # ... hop 1's table
HASH_MUL = 0x9E3779B1                                # ... and the hash: ((key * HASH_MUL mod 2^32) * slots) >> 32
U32MAX = 0xFFFFFFFF

# crafted rows (their X lists) and crafted X (their item lists)
R_SHARED, X_SHARED = 60000, 2000                     # 256 rows that all name X 2000, and X 2001 .. 2004 each in an order of its own
R_FAN, X_FAN, N_FAN = 60300, 2100, 300               # row R_FAN + i names X_FAN + i; every X_FAN + i lists items 62000 .. 62004
R_WIDE, X_WIDE = 60700, 2400                         # one row with 64 X
R_MANY, X_MANY = 60800, 3000                         # rows of 64 X each: 16 rows reach 1024 distinct X, the 17th one more
R_LONG, X_LONG, N_LONG = 60900, 2500, 64             # row R_LONG + i names X_LONG + i, a list of 1024
R_ONE, X_ONE = 60970, 2565                           # ... and one pair more
R_COLLIDE, X_COLLIDE = 61100, 2600                   # five X whose items collide in the item tables, one per row
R_XCOLLIDE = 61110                                   # a row whose X collide in hop 1's table; R_XCOLLIDE + 1: x ids 0 and 4096
R_DYADIC, X_DYADIC = 61200, 2700                     # eight rows / X with dyadic scores over 20 items
R_EMPTY, X_EMPTY = 61300, 2800                       # an X with an empty list; R_EMPTY + 1 names it and X_DYADIC
R_SELF, X_SELF = 61400, 2810                         # X_SELF lists exactly the two rows that name it
R_NOX = 69990                                        # a row without X


def slot(keys, slots):
    return ((np.asarray(keys, np.uint64) * np.uint64(HASH_MUL) & np.uint64(U32MAX)) * np.uint64(slots)) >> np.uint64(32)


def wide_prefer(rng, n):
    """magnitudes from 1e-8 to 1e16, mixed signs: any other addition order changes bits"""
    return 10.0 ** rng.uniform(-8, 16, n) * rng.choice([-1.0, 1.0], n)


def csr(lists, scores=None):
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(l) for l in lists])
    ids = np.concatenate([np.asarray(l, np.uint32) for l in lists]) if len(lists) else np.zeros(0, np.uint32)
    if scores is None:
        return off, ids
    return off, ids, (np.concatenate([np.asarray(s, np.float32) for s in scores]) if len(scores) else np.zeros(0, np.float32))


def build():
    """(i2x [ROWS] lists of x ids, x2i [N_X] lists of item rows, x2i_scores [N_X] lists of float32)"""
    rng = np.random.default_rng(71)
    every = np.arange(ROWS)
    i2x = [[] for _ in range(ROWS)]
    x2i = [np.zeros(0, np.uint32) for _ in range(N_X)]
    sc = [np.zeros(0, np.float32) for _ in range(N_X)]

    def put(x, items, scores=None):
        x2i[x] = np.asarray(items, np.uint32)
        sc[x] = (rng.standard_normal(len(items)) if scores is None else np.asarray(scores)).astype(np.float32)

    # the body: rows below 60 000 with 0 .. 5 of the X below 2 000, whose lists have 0 .. 1 024 items
    nx = rng.choice([0, 1, 2, 3, 5], 60000, p=[0.1, 0.3, 0.3, 0.2, 0.1])
    for r in range(60000):
        i2x[r] = rng.choice(2000, nx[r], replace=False).tolist()
    lens = rng.choice([0, 1, 7, 64, 65, 300, 1024], 2000, p=[0.05, 0.2, 0.3, 0.2, 0.15, 0.08, 0.02])
    for x in range(2000):
        put(x, rng.choice(ROWS, lens[x], replace=False))
    for i in range(256):
        i2x[R_SHARED + i] = [X_SHARED] + (X_SHARED + 1 + rng.permutation(4)).tolist()
    put(X_SHARED, np.arange(61000, 61050), rng.uniform(0.1, 1.0, 50))
    for j in range(1, 5):
        put(X_SHARED + j, rng.permutation(np.arange(61000, 61060))[:40], rng.uniform(0.1, 1.0, 40))
    for i in range(N_FAN):
        i2x[R_FAN + i] = [X_FAN + i]
        put(X_FAN + i, 62000 + rng.permutation(5), np.full(5, 1.0 if i < 3 else rng.choice([0.5, 1.0, 2.0])))
    i2x[R_WIDE] = (X_WIDE + rng.permutation(64)).tolist()
    for j in range(64):
        put(X_WIDE + j, rng.choice(ROWS, 10, replace=False))
    for i in range(17):
        i2x[R_MANY + i] = list(range(X_MANY + 64 * i, X_MANY + 64 * i + (64 if i < 16 else 1)))
    for x in range(X_MANY, X_MANY + 1025):
        put(x, rng.choice(ROWS, 3, replace=False))
    for i in range(N_LONG):
        i2x[R_LONG + i] = [X_LONG + i]
        put(X_LONG + i, rng.choice(ROWS, 1024, replace=False))
    i2x[R_ONE] = [X_ONE]
    put(X_ONE, [12345])
    collide = [
        np.arange(1, 7) * LDS_SLOTS,                  # multiples of the LDS tier's slot count
        7 + 1024 * np.arange(68),                     # equal low bits
        2048 * np.arange(1, 35),                      # multiples of a global-tier slot count
        every[(slot(every, LDS_SLOTS) >= 100) & (slot(every, LDS_SLOTS) < 150)][:1024],   # one long probe run in the LDS table
        every[slot(every, 1024) == 5][:1024],         # one slot of the smallest global table
    ]
    for j, items in enumerate(collide):
        i2x[R_COLLIDE + j] = [X_COLLIDE + j]
        put(X_COLLIDE + j, items)
    xs = np.arange(N_X)
    run = xs[(slot(xs, X_SLOTS) >= 100) & (slot(xs, X_SLOTS) < 140) & ((xs < X_BAND[0]) | (xs >= X_BAND[1]))][:64]
    assert len(run) >= 30
    i2x[R_XCOLLIDE] = run.tolist()
    i2x[R_XCOLLIDE + 1] = [4096, 0]
    put(4096, [100, 200, 300])
    for i in range(8):
        i2x[R_DYADIC + i] = [X_DYADIC + i]
        put(X_DYADIC + i, 63000 + rng.permutation(20), rng.choice([0.25, 0.5, 0.75, 1.0], 20))
    i2x[R_EMPTY] = [X_EMPTY]
    i2x[R_EMPTY + 1] = [X_EMPTY, X_DYADIC]
    i2x[R_SELF] = [X_SELF]
    i2x[R_SELF + 1] = [X_SELF]
    put(X_SELF, [R_SELF + 1, R_SELF], [1.0, 2.0])
    for r in range(*ROW_BAND):
        i2x[r] = []
    for x in range(*X_BAND):
        put(x, [])
    return i2x, x2i, sc


def upload(target, built):
    """the table into anything with upload_item2x / upload_x2item, each side in two parts around its band"""
    i2x, x2i, sc = built
    target.upload_item2x(*csr(i2x[:ROW_BAND[0]]), 0)
    target.upload_item2x(*csr(i2x[ROW_BAND[1]:]), ROW_BAND[1])
    target.upload_x2item(*csr(x2i[:X_BAND[0]], sc[:X_BAND[0]]), 0)
    target.upload_x2item(*csr(x2i[X_BAND[1]:], sc[X_BAND[1]:]), X_BAND[1])


def grid():
    """{name: (triggers, prefer, k, normalize, max_rule)}: the requests every implementation answers alike"""
    rng = np.random.default_rng(72)
    g = {}
    shared = R_SHARED + rng.permutation(256)
    g["shared_x_256"] = ([shared], [wide_prefer(rng, 256)], 64, True, False)
    g["shared_x_256_raw"] = ([shared], [wide_prefer(rng, 256)], 64, False, False)
    g["addition_order_x"] = ([[R_SHARED, R_SHARED + 1, R_SHARED + 2], [R_SHARED, R_SHARED + 2, R_SHARED + 1]],
                             [[1e16, 1.0, -1e16], [1e16, -1e16, 1.0]], 60, False, False)
    fan = R_FAN + rng.permutation(N_FAN)[:256]
    g["shared_item_fan"] = ([fan, fan[::-1]], [wide_prefer(rng, 256)] * 2, 10, False, False)
    g["addition_order_item"] = ([[R_FAN, R_FAN + 1, R_FAN + 2], [R_FAN, R_FAN + 2, R_FAN + 1]], [[1e16, 1.0, -1e16], [1e16, -1e16, 1.0]], 10,
                                False, False)
    g["wide_and_many"] = ([[R_WIDE], list(range(R_MANY, R_MANY + 16)), [R_XCOLLIDE, R_XCOLLIDE + 1]],
                          [[2.5], wide_prefer(rng, 16), [1.5, -3.0]], 4000, True, False)
    trig = [[R_COLLIDE, R_COLLIDE + 1, R_COLLIDE + 2], [R_COLLIDE + 3], [R_COLLIDE + 4], [R_COLLIDE + j for j in (4, 3, 2, 1, 0, 3)]]
    g["colliding_rows"] = (trig, [wide_prefer(rng, len(t)) for t in trig], 2048, True, False)
    dy = list(range(R_DYADIC, R_DYADIC + 8))
    g["ties"] = ([dy, dy[:3]], [[1, 2, 3, 4, 1, 2, 3, 4], [2, 2, 4]], 20, True, False)
    g["ties_raw"] = ([dy, dy[:3]], [[1, 2, 3, 4, 1, 2, 3, 4], [2, 2, 4]], 20, False, False)
    g["ties_max"] = ([dy, dy[:3]], [[1, 2, 3, 4, 1, 2, 3, 4], [2, 2, 4]], 20, False, True)
    g["negative"] = ([shared[:40], [R_DYADIC, R_SHARED]], [-np.abs(wide_prefer(rng, 40)), [-0.0, -1.0]], 70, True, False)
    edges = [
        [],                                                     # no triggers
        [U32MAX],
        [ROWS, ROWS + 1, U32MAX - 1],                           # >= rows
        [R_NOX],                                                # a trigger without X
        [ROW_BAND[0] + 5],                                      # never uploaded
        [R_EMPTY],                                              # an X with an empty list
        [R_EMPTY + 1],
        [R_SELF, R_SELF + 1],                                   # every candidate is a trigger
        [R_SELF],                                               # ... and one of them is not
        [R_FAN, R_FAN, R_FAN + 1],                              # a trigger twice contributes twice: here its X sum is not finite
        [R_DYADIC, R_DYADIC],
        [R_XCOLLIDE + 1, U32MAX, R_WIDE, ROWS, R_NOX, R_DYADIC + 1],
        rng.integers(0, 60000, 256),                            # 256 triggers
        [R_LONG],                                               # an X list of 1 024
    ]
    pref = [wide_prefer(rng, len(t)) for t in edges]
    pref[9] = [1e308, 1e308, 3.0]
    pref[10] = [1.5, 2.5]
    g["edges"] = (edges, pref, 1100, True, False)
    g["edges_max"] = (edges, pref, 1100, False, True)
    return g


def mixed():
    """a batch of 256 requests over the body and the crafted rows"""
    rng = np.random.default_rng(73)
    trig = []
    for q in range(256):
        n = 0 if q % 8 == 3 else int(rng.integers(1, 30))
        if q in (40, 200):
            n = 256
        trig.append(rng.integers(0, 61500, n))
    trig[7] = rng.integers(0, 60000, 12)
    trig[9] = list(range(R_LONG, R_LONG + 7))                   # the global tier at the default knob
    trig[10] = list(range(R_LONG, R_LONG + 5))                  # the LDS tier's limit
    return trig, [wide_prefer(rng, len(t)) for t in trig]


def write_grid(path, built):
    """the table and the grid's requests as flat little-endian files for tests/x2i_check.cpp:
    table.bin = rows, row_offset, n_x (uint64 each), then i2x offsets, x2i offsets (uint64), i2x ids, x2i rows (uint32), scores (float32);
    requests.bin = per case: nq, k, normalize, max_rule, total (uint32), offsets uint32[nq + 1], rows uint32[total], prefer float64[total]"""
    i2x, x2i, sc = built
    io, ii = csr(i2x)
    xo, xr, xs = csr(x2i, sc)
    with open(path / "table.bin", "wb") as f:
        f.write(np.array([ROWS, ROW_OFFSET, N_X], np.uint64).tobytes())
        for a in (io, xo, ii, xr, xs):
            f.write(np.ascontiguousarray(a).tobytes())
    with open(path / "requests.bin", "wb") as f:
        for name, (trig, pref, k, normalize, max_rule) in grid().items():
            off = np.zeros(len(trig) + 1, np.uint32)
            off[1:] = np.cumsum([len(t) for t in trig])
            f.write(np.array([len(trig), k, int(normalize), int(max_rule), off[-1]], np.uint32).tobytes())
            f.write(off.tobytes())
            f.write(np.concatenate([np.asarray(t, np.uint32).reshape(-1) for t in trig]).astype(np.uint32).tobytes())
            f.write(np.concatenate([np.asarray(p, np.float64).reshape(-1) for p in pref]).astype(np.float64).tobytes())
