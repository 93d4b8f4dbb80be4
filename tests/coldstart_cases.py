"""The pools and ordered columns the ColdStartRecall tests share (test_coldstart_cpu.py, test_gpu_coldstart.py): generated once per
row count from fixed seeds, never changed."""
import numpy as np

ROWS = (1, 31, 32, 33, 1023, 1024, 1025, 40000, 300001)
KS = (1, 7, 256, 257, 4096, 16384)
BLOCK = 1024
# pool name -> the clause that admits it over the columns of store() (None: no clause, every row).  One-comparison clauses and
# compound ones both occur: the first kind builds its bitmap only for this recall.
POOLS = {
    "none": "m_none = 1",
    "first": "m_first = 1 AND one >= 1",
    "last": "m_last = 1",
    "all_null": None,
    "all_true": "one = 1",
    "third": "m_third = 1 AND one IN (1, 2)",
    "tail": "m_tail = 1",
    "dense_sparse": "NOT (m_dense_sparse <> 1)",
}


def masks(rows: int) -> dict:
    r = np.arange(rows)
    rng = np.random.default_rng(1000 + rows)
    m = {
        "none": np.zeros(rows, bool),
        "first": r == 0,
        "last": r == rows - 1,
        "all_null": np.ones(rows, bool),
        "all_true": np.ones(rows, bool),
        "third": r % 3 == 0,
        "tail": r >= (rows - 1) // BLOCK * BLOCK,                     # only the last (partial) block
        "dense_sparse": (r < BLOCK) | (rng.random(rows) < 1.0 / 97),    # a dense first block, a sparse rest
    }
    return m


def store(rows: int) -> dict:
    """the clause columns: {name: int32 / int64 array}"""
    cols = {"one": np.ones(rows, np.int64)}
    for name, m in masks(rows).items():
        if not name.startswith("all"):
            cols["m_" + name] = m.astype(np.int32)
    return cols


NP_OF = {"i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}


def order_columns(rows: int) -> dict:
    """{(dtype name, pattern): array}: all values equal; two values whose runs of ties straddle the k-th place and block
    boundaries at the tests' k; distinct values; the integer extremes; the floats' special values"""
    rng = np.random.default_rng(2000 + rows)
    r = np.arange(rows)
    out = {}
    for dn, dt in NP_OF.items():
        is_f = dn[0] == "f"
        out[dn, "equal"] = np.full(rows, 7, dt)
        out[dn, "two"] = np.where(r % 5 == 0, dt(-3), dt(11)).astype(dt)
        out[dn, "distinct"] = (rng.permutation(rows) - rows // 2).astype(dt)      # (rows < 2^24: exact in float32 too)
        if not is_f:
            info = np.iinfo(dt)
            out[dn, "extremes"] = rng.choice(np.array([info.min, info.max, -1, 0, 1, info.min + 1, info.max - 1], dtype=dt), rows)
        else:
            info = np.finfo(dt)
            u = {"f32": np.uint32, "f64": np.uint64}[dn]
            nan_bits = {"f32": [0x7FC00000, 0x7F800001, 0xFFC00123, 0xFF800001], "f64": [0x7FF8000000000000, 0x7FF0000000000001,
                        0xFFF8000000000123, 0xFFF0000000000001]}[dn]
            special = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, info.tiny, -info.tiny, info.smallest_subnormal,
                                                -info.smallest_subnormal, info.tiny / 4, -info.tiny / 4, info.max, info.min, 1.5, -1.5],
                                               dtype=dt), np.array(nan_bits, dtype=u).view(dt)])
            out[dn, "special"] = special[rng.integers(0, len(special), rows)]
    return out


def bitmap(mask: np.ndarray) -> np.ndarray:
    """a bool mask as the clause's bitmap: bit r & 31 of word r >> 5"""
    rows = mask.shape[0]
    pad = np.zeros((rows + 31) // 32 * 32, np.uint8)
    pad[:rows] = mask
    return np.packbits(pad, bitorder="little").view("<u4").astype(np.uint32)
