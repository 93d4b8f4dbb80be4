"""The cases of the row-selection tests past one scan group of rows (test_row_scale_cpu.py, test_gpu_row_scale.py): one row count
per device, eight masks each built to stress one place of the three-level scans, a feature store from whose columns every mask
is a flag column (int32, and int64 beyond 2^40) and a compound clause, a dim-64 table whose rows name themselves, the ColdStart
order columns.  numpy only; generated from fixed seeds, never changed by a test.

rows_for(cus) is the smallest shape with, at once: five scan groups / chunks of 1 024 blocks of 1 024 rows (thread 1 of
filter_total_scan_kernel works, its group 4 is partial); two full trips and a ragged last one of the grid-stride kernels whose grid
is min(tiles, 8 x CUs) (exactly three trips from 256 CUs on; a smaller device makes more, the last still ragged); a last block of 3
rows (rows % 4 == 3: the tail branches of the 4-row loads; rows % 32 == 3: a partial last bitmap word)."""
import numpy as np

import coldstart_cases

BLOCK = 1024                     # rows per block / tile of every kernel here
G = BLOCK * 1024                 # rows per scan group / chunk
BIG = 1 << 40                    # what the int64 columns add to their values
DIM, ROW_OFFSET = 64, 7
EDGE = 1024                      # `edges`: rows on either side of a group boundary
TWO_RUN = 3000                   # `i32_two`: rows of the smaller value on either side of a chunk boundary
K_RECALL, NQ_MAX = 300, 40
MASKS = ("edges", "one_group", "last_group", "sparse", "eighth", "trip_tail", "none", "all")
VIEW_MASKS = MASKS[:6]           # (`none` admits nothing; no view is made of `all`)
PAIR_VALUES = (2.0, 1.75)        # columns 2..9 of the two duplicate pairs: above every other row's (uniform in [-1, 1))


def rows_for(cus: int) -> int:
    return (max(16 * cus, 4096) + 5) * BLOCK + 3


def device_cus() -> int:
    """the device's CU count (a GPU test's: asked of a short-lived child process)"""
    from test_gpu_table_derived import device_cus as ask
    return ask()


def shape(rows: int, cus: int) -> dict:
    blocks = (rows + BLOCK - 1) // BLOCK
    grid = min(blocks, 8 * cus)
    return {"blocks": blocks, "groups": (blocks + 1023) // 1024, "grid": grid, "trips": (blocks + grid - 1) // grid,
            "last_block_rows": rows - (blocks - 1) * BLOCK, "trip_rows": grid * BLOCK}


def _uv(rows: int):
    rng = np.random.default_rng(0xE16 + rows)
    return rng.integers(0, 31, rows).astype(np.int32), rng.integers(0, 2, rows)


def masks(rows: int, cus: int) -> dict:
    """{name: bool [rows]}, stated over the row index (`eighth`: over the two seeded random columns)"""
    r = np.arange(rows, dtype=np.int64)
    ng = shape(rows, cus)["groups"]
    edges = np.zeros(rows, bool)
    edges[0] = True
    edges[rows - 3:] = True
    for g in range(1, ng):
        edges[g * G - EDGE:g * G + EDGE] = True
    u, v = _uv(rows)
    return {
        "edges": edges,                                          # offsets are wrong exactly where a group starts
        "one_group": (r >= 3 * G) & (r < 4 * G),                 # the groups' totals: 0, 0, 0, 2^20, 0
        "last_group": r >= (ng - 1) * G,                         # only the partial group
        "sparse": r % 1021 == 5,                                 # 1 or 2 rows a block: the offsets carry through all groups
        "eighth": (u < 8) & (v == 1),                            # dense (8 / 62 of the rows): the largest view, never compacted
        "trip_tail": r >= 2 * 8 * cus * BLOCK,                   # only tiles of the trips behind the second
        "none": np.zeros(rows, bool),
        "all": np.ones(rows, bool),
    }


def store(rows: int, cus: int) -> dict:
    """{column: int32 / int64 [rows]}: the columns the clauses read, then f_<mask> (int32 0 / 1) and g_<mask> (int64 2^40 + 0 / 1)"""
    r = np.arange(rows, dtype=np.int64)
    u, v = _uv(rows)
    cols = {"r32": r.astype(np.int32), "r64": BIG + r, "inb": (r & (G - 1)).astype(np.int32), "grp": BIG + (r >> 20),
            "m32": (r % 1021).astype(np.int32), "m64": BIG + r % 1021, "u": u, "v": BIG + v}
    for name, m in masks(rows, cus).items():
        cols["f_" + name] = m.astype(np.int32)
        cols["g_" + name] = BIG + m.astype(np.int64)
    return cols


def clauses(rows: int, cus: int) -> dict:
    """{mask: (compound clause over store()'s columns, the same in numpy over those columns)}: AND / OR / IN / NOT over at least
    one int32 and one int64 column each, so none binds to the single-column form"""
    ng = shape(rows, cus)["groups"]
    last0, t0 = (ng - 1) * G, 2 * 8 * cus * BLOCK
    return {
        "edges": ("(inb < %d AND grp >= %d) OR (inb >= %d AND grp < %d) OR r32 = 0 OR r64 >= %d" % (EDGE, BIG + 1, G - EDGE, BIG + ng - 1, BIG + rows - 3),
                  lambda c: ((c["inb"] < EDGE) & (c["grp"] >= BIG + 1)) | ((c["inb"] >= G - EDGE) & (c["grp"] < BIG + ng - 1)) | (c["r32"] == 0) |
                            (c["r64"] >= BIG + rows - 3)),
        "one_group": ("r32 >= %d AND r64 < %d" % (3 * G, BIG + 4 * G), lambda c: (c["r32"] >= 3 * G) & (c["r64"] < BIG + 4 * G)),
        "last_group": ("NOT (r32 < %d OR grp < %d)" % (last0, BIG + ng - 1), lambda c: ~((c["r32"] < last0) | (c["grp"] < BIG + ng - 1))),
        "sparse": ("m32 IN (4, 5, 6) AND NOT m64 IN (%d, %d)" % (BIG + 4, BIG + 6), lambda c: np.isin(c["m32"], [4, 5, 6]) & ~np.isin(c["m64"], [BIG + 4, BIG + 6])),
        "eighth": ("u < 8 AND v = %d" % (BIG + 1), lambda c: (c["u"] < 8) & (c["v"] == BIG + 1)),
        "trip_tail": ("r32 >= %d AND NOT r64 < %d" % (t0, BIG + t0), lambda c: (c["r32"] >= t0) & ~(c["r64"] < BIG + t0)),
        "none": ("r32 < 0 AND grp = %d" % BIG, lambda c: (c["r32"] < 0) & (c["grp"] == BIG)),
        "all": ("r32 >= 0 OR grp = %d" % BIG, lambda c: (c["r32"] >= 0) | (c["grp"] == BIG)),
    }


def dup_pairs(eighth: np.ndarray):
    """the two pairs of duplicate rows: (G - 1, G), and the rows `eighth` admits last below and first above them — neighbours in
    its compaction, on either side of the first group boundary"""
    a = int(np.flatnonzero(eighth[:G - 1])[-1])
    b = G + 1 + int(np.flatnonzero(eighth[G + 1:2 * G])[0])
    return (G - 1, G), (a, b)


def table(rows: int, eighth: np.ndarray) -> np.ndarray:
    """[rows][64] float32: columns 0 and 1 the row index as two exact floats, 2..9 seeded random in [-1, 1), the rest zero; the
    rows of a duplicate pair equal beyond columns 0 and 1"""
    tab = np.zeros((rows, DIM), np.float32)
    r = np.arange(rows, dtype=np.int64)
    tab[:, 0] = r & 0xFFFFFF
    tab[:, 1] = r >> 24
    tab[:, 2:10] = np.random.default_rng(0x7AB + rows).random((rows, 8), dtype=np.float32) * np.float32(2) - np.float32(1)
    for pair, val in zip(dup_pairs(eighth), PAIR_VALUES):
        tab[list(pair), 2:10] = np.float32(val)
    return tab


def decode(x: np.ndarray) -> np.ndarray:
    """the source rows that rows of the table name in their columns 0 and 1"""
    return x[:, 0].astype(np.int64) + (x[:, 1].astype(np.int64) << 24)


def queries() -> np.ndarray:
    """[40][64]: zero in the two index columns (a duplicate pair then ties under the inner product); query 0 points at the
    duplicate pairs, which lead its answer wherever a mask admits them"""
    q = np.zeros((NQ_MAX, DIM), np.float32)
    q[:, 2:10] = np.random.default_rng(0x9E).random((NQ_MAX, 8), dtype=np.float32) * np.float32(2) - np.float32(1)
    q[0, 2:10] = 1.0
    return q


def order_columns(rows: int) -> dict:
    """i32_two: two values, the smaller within TWO_RUN rows of every chunk boundary, so the better rows and the threshold's tie run
    of a deep answer cross chunks in a dense pool and in a sparse one; i64_distinct: a permutation; f32_special: zeros,
    infinities, NaNs, subnormals (the last two as coldstart_cases.order_columns makes them)"""
    oc = coldstart_cases.order_columns(rows)
    inb = np.arange(rows, dtype=np.int64) & (G - 1)
    return {"i32_two": np.where((inb < TWO_RUN) | (inb >= G - TWO_RUN), -3, 11).astype(np.int32),
            "i64_distinct": oc["i64", "distinct"], "f32_special": oc["f32", "special"]}


bitmap = coldstart_cases.bitmap
