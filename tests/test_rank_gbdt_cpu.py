"""PG_MODEL_GBDT without a GPU: the blob pa.pack_gbdt builds (header and length as include/pairec_gpu.h documents them), a walk over
the complete trees read back from it against gbdt_ref's walk over the pointer trees, the packer's errors, and the parity inputs
of test_gpu_rank_gbdt.py: that they meet the nodes they are there for."""
import struct

import numpy as np
import pytest

import pairec_amd as pa
from gbdt_cases import BASE, BIG_THR, LE, MIXED, PARITY, blob, forest, inputs
from gbdt_ref import gbdt_margins


def walk_blob(b, x):
    """margins from the blob's complete trees, and what the walk met: {"equal", "nan_left", "nan_right", "big"} -> visits"""
    n_user, n_item, n_tree, depth, _ = struct.unpack("<5I", b[:20])
    nn, rows = 2 ** depth - 1, np.arange(len(x))
    margin = np.full(len(x), np.float64(struct.unpack("<f", b[20:24])[0]))
    met = dict.fromkeys(("equal", "nan_left", "nan_right", "big"), 0)
    for t in range(n_tree):
        at = 24 + t * (3 * nn + 1) * 4
        node = np.frombuffer(b, np.uint32, nn, at)
        thr = np.frombuffer(b, np.float32, nn, at + 4 * nn)
        leaf = np.frombuffer(b, np.float32, nn + 1, at + 8 * nn)
        n = np.zeros(len(x), dtype=np.int64)
        for _ in range(depth):
            v, flag = x[rows, node[n] & 0x7F], (node[n] >> 31) == 1
            met["equal"] += int(np.sum(v == thr[n]))
            met["nan_left"] += int(np.sum(np.isnan(v) & flag))
            met["nan_right"] += int(np.sum(np.isnan(v) & ~flag))
            met["big"] += int(np.sum((thr[n] == BIG_THR) & (v == BIG_THR)))
            n = 2 * n + 2 - ((v < thr[n]) | (np.isnan(v) & flag))
        margin += leaf[n - nn].astype(np.float64)
    return margin, met


@pytest.mark.parametrize("case", PARITY[:5], ids=lambda c: "-".join(map(str, c[:7])))
def test_pack_gbdt_header_and_length(case):
    b = blob(case)
    depth = case[2] or 8                                    # (the mixed forests reach depth 8)
    assert struct.unpack("<5If", b[:24]) == (case[0], case[1], case[3], depth, case[4], np.float32(BASE))
    assert len(b) == 24 + case[3] * (2 * (2 ** depth - 1) + 2 ** depth) * 4


@pytest.mark.parametrize("case", [MIXED, LE], ids=["mixed depths", "lessOrEqual"])
def test_the_packed_trees_walk_as_the_pointer_trees(case):
    x = inputs(case[0], case[1], case[7])[3]
    got, _ = walk_blob(blob(case), x)
    assert np.array_equal(got, gbdt_margins(forest(case), BASE, x, le=case[5]))


def test_pack_gbdt_errors():
    inner = np.arange(0, 18, 2)                             # a chain of 9 splits: node 2j has leaf 2j + 1 on its left, node 2j + 2 on its right
    chain = {"feature": np.zeros(19, int), "threshold": np.zeros(19, np.float32), "missing_left": np.zeros(19, int), "value": np.zeros(19, np.float32),
             "left": -np.ones(19, int), "right": -np.ones(19, int)}
    chain["left"][inner], chain["right"][inner] = inner + 1, inner + 2
    stump = forest(PARITY[0])[0]
    with pytest.raises(ValueError, match="tree 1 is deeper than 8"):
        pa.pack_gbdt([stump, chain], 5, 3, 0.0, 1)
    with pytest.raises(ValueError, match="tree 0 splits on a feature"):
        pa.pack_gbdt([stump], 4, 3, 0.0, 1)                 # the tree names feature 7 somewhere among its 255 nodes
    assert stump["feature"].max() == 7


@pytest.mark.parametrize("case", [PARITY[3], MIXED, PARITY[7]], ids=["5+3", "64+64", "wide"])
def test_the_parity_inputs_meet_their_nodes(case):
    _, cand, _, x = inputs(case[0], case[1], case[7])
    _, met = walk_blob(blob(case), x)
    print(met)
    assert all(met[k] > 0 for k in met)
    assert np.any(np.signbit(x[:, case[0]]) & (x[:, case[0]] == 0)) and np.any(cand >= 500)      # -0.0 met the +0.0 root; rows past the store
