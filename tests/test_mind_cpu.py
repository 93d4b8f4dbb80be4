"""PG_MODEL_MIND without a GPU: the blob pa.pack_mind builds (header and length as include/pairec_gpu.h documents them), its shape
errors, and the bars of test_gpu_mind.py — the float32 restatement of mind_ref stays under a quarter of each case's bar."""
import os
import struct
import sys

import numpy as np
import pytest

import pairec_amd as pa
from mind_ref import BARS, CASES, MAX_SEQ, reference, weights

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import pack_model  # noqa: E402


def test_pack_mind_header_and_length():
    assert pa.MIND_MAX_SEQ == MAX_SEQ == 256 and pa.MODEL_MIND == 11
    for K, d_out, h1, d_user in ((3, 64, 128, 7), (8, 128, 256, 130)):
        w = weights(K, d_out, h1, d_user)
        blob = pa.pack_mind(*w, n_iter=3, normalize=True)
        assert struct.unpack("<6I", blob[:24]) == (d_user, d_out, K, 3, h1, 1)
        assert len(blob) == 24 + 4 * (64 * 64 + K * 256 + 64 * h1 + d_user * h1 + h1 + h1 * d_out + d_out)
        assert blob[24:24 + 64 * 64 * 4] == w[0].tobytes() and blob[-4 * d_out:] == w[6].tobytes()


def test_pack_model_tool_builds_the_same_blob():
    w = weights(8, 128, 256, 130)
    z = dict(zip(("s", "routing_init", "wc", "wu", "b1", "w2", "b2"), w), n_iter=np.array([2]), normalize=np.array(1))
    kind, blob, _ = pack_model.pack_npz(z)
    assert kind == pa.MODEL_MIND and blob == pa.pack_mind(*w, n_iter=2, normalize=1)
    with pytest.raises(ValueError):
        pack_model.pack_npz(dict(z, n_iter=np.array([5])))


@pytest.mark.parametrize("change", [
    lambda w: w.__setitem__(0, w[0][:, :32]),               # S not [64][64]
    lambda w: w.__setitem__(1, w[1][:, :255]),              # b0 not MAX_SEQ wide
    lambda w: w.__setitem__(1, np.zeros((9, MAX_SEQ))),     # nine interests
    lambda w: w.__setitem__(2, w[2][:, :64]),               # h1 64
    lambda w: w.__setitem__(3, np.zeros((1025, 128))),      # d_user 1025
    lambda w: w.__setitem__(4, w[4][:-1]),                  # b1 short
    lambda w: w.__setitem__(5, w[5][:, :32]),               # d_out 32
    lambda w: w.__setitem__(6, w[6][:-1]),                  # b2 short
    lambda w: w.__setitem__(7, 5),                          # five iterations
])
def test_pack_mind_shape_errors(change):
    w = list(weights(3, 64, 128, 7)) + [3, 0]
    change(w)
    with pytest.raises(ValueError):
        pa.pack_mind(*w)


@pytest.mark.parametrize("name", list(CASES))
def test_float32_restatement_is_under_a_quarter_of_the_bar(name):
    err = np.max(np.abs(reference(name, np.float32).astype(np.float64) - reference(name)))
    print("%s: float32 against fp64 %.3e, bar %.3e" % (name, err, BARS[name]))
    assert np.all(np.isfinite(reference(name))) and err <= BARS[name] / 4
