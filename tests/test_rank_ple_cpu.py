"""PG_MODEL_PLE without a GPU: the blob pa.pack_ple builds (header and length as include/pairec_gpu.h documents them), and the
scale of the GPU test's saturated case — its gate logits must reach about +-80 at BOTH levels in the fp64 reference, and the
second level's inputs are mixes whose size is not known in advance."""
import struct

import pytest

import pairec_amd as pa
from ple_ref import ple_scores
from test_gpu_rank_ple import D_USER, PARITY, inputs, weights


@pytest.mark.parametrize("shape", [(64, 1, 1, 2, 64, 2, 32), (128, 3, 2, 1, 128, 1, 64)], ids=str)
def test_pack_ple_header_and_length(shape):
    d_item, T, e_t, e_s, h_e, n_level, h_t = shape
    w = weights(*shape)
    b = pa.pack_ple(w["levels"], w["wt"], w["bt"], w["wo"], w["bo"], D_USER)
    assert struct.unpack("<8I", b[:32]) == (D_USER, d_item, T, e_t, e_s, h_e, n_level, h_t)
    floats = T * (h_e * h_t + 2 * h_t + 1)
    for lv in range(n_level):
        n_in = h_e if lv else D_USER + d_item
        floats += (T * e_t + e_s) * (n_in + 1) * h_e + T * (n_in + 1) * (e_t + e_s)
        if lv + 1 < n_level:
            floats += (n_in + 1) * (T * e_t + e_s)
    assert len(b) == 32 + 4 * floats


def test_the_saturated_case_saturates_both_levels():
    case = [c for c in PARITY if c[7] == "saturated"][0]
    trace = {}
    ple_scores(weights(*case), D_USER, *inputs(case[0]), trace=trace)
    print("largest |gate logit| per level:", trace)
    assert 60 <= trace[0] <= 100 and 60 <= trace[1] <= 100
