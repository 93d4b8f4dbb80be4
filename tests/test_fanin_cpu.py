"""CPU checks behind the fan-in merge: tests/fanin_ref.py — the specification the GPU tests compare with — reads
UniqueFilter as the host mirror does (ph_unique_filter, the line-for-line rendering of filter/unique_filter.go:26-49): Item.Score
and RetrieveId from the FIRST occurrence, RecallScores[recall] from that recall's LAST one; and the limits the header states are
the ones csrc/fanin.hip is built with."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import fanin_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64MAX = ref.U64MAX


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(os.environ.get("PH_HOST_LIB") or os.path.join(ROOT, "pairec_amd", "libpairec_host.so"))
    L.ph_unique_filter.restype = C.c_char_p
    L.ph_unique_filter.argtypes = [C.c_char_p]
    return L


def mirror_merge(H, sources):
    """the six arrays from ph_unique_filter's answer; an item's source is looked up in the input, which the mirror does not echo"""
    nq = sources[0][0].shape[0]
    cap = sum(r.shape[1] for r, _ in sources)
    per_request = []
    for q in range(nq):
        items, first = [], {}
        for s, (rows, scores) in enumerate(sources):
            sc = ref.widen(scores)
            for j, r in enumerate(rows[q].tolist()):
                if r == U64MAX:
                    continue
                items.append({"id": str(r), "score": float(sc[q, j]), "retrieve_id": "s%d" % s, "algo_scores": {}})
                first.setdefault(str(r), s)
        out = json.loads(H.ph_unique_filter(json.dumps(items).encode()))
        lst = []
        for it in out:
            src = first[it["id"]]
            rs = {int(k[1:]): float(v) for k, v in it["recall_scores"].items()} or {src: float(it["score"])}
            lst.append((int(it["id"]), float(it["score"]), src, rs))
        per_request.append(lst)
    return ref.arrays_of(per_request, len(sources), cap)


def random_sources(rng, nq, ks, universe, pad=0.1):
    """ids from a small universe (duplicates across AND inside the sources), padding sprinkled in, dyadic scores (exact in JSON)"""
    src = []
    for i, k in enumerate(ks):
        rows = (rng.integers(0, universe, (nq, k)) + 1000).astype(np.uint64)
        rows[rng.random((nq, k)) < pad] = U64MAX
        sc = rng.integers(-4096, 4096, (nq, k)) / 64.0
        src.append((rows, sc.astype(np.float32) if i % 2 == 0 else sc.astype(np.float64)))
    return src


@pytest.mark.parametrize("seed,ks,universe", [(1, [7], 4), (2, [5, 9], 8), (3, [20, 1, 33], 25), (4, [6] * 8, 12), (5, [40, 40, 40], 1000)])
def test_fanin_ref_reads_unique_filter_as_the_host_mirror_does(H, seed, ks, universe):
    rng = np.random.default_rng(seed)
    src = random_sources(rng, 5, ks, universe)
    src[-1][0][:] = src[-1][0] if len(ks) == 1 else U64MAX          # (several sources: the last one is padding only)
    src[0][0][4] = U64MAX                                            # request 4 of source 0: nothing but padding
    ref.same(ref.merge(src), mirror_merge(H, src))


def test_first_score_and_last_in_source_recall_score(H):
    """id 7: twice in source 0 (scores 1, 2), three times in source 1 (3, 4, 5); id 9 twice in source 1 only; id 8 once"""
    src = [(np.array([[7, 8, 7]], np.uint64), np.array([[1.0, 1.5, 2.0]], np.float32)),
           (np.array([[7, 9, 7, 9, 7]], np.uint64), np.array([[3.0, 6.0, 4.0, 6.5, 5.0]], np.float64))]
    rows, score, source, planes, mask, count = ref.merge(src)
    assert count.tolist() == [3] and rows[0, :3].tolist() == [7, 8, 9] and rows[0, 3] == U64MAX
    assert score[0, :3].tolist() == [1.0, 1.5, 6.0] and np.isneginf(score[0, 3:]).all()
    assert source[0, :4].tolist() == [0, 0, 1, 0xFF]
    assert planes[0, 0, :2].tolist() == [2.0, 1.5] and planes[1, 0, [0, 2]].tolist() == [5.0, 6.5]
    assert np.isnan(planes[0, 0, 2]) and np.isnan(planes[1, 0, 1]) and np.isnan(planes[:, 0, 3:]).all()
    assert planes.view(np.uint64)[0, 0, 2] == ref.NAN_BITS
    assert mask[0, :4].tolist() == [3, 1, 2, 0]
    ref.same(ref.merge(src), mirror_merge(H, src))


def test_header_constants_are_the_kernels():
    with open(os.path.join(ROOT, "include", "pairec_gpu.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "pairec_amd", "csrc", "fanin.hip")) as f:
        hip = f.read()
    for macro, const in (("PG_FANIN_MAX_SOURCES", "kFaninMaxSources"), ("PG_FANIN_MAX_CAP", "kFaninMaxCap"),
                         ("PG_FANIN_LDS_MAX_CAP", "kFaninLdsMaxCap"), ("PG_FANIN_CHUNK", "kFaninChunk")):
        h = re.search(r"#define\s+%s\s+(\d+)" % macro, hdr)
        k = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % const, hip)
        assert h and k and int(h.group(1)) == int(k.group(1)), macro
    assert re.search(r"fanin_lds_max_cap.*8192", hdr)
