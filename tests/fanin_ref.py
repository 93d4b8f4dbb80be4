"""The fan-in merge's specification on the CPU: arrays → OracleItems with RetrieveId "s<k>" → o.unique_filter
(filter/unique_filter.go:26-49 restated) → the six output arrays of pg_fanin_merge_dev, padding included.  Scores never meet
arithmetic on the way: float32 sources are widened (numpy's astype, the host's conversion instruction), everything else
travels as bits."""
import struct

import numpy as np

from oracle import oracle as o

U64MAX = 0xFFFFFFFFFFFFFFFF
NAN_BITS = 0x7FF8000000000000
NEG_INF_BITS = 0xFFF0000000000000


def bits_of(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def widen(scores: np.ndarray) -> np.ndarray:
    """[nq][k] float32 or float64 → float64, float64 untouched"""
    sc = np.ascontiguousarray(scores)
    return sc if sc.dtype == np.float64 else np.ascontiguousarray(sc, dtype=np.float32).astype(np.float64)


def items_of(sources, q):
    """request q's concatenation: sources as given, entries in list order, padding dropped"""
    items = []
    for s, (rows, scores) in enumerate(sources):
        sc = widen(scores)
        for j, r in enumerate(np.asarray(rows, dtype=np.uint64)[q].tolist()):
            if r != U64MAX:
                items.append(o.OracleItem(str(r), sc[q, j], "s%d" % s))
    return items


def arrays_of(per_request, n_src, cap):
    """per_request[q] = [(id, score, source, {source: score})] in output order → the six arrays"""
    nq = len(per_request)
    rows = np.full((nq, cap), U64MAX, dtype=np.uint64)
    score = np.full((nq, cap), NEG_INF_BITS, dtype=np.uint64)
    source = np.full((nq, cap), 0xFF, dtype=np.uint8)
    planes = np.full((n_src, nq, cap), NAN_BITS, dtype=np.uint64)
    mask = np.zeros((nq, cap), dtype=np.uint32)
    count = np.zeros(nq, dtype=np.uint32)
    for q, lst in enumerate(per_request):
        count[q] = len(lst)
        for slot, (item_id, sc, src, rs) in enumerate(lst):
            rows[q, slot] = item_id
            score[q, slot] = bits_of(sc)
            source[q, slot] = src
            for k, v in rs.items():
                planes[k, q, slot] = bits_of(v)
                mask[q, slot] |= np.uint32(1 << k)
    return rows, score.view(np.float64), source, planes.view(np.float64), mask, count


def merge(sources):
    """sources = [(rows [nq][k_s] uint64, scores [nq][k_s] float32 | float64)] →
    (rows [nq][cap] u64, score [nq][cap] f64, source [nq][cap] u8, recall_scores [n][nq][cap] f64, source_mask [nq][cap] u32,
    count [nq] u32).  An item nobody duplicated has no RecallScores in the reference; its plane holds its own recall's score."""
    nq = np.asarray(sources[0][0]).shape[0]
    cap = sum(np.asarray(r).shape[1] for r, _ in sources)
    per_request = []
    for q in range(nq):
        out = []
        for it in o.unique_filter(items_of(sources, q)):
            rs = it.recall_scores if it.recall_scores is not None else {it.retrieve_id: it.score}
            out.append((int(it.id), it.score, int(it.retrieve_id[1:]), {int(k[1:]): v for k, v in rs.items()}))
        per_request.append(out)
    return arrays_of(per_request, len(sources), cap)


def same(got, want, planes=True):
    """every output array by bits"""
    names = ("rows", "score", "source", "recall_scores", "source_mask", "count")
    for i, name in enumerate(names):
        if not planes and i in (3, 4):
            assert got[i] is None, name
            continue
        g, w = np.ascontiguousarray(got[i]), np.ascontiguousarray(want[i])
        assert g.shape == w.shape and g.dtype == w.dtype, name
        if g.dtype == np.float64:
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert np.array_equal(g, w), "%s differs at %s" % (name, np.argwhere(g != w)[:4].tolist())
