"""A sequential restatement of the list recall (UserGroupHotRecall, UserGlobalHotRecall, UserTopicRecall), in plain
Python over numpy arrays, written from the specification in include/pairec_gpu.h and the reference DAOs
(module/user_group_hot_recall_hologres_dao.go:47-140, module/user_global_hot_recall_hologres_dao.go:50-149,
module/user_topic_mysql_dao.go:58-138) — not from the C++.  Slow and obvious on purpose."""
import struct

import numpy as np

GROUP, GLOBAL, TOPIC = 0, 1, 2
MAX_ENTRIES = 65536
UNSCORED, PAD_SOURCE = 0x80, 0xFF
PAD_ROW = 0xFFFFFFFFFFFFFFFF
M64 = (1 << 64) - 1


class Unsupported(Exception):
    """a request beyond MAX_ENTRIES: .request is the smallest such one"""

    def __init__(self, request):
        super().__init__("request %d" % request)
        self.request = request


def parse_item_ids(text, row_of, source_of):
    """the DAOs' item_ids text → (rows, scores, source bytes).  Entries are separated by ',', empty ones dropped
    (user_global_hot_recall_hologres_dao.go:96-101); an entry is "id" (:112-118), "id:source" (:119-129) or "id:source:score"
    (:130-141); an empty source is the recall's own name = index 0; entries of four or more parts are dropped, as the DAO's
    if / else if chain drops them.  row_of maps an item id to its local row, source_of a RetrieveId string to its index 1..126.
    utils.ToFloat(s, 0) yields 0 for text that is no number."""
    rows, scores, source = [], [], []
    for ent in text.split(","):
        if not ent:
            continue
        parts = ent.split(":")
        if len(parts) > 3:
            continue
        src = 0 if len(parts) == 1 or parts[1] == "" else source_of[parts[1]]
        assert 0 <= src <= 126
        if len(parts) == 3:
            try:
                sc = float(parts[2])
            except ValueError:
                sc = 0.0
        else:
            sc, src = 0.0, src | UNSCORED
        rows.append(row_of[parts[0]])
        scores.append(sc)
        source.append(src)
    return np.array(rows, np.uint32), np.array(scores, np.float64), np.array(source, np.uint8)


def draw(seed, p):
    """u(q, p): the splitmix64 finaliser of seed + golden * (1 + p), its top 53 bits as a double in [0, 1)"""
    x = (int(seed) + 0x9E3779B97F4A7C15 * (1 + int(p))) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return float(x >> 11) * 2.0 ** -53


def topic_quotas(values, k):
    """take_j = int64((v_j / total) * k), 0 taken as 0.5, total summed in order (user_topic_mysql_dao.go:75-77, :101-106)"""
    vs = [np.float64(0.5) if float(v) == 0.0 else np.float64(v) for v in values]
    with np.errstate(all="ignore"):                        # (a sum that overflows is +inf: every share is 0)
        total = np.float64(0.0)
        for v in vs:
            total = total + v
        return [int((v / total) * np.float64(k)) for v in vs]


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def concatenation(mode, offsets, triggers, values, k):
    """the entry indices of one request's concatenation, in order"""
    n_triggers = len(offsets) - 1
    quota = topic_quotas(values, k) if mode == TOPIC else None
    ent = []
    for j, t in enumerate(triggers):
        t = int(t)
        if t >= n_triggers:                                  # UINT32_MAX included: a trigger_id without a row
            continue
        b, e = int(offsets[t]), int(offsets[t + 1])
        if mode == TOPIC:
            e = min(e, b + quota[j])
        ent.extend(range(b, e))
    return ent


def recall(rows, row_offset, offsets, item_rows, scores, source, mode, triggers, k, values=None, seed=None):
    """→ (rows [nq][k] uint64, scores [nq][k] f64, source [nq][k] uint8, counts [nq] uint32); raises Unsupported"""
    nq = len(triggers)
    cats = [concatenation(mode, offsets, triggers[q], values[q] if mode == TOPIC else None, k) for q in range(nq)]
    for q, ent in enumerate(cats):
        if len(ent) > MAX_ENTRIES:
            raise Unsupported(q)
    o_rows = np.full((nq, k), PAD_ROW, np.uint64)
    o_sc = np.full((nq, k), -np.inf, np.float64)
    o_src = np.full((nq, k), PAD_SOURCE, np.uint8)
    o_cnt = np.zeros(nq, np.uint32)
    # (Python floats are float64: a stored score keeps its bits, -0.0 and subnormals included)
    item_rows, scores, source = np.asarray(item_rows).tolist(), np.asarray(scores, np.float64).tolist(), np.asarray(source).tolist()
    for q, ent in enumerate(cats):
        n = len(ent)
        sd = 0 if seed is None else int(seed[q])
        items = []                                           # (score, p, entry)
        for p, e in enumerate(ent):
            if source[e] & UNSCORED:
                sc = draw(sd, p) if mode == GLOBAL else 0.0
            else:
                sc = scores[e]
            items.append((sc, p, e))
        if mode == GROUP or (mode == GLOBAL and n > k):
            # score descending, then p ascending; -0.0 == 0.0 in this comparison, so the tie falls to p
            items.sort(key=lambda it: (-it[0], it[1]))
        kept = min(n, k)
        for j in range(kept):
            sc, p, e = items[j]
            o_rows[q, j] = int(row_offset) + item_rows[e]
            o_sc[q, j] = sc
            o_src[q, j] = source[e] & 0x7F
        o_cnt[q] = kept
    return o_rows, o_sc, o_src, o_cnt


def same(got, want):
    """rows, sources and counts as integers, scores as bit patterns"""
    g_rows, g_sc, g_src, g_cnt = got
    w_rows, w_sc, w_src, w_cnt = want
    assert np.array_equal(np.asarray(g_cnt, np.uint32), w_cnt), (g_cnt, w_cnt)
    assert np.array_equal(g_rows, w_rows), np.argwhere(g_rows != w_rows)[:4].tolist()
    gb, wb = np.ascontiguousarray(g_sc).view(np.uint64), np.ascontiguousarray(w_sc).view(np.uint64)
    assert np.array_equal(gb, wb), np.argwhere(gb != wb)[:4].tolist()
    if g_src is not None:
        assert np.array_equal(g_src, w_src), np.argwhere(g_src != w_src)[:4].tolist()
