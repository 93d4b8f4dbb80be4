"""A sequential restatement of the SSDSort stage's specification (include/pairec_gpu.h: pg_ssd_sort_dev): plain
Python, one entry at a time, in the steps the header numbers, on top of the oracle's ssd_quality / ssd_embeddings / ssd_window.
tests/test_ssd_stage_cpu.py holds it against a literal transcription of the Go Sort / doSort; the kernels are held against it by
bits (tests/test_gpu_ssd_stage.py)."""
import numpy as np

from oracle import oracle as o

NONE32 = 0xFFFFFFFF
PAD64 = 0xFFFFFFFFFFFFFFFF
QNAN_BITS = 0x7FF8000000000000

DEFAULTS = dict(gamma=0.25, topn=10, window=5, normalize_emb=True, ensure_pos_similarity=True, norm_quality_score=0, use_ssd_star=False,
                candidate_count=0, min_score_percent=0.0, abort_run_cnt=0, filter_source_mask=0)


def params(**kw):
    p = dict(DEFAULTS)
    for k in kw:
        assert k in p, k
    p.update(kw)
    return p


def oracle_window(emb32, quality, p):
    """SSDWithSlidingWindow behind the normalisation: the oracle's, on the cut list's table rows"""
    emb = o.ssd_embeddings(emb32, p["normalize_emb"], p["ensure_pos_similarity"])
    with np.errstate(all="ignore"):
        return [int(i) for i in o.ssd_window(emb, quality, p["gamma"], p["topn"], p["window"], p["use_ssd_star"])]


def stage_list(score, source, emb32_of, p, enable=True, window_fn=oracle_window):
    """One request over its REAL entries 0 .. n-1 (padding gone already): score[i], source[i] (or source None), emb32_of(list of
    entries) → their fp32 table rows.  → (result: entries in answer order, quality: {entry: ssd_quality_score}, picks: the window's
    pick sequence over the cut list, or None where the request was not re-ranked)"""
    n = len(score)
    every = list(range(n))
    # 1. the gates
    if not enable or (p["abort_run_cnt"] > 0 and n <= p["abort_run_cnt"]):
        return every, {}, None
    # 2. the split
    mask = p["filter_source_mask"] if source is not None else 0
    backup = [i for i in every if source is not None and int(source[i]) < 32 and (mask >> int(source[i])) & 1]
    taken = set(backup)
    selected = [i for i in every if i not in taken]
    if not selected:
        return backup, {}, None
    # 3. gamma
    if p["gamma"] == 0:
        return selected + backup, {}, None
    # 4. the cuts
    topn, cc, pct = p["topn"], p["candidate_count"], p["min_score_percent"]
    cut = selected
    if (cc > 0 or pct > 0) and len(cut) > topn:
        if cc > 0:
            cut = cut[:max(topn, cc)]
        if pct > 0 and len(cut) > topn:
            idx = len(cut)
            top = np.float64(score[cut[0]])
            for j in range(topn, len(cut)):
                with np.errstate(all="ignore"):
                    if np.float64(score[cut[j]]) / top < pct:           # (a NaN quotient does not cut)
                        idx = j
                        break
            cut = cut[:idx]
    # 5. the normalisation
    rel = np.array([score[i] for i in cut], dtype=np.float64)
    with np.errstate(all="ignore"):
        qual, ok = o.ssd_quality(rel, p["norm_quality_score"])
    if not ok:
        return cut + backup, {}, None
    quality = {cut[i]: qual[i] for i in range(len(cut))} if p["norm_quality_score"] else {}
    # 6. the window over the cut list
    picks = window_fn(emb32_of(cut), qual, p)
    # 7.
    return [cut[i] for i in picks] + backup, quality, picks


def stage(tab, row_offset, rows, score, p, order=None, source=None, count=None, enable=None, window_fn=oracle_window):
    """nq requests as pg_ssd_sort_dev takes them: tab fp32 [table rows][dim] with global row ids row_offset + i, rows / score /
    source / order [nq][cap], count / enable [nq].  → (pos [nq][cap] u32, count [nq] u32, out_rows [nq][cap] u64, quality bits
    [nq][cap] u64 by input position, picks: per request the window's pick sequence or None)"""
    rows = np.asarray(rows, dtype=np.uint64)
    nq, cap = rows.shape
    pos = np.full((nq, cap), NONE32, np.uint32)
    out_rows = np.full((nq, cap), PAD64, np.uint64)
    qbits = np.full((nq, cap), QNAN_BITS, np.uint64)
    cnt = np.zeros(nq, np.uint32)
    all_picks = []
    for q in range(nq):
        n = cap if count is None else min(int(count[q]), cap)
        elems = []
        for j in range(n):                                               # padding leaves the list first
            e = j if order is None else int(order[q, j])
            if e >= cap:
                continue
            r = int(rows[q, e])
            if r == PAD64 or r < row_offset or r - row_offset >= tab.shape[0]:
                continue
            elems.append(e)
        sc = [score[q, e] for e in elems]
        src = None if source is None else [source[q, e] for e in elems]
        res, quality, picks = stage_list(sc, src, lambda ent: tab[[int(rows[q, elems[i]]) - row_offset for i in ent]], p,
                                         enable=True if enable is None else bool(enable[q]), window_fn=window_fn)
        all_picks.append(picks)
        cnt[q] = len(res)
        for k, i in enumerate(res):
            pos[q, k] = elems[i]
            out_rows[q, k] = rows[q, elems[i]]
        for i, v in quality.items():
            qbits[q, elems[i]] = np.float64(v).view(np.uint64)
    return pos, cnt, out_rows, qbits, all_picks
