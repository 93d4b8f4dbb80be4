"""CPU tests of the SSDSort stage (include/pairec_gpu.h: pg_ssd_sort_dev).  No GPU needed.

(a) the header declares pg_ssd_sort_dev, the library exports it and _lib.EXPORTS lists it;
(b) a literal transcription of the Go Sort / doSort (sort/ssd_sort.go:110-343: item lists, items[:cnt], the `for ; idx < len`
    loop) and of the normalisation in front of the window (:366-391, gonum's stat.PopMeanVariance / StdScore spelled out operation
    by operation) against tests/ssd_stage_ref.py, which states the answer in the header's steps on top of the oracle — on seeded
    random small cases with pairwise distinct scores and on hand cases at every branch.  The window loop itself (:393-486) is the
    oracle's in both; tests/test_gpu_ssd.py is its check.

Go's sort.Sort is unstable; the transcription sorts stably, which with pairwise distinct scores is the same thing, and with the
hand cases' equal scores keeps the order that arrived — what the stage defines (the header says why)."""
import ctypes as C
import os
import re

import numpy as np

from pairec_amd import _lib

import ssd_stage_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TAB, DIM = 40, 8
TAB = (np.random.default_rng(5).standard_normal((4, DIM))[np.random.default_rng(6).integers(0, 4, N_TAB)]
       + 0.2 * np.random.default_rng(7).standard_normal((N_TAB, DIM))).astype(np.float32)
F = np.float64


def test_header_library_and_binding_carry_the_symbol():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pairec_gpu.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+pg_ssd_sort_dev\s*\(", src)
    assert hasattr(C.CDLL(_lib.LIB_PATH), "pg_ssd_sort_dev")
    assert "pg_ssd_sort_dev" in _lib.EXPORTS


# ---- the Go code, line by line ---------------------------------------------------------------------------------------------------
class _Item:
    def __init__(self, ident, score, retrieve_id, row):
        self.id, self.score, self.retrieve_id, self.row, self.algo = ident, F(score), retrieve_id, row, {}


def _sort_desc(items):
    items.sort(key=lambda it: -it.score)                                 # gosort.Sort(gosort.Reverse(ItemScoreSlice(..)))


def _pop_mean_variance(x):
    """stat.PopMeanVariance(x, nil): Mean, then the two-pass variance with the compensation term"""
    n = F(len(x))
    s = F(0.0)
    for v in x:
        s = s + v
    mean = s / n
    ss, comp = F(0.0), F(0.0)
    for v in x:
        d = v - mean
        ss = ss + d * d
        comp = comp + d
    return mean, (ss - comp * comp / n) / n


def _go_window(items, p, ctx_size):
    """SSDWithSlidingWindow :346-391 literally, :393-486 through the oracle"""
    relevance = [it.score for it in items]
    do_norm = p["norm_quality_score"]
    with np.errstate(all="ignore"):
        if do_norm == 1:
            mean, variance = _pop_mean_variance(relevance)
            if mean == 0 or variance == 0:
                return items
            std = np.sqrt(variance)
            for i, x in enumerate(relevance):
                relevance[i] = (x - mean) / std                          # stat.StdScore
                items[i].algo["ssd_quality_score"] = relevance[i]
        elif do_norm == 2:
            max_score, min_score = relevance[0], relevance[len(items) - 1]
            span = max_score - min_score
            if span == 0:
                return items
            eps = F(1e-6)
            for i, x in enumerate(relevance):
                relevance[i] = ((x - min_score) / span) * (1 - eps) + eps
                items[i].algo["ssd_quality_score"] = relevance[i]
    picks = ref.oracle_window(TAB[[it.row for it in items]], np.array(relevance, dtype=F), dict(p, topn=ctx_size))
    return [items[i] for i in picks]


def _go_do_sort(items, p, ctx_size):
    if len(items) == 0:
        return items
    _sort_desc(items)
    gamma = p["gamma"]
    if gamma == 0:
        return items
    candidate_cnt, min_score_percent = p["candidate_count"], p["min_score_percent"]
    if (candidate_cnt > 0 or min_score_percent > 0) and len(items) > ctx_size:
        if candidate_cnt > 0:
            cnt = max(ctx_size, candidate_cnt)
            if cnt < len(items):
                items = items[:cnt]
        if min_score_percent > 0 and len(items) > ctx_size:
            idx = ctx_size
            max_score = items[0].score
            while idx < len(items):
                with np.errstate(all="ignore"):
                    percent = items[idx].score / max_score
                if percent < min_score_percent:
                    break
                idx += 1
            items = items[:idx]
    return _go_window(items, p, ctx_size)


def _go_sort(candidates, p, ctx_size, condition_holds, filter_retrieve_ids):
    if len(candidates) == 0:
        return candidates
    if not condition_holds:
        _sort_desc(candidates)
        return candidates
    if p["abort_run_cnt"] > 0 and len(candidates) <= p["abort_run_cnt"]:
        _sort_desc(candidates)
        return candidates
    if filter_retrieve_ids is not None and len(filter_retrieve_ids) > 0:
        backup, selected = [], []
        for item in candidates:
            if item.retrieve_id in filter_retrieve_ids:
                backup.append(item)
            else:
                selected.append(item)
        result = _go_do_sort(selected, p, ctx_size)
        if len(backup) > 0:
            result = result + backup
    else:
        result = _go_do_sort(candidates, p, ctx_size)
    return result


# ---- one request both ways -------------------------------------------------------------------------------------------------------
def both(score, p, source=None, rows=None, enable=True):
    """score (in list order), source, rows of TAB for one request → asserts the restatement equals the transcription; returns the
    answer (entries in order) and whether it was re-ranked"""
    n = len(score)
    rows = list(range(n)) if rows is None else rows
    ids = [s for s in range(32) if (p["filter_source_mask"] >> s) & 1] if source is not None else []
    items = [_Item(i, score[i], None if source is None else int(source[i]), rows[i]) for i in range(n)]
    got_items = _go_sort(items, p, p["topn"], enable, ids)
    res, quality, picks = ref.stage_list([F(s) for s in score], source, lambda ent: TAB[[rows[i] for i in ent]], p, enable=enable)
    assert [it.id for it in got_items] == res
    go_quality = {it.id: it.algo["ssd_quality_score"] for it in items if "ssd_quality_score" in it.algo}
    # (a request that bails has recorded nothing: both bail-outs come before the first AddAlgoScore)
    assert sorted(go_quality) == sorted(quality)
    for i in quality:
        assert F(quality[i]).view(np.uint64) == F(go_quality[i]).view(np.uint64)
    return res, picks is not None


def test_random_small_cases_equal_the_transcription():
    rng = np.random.default_rng(20240607)
    reranked = cut = 0
    for _ in range(4000):
        n = int(rng.integers(0, 15))
        score = np.sort(rng.choice(np.arange(1, 400), n, replace=False) / 97.0 - (1.5 if rng.random() < 0.2 else 0.0))[::-1]
        assert len(set(score.tolist())) == n
        source = rng.integers(0, 5, n) if rng.random() < 0.7 else None
        p = ref.params(gamma=float(rng.choice([0.0, 0.25, 0.25, 0.25])), topn=int(rng.integers(1, 8)), window=int(rng.choice([0, 2, 3, 5])),
                       norm_quality_score=int(rng.integers(0, 3)), use_ssd_star=bool(rng.integers(0, 2)),
                       candidate_count=int(rng.choice([0, 0, 2, 5, 9])), min_score_percent=float(rng.choice([0.0, 0.0, 0.4, 0.8])),
                       abort_run_cnt=int(rng.choice([0, 0, 0, 4])), filter_source_mask=int(rng.integers(0, 32)) if rng.random() < 0.6 else 0)
        rows = rng.choice(N_TAB, n, replace=False).tolist()
        res, rr = both(score.tolist(), p, source, rows, enable=rng.random() < 0.9)
        reranked += rr
        cut += rr and len(res) < n
    assert reranked > 1000 and cut > 200                                 # the cases reach the window and the cuts


DESC = [9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0, 0.5]


def test_candidate_count_below_topn_cuts_to_topn():
    res, rr = both(DESC, ref.params(topn=4, candidate_count=2))
    assert rr and len(res) == 4


def test_a_list_no_longer_than_topn_is_not_cut():
    res, rr = both(DESC[:4], ref.params(topn=4, candidate_count=2, min_score_percent=0.99))
    assert rr and sorted(res) == [0, 1, 2, 3]
    res, rr = both(DESC[:3], ref.params(topn=4, candidate_count=2, min_score_percent=0.99))
    assert rr and sorted(res) == [0, 1, 2]


def test_min_percent_cut_landing_exactly_at_topn():
    # score[4] / score[0] = 5 / 9 < 0.6 at idx = topn: four entries remain, all of them picked
    res, rr = both(DESC, ref.params(topn=4, min_score_percent=0.6))
    assert rr and sorted(res) == [0, 1, 2, 3]
    # ... and one behind it
    res, rr = both(DESC, ref.params(topn=4, min_score_percent=0.5))
    assert rr and len(res) == 4 and set(res) <= {0, 1, 2, 3, 4}


def test_a_negative_top_score_turns_the_quotient_round():
    # every quotient is >= 1 below a negative top score: nothing is cut although the scores fall
    neg = [-1.0, -2.0, -3.0, -4.0, -5.0, -6.0]
    res, rr = both(neg, ref.params(topn=2, min_score_percent=0.5, gamma=0.25))
    assert rr and len(res) == 2
    # ... and a bound above 1 cuts where a quotient stays below it: -2 / -1 = 2 < 2.5 at idx = topn
    res, rr = both(neg, ref.params(topn=1, min_score_percent=2.5))
    assert rr and res == [0]


def test_a_nan_quotient_does_not_cut():
    zeros = [0.0] * 6                                                    # 0 / 0 at every idx: no cut, six candidates, three picks
    res, rr = both(zeros, ref.params(topn=3, min_score_percent=0.5))
    assert rr and len(res) == 3
    inf = [float("inf"), float("inf"), 1.0, 0.5]                         # inf / inf, then 1 / inf = 0 < 0.5 cuts at idx 2
    res, rr = both(inf, ref.params(topn=1, min_score_percent=0.5))
    assert rr and res == [0]


def test_mode_1_on_all_zero_scores_bails():
    res, rr = both([0.0] * 7, ref.params(topn=3, norm_quality_score=1, candidate_count=5), source=[0, 1, 0, 0, 1, 0, 0])
    assert not rr and res == [0, 1, 2, 3, 4]                             # the CUT list unchanged
    res, rr = both([0.0] * 7, ref.params(topn=3, norm_quality_score=1, candidate_count=5, filter_source_mask=2), source=[0, 1, 0, 0, 1, 0, 0])
    assert not rr and res == [0, 2, 3, 5, 6, 1, 4]                       # ... and the backup behind it
    res, rr = both([2.5] * 7, ref.params(topn=3, norm_quality_score=1))  # variance 0, mean not
    assert not rr and res == list(range(7))
    res, rr = both([3.0, 1.0, -1.0, -3.0], ref.params(topn=3, norm_quality_score=1))      # mean 0, variance not
    assert not rr and res == [0, 1, 2, 3]


def test_mode_2_on_all_equal_scores_bails():
    res, rr = both([0.75] * 6, ref.params(topn=3, norm_quality_score=2))
    assert not rr and res == list(range(6))
    res, rr = both([0.75] * 6, ref.params(topn=3, norm_quality_score=2, candidate_count=4, filter_source_mask=1), source=[0, 1, 1, 1, 1, 1])
    assert not rr and res == [1, 2, 3, 4, 0]                             # the cut list, then the backup


def test_abort_run_cnt_at_its_boundary():
    res, rr = both(DESC[:6], ref.params(topn=3, abort_run_cnt=6, candidate_count=4))
    assert not rr and res == list(range(6))
    res, rr = both(DESC[:7], ref.params(topn=3, abort_run_cnt=6, candidate_count=4))
    assert rr and len(res) == 3


def test_a_request_whose_entries_all_go_to_backup():
    res, rr = both(DESC[:5], ref.params(topn=3, filter_source_mask=0b1010), source=[1, 3, 3, 1, 1])
    assert not rr and res == [0, 1, 2, 3, 4]


def test_gamma_zero_keeps_selected_and_appends_backup():
    res, rr = both(DESC[:6], ref.params(topn=2, gamma=0.0, candidate_count=3, filter_source_mask=0b1), source=[1, 0, 1, 0, 1, 1])
    assert not rr and res == [0, 2, 4, 5, 1, 3]                          # no cut either: gamma is looked at first


def test_the_batch_form_drops_padding_first_and_reports_element_positions():
    """ref.stage: count, order values beyond cap, UINT64_MAX rows and rows outside the table are padding; positions are elements"""
    rows = np.array([[103, ref.PAD64, 105, 100 + N_TAB + 2, 107, 109, 111, 102]], dtype=np.uint64)      # global rows 100 .. 100 + N_TAB - 1
    score = np.array([[1.0, 9.0, 3.0, 8.0, 5.0, 6.0, 7.0, 2.0]])
    order = np.array([[6, 1, 5, 9, 4, 3, 2, 0]], dtype=np.uint32)        # descending by score; 9 is beyond cap; 7 is behind the count
    p = ref.params(topn=2, gamma=0.0)
    pos, cnt, out_rows, qbits, rr = ref.stage(TAB, 100, rows, score, p, order=order, count=np.array([7]))
    assert cnt[0] == 4 and pos[0, :4].tolist() == [6, 5, 4, 2] and (pos[0, 4:] == ref.NONE32).all()
    assert out_rows[0, :4].tolist() == [111, 109, 107, 105] and (out_rows[0, 4:] == ref.PAD64).all()
    assert (qbits == ref.QNAN_BITS).all() and rr[0] is None
