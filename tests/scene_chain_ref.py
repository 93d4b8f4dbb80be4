"""A scene's device stages composed on the CPU: the existing restatements, one after the other, in the order a scene enqueues the
`_dev` entries (include/pairec_gpu.h), returning the arrays after EVERY stage so that a comparison can name the first stage that
diverges.  No new arithmetic: each stage's answer stays defined where it is defined today.

  list stages   fanin_ref.merge → cond_ref.item_state_filter → trim_ref.trim → blend_ref.blend → dimcap_ref.dimcap →
                classcut_ref.masks + classcut_ref.classcut → trim2_ref.trim2; the fan-in's planes (RecallScores), source mask and
                count and one fp32 plane travel through all of them
  sort stages   on trim2's lists: cond_ref.boost_requests (on the device in place, d_out_score == d_score) → oracle.sort_scores per
                request over the whole width (padding's -inf included, as pg_sort_scores_dev over uniform segments) →
                dimcap_ref.distinct_ids_array → mixsort_ref.mix_sort on the sort's order → ssd_stage_ref.stage on the mix's order
                and count with the boosted scores
  side branch   diversity_ref.diversity_rules on trim2's rows (the store's integer columns), count and source

run() → {stage: {array: numpy array}} in STAGES' order.  A key that starts with "_" is bookkeeping, not an output.  Because the
boost runs in place, trim2's score buffer holds the boosted scores when a device chain is read back: a device result leaves
("trim2", "score") out (IN_PLACE) and the buffer is checked as the boost's output — padding keeps its bits there, so the padding
trim2 wrote is checked all the same."""
from collections import OrderedDict

import numpy as np

import blend_ref
import classcut_ref
import cond_ref
import dimcap_ref
import diversity_ref
import fanin_ref
import mixsort_ref
import ssd_stage_ref
import trim2_ref
import trim_ref
from oracle import oracle as o
from scene_chain_cases import CLASS_TREES, DIV_COLS, RECALLS, STORE_ROWS, table

LIST_ARRAYS = ("rows", "score", "source", "planes_f64", "source_mask", "planes_f32", "count")
STAGES = ("fanin", "filter", "trim", "blend", "dimcap", "classcut", "trim2", "boost", "sort", "distinct", "mix", "ssd", "diversity")
LIST_STAGES = STAGES[:7]
IN_PLACE = {("trim2", "score")}


def lists(d):
    """a list stage's arrays in the order the restatements take them"""
    return d["rows"], d["score"], d["source"], d["count"], d["planes_f64"], d["source_mask"], d["planes_f32"]


def as_stage(t):
    return dict(zip(LIST_ARRAYS, t))


def gather(w, rows):
    """the store's columns at rows of any shape → ({name: values, rows' shape}, item_in); a row outside reads row 0 and item_in 0"""
    rows = np.asarray(rows, np.uint64)
    inside = rows < np.uint64(STORE_ROWS)
    idx = np.where(inside, rows, 0).astype(np.int64)
    return {k: v[idx] for k, v in w.store.items()}, inside


# ---- the stages: f(w, b, cfg, r) → {array: value}, r the results so far ---------------------------------------------------------
def fanin(w, b, cfg, r):
    rows, score, source, planes, mask, count = fanin_ref.merge(b.sources)
    return dict(rows=rows, score=score, source=source, planes_f64=planes, source_mask=mask, count=count)


def filter_(w, b, cfg, r):
    f = r["fanin"]
    return as_stage(cond_ref.item_state_filter(cfg.filter[0]["Conditions"], w.store, STORE_ROWS, f["rows"], f["score"], f["source"], f["count"],
                                               f["planes_f64"], f["source_mask"], b.p32, users=b.users))


def trim(w, b, cfg, r):
    return as_stage(trim_ref.trim(cfg.trim, *lists(r["filter"])))


def blend(w, b, cfg, r):
    return as_stage(blend_ref.blend(cfg.blend, *lists(r["trim"])))


def dimcap(w, b, cfg, r):
    d = r["blend"]
    column, limit, null_mode, null_value = cfg.dimcap
    cols, inside = gather(w, d["rows"])
    return as_stage(dimcap_ref.dimcap(cols[column].astype(np.int64), inside.astype(np.uint8), limit, null_mode, null_value, *lists(d)))


def class_masks(w, d):
    """[nq][cap] uint8: the class bits of a stage's entries"""
    cols, inside = gather(w, d["rows"])
    nq, cap = d["rows"].shape
    return np.stack([classcut_ref.masks(CLASS_TREES, cap, {k: v[q] for k, v in cols.items()}, inside[q], d["score"][q], d["source"][q], RECALLS)
                     for q in range(nq)])


def classcut(w, b, cfg, r):
    d = r["dimcap"]
    out = as_stage(classcut_ref.classcut(cfg.class_rules, d["rows"], d["score"], class_masks(w, d), d["source"], d["count"], d["planes_f64"],
                                         d["source_mask"], d["planes_f32"]))
    return out


def trim2(w, b, cfg, r):
    return as_stage(trim2_ref.trim2(cfg.trim2, *lists(r["classcut"])))


def boost(w, b, cfg, r):
    d = r["trim2"]
    bits, rule = cond_ref.boost_requests(cfg.boost, False, w.store, STORE_ROWS, d["rows"], d["score"], d["count"], b.users)
    return dict(score=np.ascontiguousarray(bits).view(np.float64), rule=rule)


def sort(w, b, cfg, r):
    sc = r["boost"]["score"]
    return dict(order=np.stack([np.asarray(o.sort_scores(sc[q], True), np.uint32) for q in range(sc.shape[0])]))


def distinct_match(w, b, cfg, d):
    """[nq][n_rules][cap] bool: rule r's FilterParam on entry p"""
    cols, inside = gather(w, d["rows"])
    nq, cap = d["rows"].shape
    return np.array([[[cond_ref.match(ru["Conditions"], p, {k: v[q] for k, v in cols.items()}, inside[q], b.users[q]) for p in range(cap)]
                      for ru in cfg.distinct] for q in range(nq)], dtype=bool)


def distinct(w, b, cfg, r):
    d = r["trim2"]
    m = distinct_match(w, b, cfg, d)
    live = dimcap_ref.live_mask(d["rows"], d["count"])
    return dict(ids=np.stack([dimcap_ref.distinct_ids_array(m[q], cfg.distinct_ids, live[q]) for q in range(m.shape[0])]).astype(np.int64))


def mix(w, b, cfg, r):
    d = r["trim2"]
    cols, inside = gather(w, d["rows"])
    nq, cap = d["rows"].shape
    order, count = mixsort_ref.mix_sort(cfg.mix, cfg.mix_size, cfg.mix_remain, cfg.ctx_size, nq, cap, cols=cols, item_in=inside, source=d["source"],
                                        order=r["sort"]["order"], count=d["count"], seed=b.seeds, users=b.users, recall_names=RECALLS)
    return dict(order=order, count=count)


def ssd(w, b, cfg, r):
    d = r["trim2"]
    pos, cnt, out_rows, qbits, picks = ssd_stage_ref.stage(table(w), 0, d["rows"], r["boost"]["score"], ssd_stage_ref.params(**cfg.ssd),
                                                           order=r["mix"]["order"], source=d["source"], count=r["mix"]["count"], enable=b.enable)
    return dict(pos=pos, count=cnt, rows=out_rows, quality=qbits.view(np.float64), _picks=picks)


def div_planes(w, d):
    """[n_cols][nq][cap] int64: DIV_COLS at the entries' rows, the column default outside the store"""
    cols, inside = gather(w, d["rows"])
    return np.stack([np.where(inside, cols[c].astype(np.int64), np.int64(w.defaults[c])) for c in DIV_COLS])


def diversity(w, b, cfg, r):
    d = r["trim2"]
    return dict(order=diversity_ref.diversity_rules(cfg.div, div_planes(w, d), count=d["count"], source=d["source"], enable=b.enable))


REF = dict(fanin=fanin, filter=filter_, trim=trim, blend=blend, dimcap=dimcap, classcut=classcut, trim2=trim2, boost=boost, sort=sort,
           distinct=distinct, mix=mix, ssd=ssd, diversity=diversity)


def run(w, b, cfg=None, impl=None):
    """the whole chain for batch b → {stage: {array: value}}; cfg replaces the batch's scene (a perturbed rule), impl replaces
    stage functions ({stage: f}: the library's host statements in tests/test_scene_chain_cpu.py)"""
    cfg = b.cfg if cfg is None else cfg
    r = OrderedDict()
    for name in STAGES:
        r[name] = (impl or {}).get(name, REF[name])(w, b, cfg, r)
    return r


# ---- comparison by bits --------------------------------------------------------------------------------------------------------
def as_bits(stage, name, a):
    """an output array as unsigned integers of its element width.  One fold, cond_ref.score_bits': the default NaN an invalid
    operation GENERATES in a boost expression has a platform-defined sign; only the boost's scores pass through it"""
    a = np.ascontiguousarray(a)
    u = a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    return cond_ref.score_bits(u) if (stage, name) == ("boost", "score") else u


def first_difference(got, want, absent=()):
    """the first (stage, array, element) in STAGES' order at which two results differ, by bits, padding included → None, or a dict
    {stage, array, request, slot, plane, got, want}; a missing or misshapen array is a difference of its own.  absent: (stage,
    array) pairs `got` is allowed to leave out (IN_PLACE for a device chain)"""
    for stage in STAGES:
        for name, wa in want[stage].items():
            if name.startswith("_") or wa is None or (stage, name) in absent and name not in got[stage]:
                continue
            ga = got[stage].get(name)
            if ga is None or np.asarray(ga).shape != wa.shape or np.asarray(ga).dtype.itemsize != wa.dtype.itemsize:
                return dict(stage=stage, array=name, request=None, slot=None, plane=None, got=None if ga is None else np.asarray(ga).shape,
                            want=wa.shape)
            g, x = as_bits(stage, name, ga), as_bits(stage, name, wa)
            bad = np.argwhere(g != x)
            if bad.size:
                i = tuple(int(v) for v in bad[0])
                plane, request, slot = (i[0], i[1], i[2]) if len(i) == 3 else (None, i[0], i[1] if len(i) == 2 else None)
                return dict(stage=stage, array=name, request=request, slot=slot, plane=plane, got=hex(int(g[i])), want=hex(int(x[i])))
    return None


def describe(diff, batch=""):
    """a failure message that names batch, stage, array, request and slot"""
    if diff is None:
        return "equal"
    where = "request %s slot %s" % (diff["request"], diff["slot"]) + ("" if diff["plane"] is None else " plane %d" % diff["plane"])
    return "batch %s: stage %s, array %s, %s: device %s, reference %s" % (batch, diff["stage"], diff["array"], where, diff["got"], diff["want"])
