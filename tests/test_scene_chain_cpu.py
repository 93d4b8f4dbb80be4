"""The scene chain without a GPU (tests/scene_chain_cases.py, tests/scene_chain_ref.py):

  * the fixtures cannot pass a chain test vacuously — for every shape every stage changes some request's list, none empties every
    request, there is a short count, padding inside a list and an entry two recalls hold, and SSD fills a page;
  * the composed Python reference equals the same chain through the library's host statements, bit for bit after every stage —
    pg_candidates_blend_host, pg_candidates_dimcap_host, pg_classcut_masks_host + pg_candidates_classcut_host,
    pg_candidates_trim2_host, pg_boost_scores_host, pg_distinct_ids_host, pg_mix_sort_host, pg_diversity_rules_host, each fed by the
    host statement before it (the stages without one — fan-in, ItemStateFilter, the trim, the sort, SSD — are the reference's);
  * the comparison names the stage whose rule was perturbed, and no earlier one."""
import copy

import numpy as np
import pytest

import pairec_amd as pa
import scene_chain_cases as cases
import scene_chain_ref as ref
from dimcap_ref import live_mask

SHAPE_NAMES = ("small", "mid", "large")
PAD = cases.U64MAX


@pytest.fixture(scope="module")
def world():
    return cases.world()


@pytest.fixture(scope="module")
def chains(world):
    """{shape: (batch, reference result)}, computed once"""
    out = {}
    for shape in SHAPE_NAMES:
        b = cases.batch(shape, cases.BATCH_SEEDS[shape])
        out[shape] = (b, ref.run(world, b))
    return out


def live_rows(d, q):
    """request q's real rows of a list stage, in order"""
    return d["rows"][q][live_mask(d["rows"], d["count"])[q]].tolist()


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_every_stage_changes_some_list_and_none_empties_all(chains, shape):
    b, r = chains[shape]
    nq = b.nq
    changed = {}
    # fan-in: a request whose union is shorter than its concatenation (UniqueFilter dropped something)
    real = np.sum([(rows != PAD).sum(axis=1) for rows, _ in b.sources], axis=0)
    changed["fanin"] = bool(np.any(r["fanin"]["count"] < real))
    prev = "fanin"
    for st in ref.LIST_STAGES[1:]:
        changed[st] = any(live_rows(r[st], q) != live_rows(r[prev], q) for q in range(nq))
        prev = st
    t2 = r["trim2"]
    live = live_mask(t2["rows"], t2["count"])
    changed["boost"] = bool(np.any((r["boost"]["score"].view(np.uint64) != t2["score"].view(np.uint64)) & live))
    ident = np.arange(t2["rows"].shape[1], dtype=np.uint32)
    n_of = [int(c) for c in t2["count"]]
    changed["sort"] = any(not np.array_equal(r["sort"]["order"][q, :n_of[q]], ident[:n_of[q]]) for q in range(nq))
    changed["distinct"] = bool(np.any((r["distinct"]["ids"] != (ident + 1).astype(np.int64)[None, :]) & live))
    changed["mix"] = any(not np.array_equal(r["mix"]["order"][q, :n_of[q]], r["sort"]["order"][q, :n_of[q]]) for q in range(nq))
    picks = r["ssd"]["_picks"]
    changed["ssd"] = any(p is not None and p != list(range(len(p))) for p in picks)
    changed["diversity"] = any(not np.array_equal(r["diversity"]["order"][q, :n_of[q]], ident[:n_of[q]]) for q in range(nq))
    assert all(changed[st] for st in ref.STAGES), {k: v for k, v in changed.items() if not v}
    for st in ref.STAGES:
        if "count" in r[st]:
            assert int(r[st]["count"].max()) > 0, "%s empties every request" % st
    # a boost that matched, a filter that kept and dropped inside the store and outside it
    assert np.any(r["boost"]["rule"][live] != 0xFF) and np.any(r["boost"]["rule"][live] == 0xFF)
    # SSD fills a page: at least topn picks for at least one request, and (but for small) one request the gate leaves alone
    assert any(p is not None and len(p) >= b.cfg.ssd["topn"] for p in picks)
    assert shape == "large" or any(p is None for p in picks)


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_short_counts_padding_and_shared_entries(chains, shape):
    b, r = chains[shape]
    # padding inside a recall's list: a UINT64_MAX with a real row behind it, in every source
    for rows, _ in b.sources:
        assert any(np.any(rows[q] == PAD) and np.flatnonzero(rows[q] == PAD)[0] < np.flatnonzero(rows[q] != PAD)[-1] for q in range(b.nq))
    # duplicates inside a source, overlap between the sources
    assert any(len(set(rows[q].tolist())) < rows.shape[1] - int((rows[q] == PAD).sum()) for rows, _ in b.sources for q in range(b.nq))
    # NaN, +0 and -0 scores and ties arrive
    sc = np.concatenate([np.asarray(s, np.float64).reshape(-1) for _, s in b.sources])
    assert np.isnan(sc).any() and np.any((sc == 0) & np.signbit(sc)) and np.any((sc == 0) & ~np.signbit(sc))
    assert np.unique(sc[~np.isnan(sc)]).size < 0.7 * sc.size                # (40 % of the scores come from five values)
    assert b.sources[1][1].dtype == np.float64 and b.sources[0][1].dtype == np.float32
    # every list stage is entered with a count below its cap by some request, and with an entry that two recalls hold
    prev = "fanin"
    for st in ref.LIST_STAGES[1:]:
        d = r[prev]
        cap = d["rows"].shape[1]
        assert np.any(d["count"] < cap) and np.any(d["count"] > 0), st
        held_twice = (d["source_mask"] & (d["source_mask"] - 1)) != 0
        assert np.any(held_twice & live_mask(d["rows"], d["count"])), "no entry of two recalls goes into %s" % st
        prev = st
    # candidates' rows reach past the store, and some lie inside it, into every stage that reads it
    for st in ("fanin", "blend", "dimcap", "trim2"):
        rows = r[st]["rows"][live_mask(r[st]["rows"], r[st]["count"])]
        assert np.any(rows < cases.STORE_ROWS) and np.any(rows >= cases.STORE_ROWS), st


def test_the_shapes_cross_the_tier_boundaries(chains):
    """the constants are the sources': a chunk of 1 024 positions; fan-in's LDS tier 8 192, the one-workgroup sort 8 192, blend's LDS
    list 2 064, dimcap's LDS tier 6 144; DiversityRuleSort's and SSD's 8 192, the mix size 4 096"""
    width = {shape: {st: chains[shape][1][st]["rows"].shape[1] for st in ref.LIST_STAGES} for shape in SHAPE_NAMES}
    assert all(w > 1024 for w in width["mid"].values())
    assert int(chains["mid"][1]["fanin"]["count"].max()) > 1024          # a list that is longer than one chunk, not only wider
    lg = width["large"]
    assert lg["fanin"] > 8192 and lg["trim"] > 2064 and lg["blend"] > pa.DIMCAP_LDS_MAX_CAP and lg["trim2"] <= pa.DIV_MAX_N
    assert chains["large"][0].cfg.mix_size <= pa.MIX_MAX_SIZE
    assert int(chains["large"][1]["blend"]["count"].max()) > 2064


# ---- the reference against the library's host statements ------------------------------------------------------------------------
def host_impl(world):
    """{stage: f} for the stages that have a pure host statement in the library, and the compiled sets to free"""
    sets = dict(boost=pa.Cond(cases.BOOST, cases.DECL, boost=True), distinct=pa.Cond(cases.DISTINCT, cases.DECL))

    def blend(w, b, cfg, r):
        return ref.as_stage(pa.candidates_blend_host(cfg.blend, *ref.lists(r["trim"])))

    def dimcap(w, b, cfg, r):
        d = r["blend"]
        cols, inside = ref.gather(w, d["rows"])
        return ref.as_stage(pa.candidates_dimcap_host((None,) + tuple(cfg.dimcap[1:]), cols[cfg.dimcap[0]].astype(np.int64), d["rows"], d["score"],
                                                      inside.astype(np.uint8), d["source"], d["count"], d["planes_f64"], d["source_mask"],
                                                      d["planes_f32"]))

    def classcut(w, b, cfg, r):
        d = r["dimcap"]
        cc = pa.Classcut([(e, t, c) for e, (t, c) in zip(w.class_exprs, cfg.class_rules)], cases.DECL, cases.RECALLS)
        try:
            cols, inside = ref.gather(w, d["rows"])
            masks = np.stack([cc.masks_host(d["score"][q], {k: v[q] for k, v in cols.items()}, inside[q], d["source"][q]) for q in range(b.nq)])
            assert np.array_equal(masks, ref.class_masks(w, d)), "pg_classcut_masks_host differs from classcut_ref.masks"
            return ref.as_stage(pa.candidates_classcut_host(cc, d["rows"], d["score"], d["source"], d["count"], d["planes_f64"], d["source_mask"],
                                                            d["planes_f32"], cols=cols, item_in=inside))
        finally:
            cc.free()

    def trim2(w, b, cfg, r):
        return ref.as_stage(pa.candidates_trim2_host(cfg.trim2, *ref.lists(r["classcut"])))

    def boost(w, b, cfg, r):
        d = r["trim2"]
        live = live_mask(d["rows"], d["count"])
        score, rule = d["score"].copy(), np.full(d["rows"].shape, 0xFF, np.uint8)
        for q in range(b.nq):
            idx = np.flatnonzero(live[q])
            if idx.size:
                cols, inside = ref.gather(w, d["rows"][q, idx])
                score[q, idx], rule[q, idx] = sets["boost"].boost_host(d["score"][q, idx], cols, inside, b.users[q])
        return dict(score=score, rule=rule)

    def distinct(w, b, cfg, r):
        d = r["trim2"]
        live = live_mask(d["rows"], d["count"])
        cols, inside = ref.gather(w, d["rows"])
        ids = np.stack([pa.distinct_ids_host(sets["distinct"], cfg.distinct_ids, {k: v[q] for k, v in cols.items()}, inside[q], b.users[q])
                        for q in range(b.nq)])
        return dict(ids=np.where(live, ids, 0))                        # (the host statement knows no padding: the entry writes 0 there)

    def mix(w, b, cfg, r):
        d = r["trim2"]
        m = pa.Mix(cfg.mix, cases.DECL, size=cfg.mix_size, remain_item=cfg.mix_remain, recall_names=cases.RECALLS)
        try:
            cols, inside = ref.gather(w, d["rows"])
            nq, cap = d["rows"].shape
            order, count = m.sort_host(cfg.ctx_size, nq, cap, cols=cols, item_in=inside, source=d["source"], order=r["sort"]["order"],
                                       count=d["count"], seed=b.seeds, users=b.users)
        finally:
            m.free()
        return dict(order=order, count=count)

    def diversity(w, b, cfg, r):
        d = r["trim2"]
        return dict(order=pa.diversity_rules_host(cfg.div, ref.div_planes(w, d), d["count"], d["source"], b.enable))

    return dict(blend=blend, dimcap=dimcap, classcut=classcut, trim2=trim2, boost=boost, distinct=distinct, mix=mix, diversity=diversity), sets


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_reference_equals_the_chain_of_host_statements(world, chains, shape):
    b, want = chains[shape]
    impl, sets = host_impl(world)
    try:
        got = ref.run(world, b, impl=impl)
    finally:
        for s in sets.values():
            s.free()
    diff = ref.first_difference(got, want)
    assert diff is None, ref.describe(diff, shape).replace("device", "host statements")


# ---- the comparison is not vacuous ----------------------------------------------------------------------------------------------
def perturbed(cfg, stage):
    """the scene with one stage's rule changed"""
    c = copy.deepcopy(cfg)
    if stage == "filter":
        c.filter[0]["Conditions"][0]["Value"] = 2
    elif stage == "trim":
        c.trim = [c.trim[1], c.trim[0], c.trim[2]]
    elif stage == "blend":
        c.blend = (c.blend[0], c.blend[1], [(s, wt + 1 + i) for i, (s, wt) in enumerate(c.blend[2])])
    elif stage == "dimcap":
        c.dimcap = (c.dimcap[0], c.dimcap[1] + 1, c.dimcap[2], c.dimcap[3])
    elif stage == "classcut":
        c.class_rules = [c.class_rules[0], (c.class_rules[1][0], c.class_rules[2][1]), (c.class_rules[2][0], c.class_rules[1][1])]
    elif stage == "trim2":
        c.trim2 = [c.trim2[1], c.trim2[0], c.trim2[2]]
    elif stage == "boost":
        c.boost[0]["Expression"] = "score * 2 - x"
    elif stage == "distinct":
        c.distinct_ids = [c.distinct_ids[0] + 1, c.distinct_ids[1]]
    elif stage == "mix":
        c.mix[0]["Positions"] = [3, 5, 1]
    elif stage == "ssd":
        c.ssd["filter_source_mask"] = 0b001
    elif stage == "diversity":
        c.div["rules"][0]["interval"] = 2
    return c


RULED = ("filter", "trim", "blend", "dimcap", "classcut", "trim2", "boost", "distinct", "mix", "ssd", "diversity")


@pytest.mark.parametrize("stage", RULED)
def test_the_comparison_names_the_perturbed_stage(world, chains, stage):
    b, want = chains["small"]
    got = ref.run(world, b, cfg=perturbed(b.cfg, stage))
    diff = ref.first_difference(got, want)
    assert diff is not None and diff["stage"] == stage, (stage, diff)
    assert diff["request"] is not None and stage in ref.describe(diff, "small") and "request %d" % diff["request"] in ref.describe(diff, "small")
    # an array left out, one of another shape and a single flipped padding bit are differences too
    assert ref.first_difference(want, want) is None
    broken = {k: dict(v) for k, v in want.items()}
    name = [k for k in want[stage] if not k.startswith("_") and want[stage][k] is not None][0]
    del broken[stage][name]
    assert ref.first_difference(broken, want)["stage"] == stage
    flipped = want[stage][name].copy()
    flipped.reshape(-1).view(np.uint8)[-1] ^= 1                          # the last byte of the array: padding where there is any
    broken[stage][name] = flipped
    d2 = ref.first_difference(broken, want)
    assert d2["stage"] == stage and d2["array"] == name
