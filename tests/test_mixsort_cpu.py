"""CPU tests of MultiRecallMixSort (include/pairec_gpu.h: pg_mix_*).  No GPU needed.

(a) a literal transcription of the Go loops (sort/multi_recall_mix_sort.go, sort/mix_sort_strategy.go: strategy objects, the item
    loop with its early exit, BuildItems, remainItemIterator, the shrink branch) against tests/mixsort_ref.py, which states the
    answer strategy by strategy, on the reference's own test cases (tests/golden/multi_recall_mix_sort.json) and on 20 000 seeded
    random small cases; rand.Intn(k) is replaced in both by draw(seed, s, j) % k.  The transcription never takes the shrink branch.
(b) pg_mix_sort_host against the ref on the same cases, with and without order, count and seed.
(c) every refusal returns its code and names the cause."""
import json
import os

import numpy as np
import pytest

import pairec_amd as pa
from pairec_amd import _lib

import cond_ref
import mixsort_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "multi_recall_mix_sort.json")))
COLS = [("c", pa.F_I32), ("p", pa.F_I64), ("sex", pa.F_I32), ("tag", pa.F_I32)]


# ---- the Go code, line by line ---------------------------------------------------------------------------------------------------
class _Strategy:
    """mixSortStrategy and its three embedders (mix_sort_strategy.go:31-245)"""

    def __init__(self, kind, config, size, index, seed, shrink):
        self.kind, self.number, self.total_size, self.index, self.items = kind, 0, size, 0, []
        self.mask = ref.source_mask(config, config.get("_recall_names", ())) if config else 0
        self.conds = (config.get("Conditions") or None) if config else None          # filterParam != nil iff len(Conditions) > 0
        self.s, self.seed, self.shrink = index, seed, shrink
        if kind == "fix":
            self.positions = list(config.get("Positions") or [])
            self.position_field = config.get("PositionField", "") or ""
            self.number = len(self.positions)
            if self.number == 0 and config.get("Number", 0) > 0:
                self.number = config["Number"]
        elif kind == "random":
            if config.get("NumberRate", 0.0) > 0.0:
                self.number = int(float(size) * config["NumberRate"])
            elif config.get("Number", 0) > 0:
                self.number = config["Number"]
        else:
            self.number = size

    def contains_recall_name(self, item):
        if self.kind == "default":
            return True
        return item["source"] < 32 and (self.mask >> item["source"]) & 1 == 1

    def append_item(self, item):
        if len(self.items) == self.number:
            return
        self.items.append(item)

    def is_full(self):
        return len(self.items) >= self.number

    def build_items(self, items):
        if self.kind == "fix":
            if len(self.positions) == 0 and self.position_field != "":
                for i in range(self.number):
                    if i < len(self.items):
                        p = self.items[i]["pos"].get(self.position_field, -1)
                        if p > 0:
                            self.positions.append(p)
            for pos in self.positions:
                if pos <= self.total_size and self.index < len(self.items):
                    items[pos - 1] = self.items[self.index]
                    self.index += 1
            return items
        if self.kind == "random":
            start = end = 0
            for j, item in enumerate(self.items):
                if not any(x is None for x in items[:self.total_size]):
                    break
                end = start + ref.draw(self.seed, self.s, j) % (self.total_size // self.number)
                if end >= self.total_size:
                    end = self.total_size - 1
                attempts = 0
                while items[end] is not None and attempts < self.total_size:
                    end = (end + 1) % self.total_size
                    attempts += 1
                if items[end] is None:
                    items[end] = item
                start += self.total_size // self.number
            return items
        for i in range(len(items)):
            if items[i] is None and self.index < len(self.items):
                items[i] = self.items[self.index]
                self.index += 1
        return items


def go_do_sort(rules, conf_size, remain_item, ctx_size, items, evaluate, seed, shrink):
    """doSort (multi_recall_mix_sort.go:62-178); items: dicts with a unique "id"; evaluate(conds, item) → bool"""
    size = ctx_size
    if conf_size > size:
        size = conf_size
    if len(items) < size:
        return items
    result = [None] * size
    strategies = []
    for config in rules:                                                          # createMixStrategies
        if config["MixStrategy"] == "fix_position":
            strategies.append(_Strategy("fix", config, size, len(strategies), seed, shrink))
        elif config["MixStrategy"] == "random_position":
            strategies.append(_Strategy("random", config, size, len(strategies), seed, shrink))
    default = _Strategy("default", None, size, -1, seed, shrink)
    for item in items:
        found = False
        for st in strategies:
            if st.contains_recall_name(item):
                if not st.is_full():
                    found = True
                    st.append_item(item)
                    break
            if st.conds is not None:
                ok = evaluate(st.conds, item)
                if ok:
                    if not st.is_full():
                        found = ok
                        st.append_item(item)
                        break
        if not found:
            default.append_item(item)
        if default.is_full():
            if all(st.is_full() for st in strategies):
                break
    for st in strategies:
        if st.kind == "fix":
            result = st.build_items(result)
    for st in strategies:
        if st.kind == "random":
            result = st.build_items(result)
    result = default.build_items(result)
    size = len(result)
    it = None
    i = 0
    while i < size:
        if result[i] is None:
            if it is None:
                it = _RemainIterator(result, items)
            item = it.find()
            if item is not None:
                result[i] = item
            else:
                shrink.append(1)
                result[i] = result[size - 1]
                result = result[:size - 1]
                i -= 1
                size -= 1
        i += 1
    if remain_item:
        if it is None:
            it = _RemainIterator(result, items)
        while True:
            item = it.find()
            if item is None:
                break
            result.append(item)
    return result


class _RemainIterator:
    def __init__(self, result, items):
        self.index, self.items = 0, items
        self.result_map = {item["id"] for item in result if item is not None}

    def find(self):
        item = None
        while self.index < len(self.items):
            if self.items[self.index]["id"] not in self.result_map:
                item = self.items[self.index]
                self.result_map.add(item["id"])
                self.index += 1
                break
            self.index += 1
        return item


def literal(strategies, size, remain, ctx_size, nq, cap, cols, item_in, source, order, count, seed, users, recall_names, shrink):
    """go_do_sort per request on [nq][cap] arrays → (out_order, out_count) like the ref"""
    out = np.full((nq, cap), ref.EMPTY, dtype=np.uint32)
    cnt = np.zeros(nq, dtype=np.uint32)
    rules = [dict(st, _recall_names=recall_names) for st in strategies]
    for q in range(nq):
        n = cap if count is None else min(int(count[q]), cap)
        cq = {k: np.asarray(v).reshape(nq, cap)[q] for k, v in (cols or {}).items()}
        iq = np.ones(cap, bool) if item_in is None else np.asarray(item_in).reshape(nq, cap)[q].astype(bool)
        items = []
        for j in range(n):
            e = int(order[q][j]) if order is not None else j
            pos = {k: int(v[e]) for k, v in cq.items() if iq[e]}                  # utils.ToInt(GetProperty(field), -1)
            items.append({"id": e, "source": int(source[q][e]) if source is not None else 0xFF, "pos": pos})
        user = {} if users is None else (users[q] or {})
        res = go_do_sort(rules, size, remain, ctx_size, items, lambda conds, item: cond_ref.match(conds, item["id"], cq, iq, user),
                         0 if seed is None else int(seed[q]), shrink)
        out[q, :len(res)] = [item["id"] for item in res]
        cnt[q] = len(res)
    return out, cnt


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def encode(conds):
    """string values → dictionary ids (the golden file's table)"""
    out = []
    for c in conds or ():
        c = dict(c)
        if isinstance(c.get("Value"), str) and c.get("Type") == "string":
            c["Value"] = GOLDEN["strings"][c["Value"]]
        out.append(c)
    return out


def golden_runs():
    for case in GOLDEN["cases"]:
        it = case["items"]
        n = len(it["source"])
        score = np.array(it["score"], dtype=np.float64)
        order = np.argsort(-score, kind="stable").astype(np.uint32)                 # ItemRankScoreSort first
        rules = [dict(r, Conditions=encode(r.get("Conditions"))) for r in case["config"]["MixSortRules"]]
        cols = {k: np.array(v, dtype=np.int32).reshape(1, n) for k, v in it.get("columns", {}).items()}
        for size in case["sizes"]:
            yield case, dict(strategies=rules, size=case["config"].get("Size", 0), remain=bool(case["config"].get("RemainItem", False)),
                             ctx_size=size, nq=1, cap=n, cols=cols, item_in=None, source=np.array(it["source"], dtype=np.uint8).reshape(1, n),
                             order=order.reshape(1, n), count=None, seed=np.array([size], dtype=np.uint64), users=None,
                             recall_names=tuple(case["recall_names"]))


def check_golden_facts(case, run, out, cnt):
    it, facts = case["items"], case["facts"]
    res = [int(e) for e in out[0][:cnt[0]]]
    assert ref.EMPTY not in res and len(set(res)) == len(res)                       # "item has nil item"
    if "positions_hold" in facts:
        f = facts["positions_hold"]
        for k, pos in enumerate(f["positions"]):
            e = res[pos - 1]
            if "recall_name" in f:
                assert case["recall_names"][it["source"][e]] == f["recall_name"]
                assert it["score"][e] == f["scores"][k]
            else:
                assert it["columns"][f["column"]][e] == GOLDEN["strings"][f["value"]]
    if "first_scores" in facts:
        assert case["recall_names"][it["source"][res[0]]] == facts["first_recall_name"]
        assert [it["score"][e] for e in res[:3]] == facts["first_scores"]
    if "length" in facts:
        assert len(res) == (run["ctx_size"] if facts["length"] == "ctx_size" else len(it["source"]))


def random_config(rng):
    """one config over nq requests: n <= 40, S <= 30, 0..4 strategies; duplicate positions, positions > S, column positions <= 0,
    number 0 and number = S all occur"""
    S = int(rng.integers(1, 31))
    conf_size = int(rng.choice([0, S, int(rng.integers(0, S + 1))]))
    ctx_size = S if conf_size < S or rng.random() < 0.5 else int(rng.integers(0, S + 1))
    nq = 4
    cap = int(rng.integers(1, 41))
    strategies = []
    for _ in range(int(rng.integers(0, 5))):
        st = {}
        if rng.random() < 0.55:
            st["MixStrategy"] = "fix_position"
            k = rng.random()
            if k < 0.6:
                st["Positions"] = [int(p) for p in rng.integers(1, S + 4, size=int(rng.integers(1, 8)))]
            elif k < 0.9:
                st["PositionField"] = "p"
                st["Number"] = int(rng.choice([0, S, int(rng.integers(0, 42))]))
            else:
                st["Number"] = int(rng.integers(0, 6))                             # takes entries, places none
        else:
            st["MixStrategy"] = "random_position"
            if rng.random() < 0.4:
                st["NumberRate"] = float(rng.choice([0.1, 0.25, 0.3, 0.5, 1.0]))
            else:
                st["Number"] = int(rng.choice([0, S, int(rng.integers(0, S + 1))]))
        if rng.random() < 0.7:
            st["SourceMask"] = int(rng.integers(0, 16))
        if rng.random() < 0.5:
            st["Conditions"] = [{"Name": "c", "Operator": "equal", "Type": "int", "Value": int(rng.integers(0, 4))}]
            if rng.random() < 0.25:
                st["Conditions"].append({"Name": "age", "Domain": "user", "Operator": "greater", "Type": "int", "Value": 30})
        strategies.append(st)
    shape = (nq, cap)
    run = dict(strategies=strategies, size=conf_size, remain=bool(rng.random() < 0.5), ctx_size=ctx_size, nq=nq, cap=cap,
               cols={"c": rng.integers(0, 4, size=shape).astype(np.int32), "p": rng.integers(-2, S + 4, size=shape).astype(np.int64)},
               item_in=(rng.random(shape) < 0.9).astype(np.uint8) if rng.random() < 0.5 else None,
               source=rng.integers(0, 6, size=shape).astype(np.uint8),
               order=np.stack([rng.permutation(cap) for _ in range(nq)]).astype(np.uint32) if rng.random() < 0.5 else None,
               count=rng.integers(0, cap + 1, size=nq).astype(np.uint32) if rng.random() < 0.5 else None,
               seed=rng.integers(0, 1 << 63, size=nq).astype(np.uint64) if rng.random() < 0.5 else None,
               users=[({"age": int(rng.integers(20, 41))} if rng.random() < 0.8 else None) for _ in range(nq)], recall_names=())
    if run["count"] is not None and rng.random() < 0.5:
        run["count"][int(rng.integers(0, nq))] = cap
    return run


def host(run):
    m = pa.mix_compile(run["strategies"], COLS, run["size"], run["remain"], run["recall_names"])
    try:
        return m.sort_host(run["ctx_size"], run["nq"], run["cap"], cols=run["cols"], item_in=run["item_in"], source=run["source"], order=run["order"],
                           count=run["count"], seed=run["seed"], users=run["users"])
    finally:
        m.free()


def want(run):
    kw = {k: run[k] for k in ("cols", "item_in", "source", "order", "count", "seed", "users", "recall_names")}
    return ref.mix_sort(run["strategies"], run["size"], run["remain"], run["ctx_size"], run["nq"], run["cap"], **kw)


def test_golden_cases_literal_ref_and_host_agree_and_hold_the_facts():
    shrink = []
    runs = 0
    for case, run in golden_runs():
        w_out, w_cnt = want(run)
        kw = {k: run[k] for k in ("cols", "item_in", "source", "order", "count", "seed", "users", "recall_names")}
        l_out, l_cnt = literal(run["strategies"], run["size"], run["remain"], run["ctx_size"], run["nq"], run["cap"], shrink=shrink, **kw)
        h_out, h_cnt = host(run)
        assert np.array_equal(l_out, w_out) and np.array_equal(l_cnt, w_cnt), (case["name"], run["ctx_size"])
        assert np.array_equal(h_out, w_out) and np.array_equal(h_cnt, w_cnt), (case["name"], run["ctx_size"])
        check_golden_facts(case, run, w_out, w_cnt)
        runs += 1
    assert runs == 10 + 1 + 11 + 21 + 10 + 11 + 21 and not shrink


def test_random_cases_literal_ref_and_host_agree():
    rng = np.random.default_rng(20260101)
    shrink = []
    cases = placed = 0
    while cases < 20000:
        run = random_config(rng)
        S = max(run["ctx_size"], run["size"])
        if S < 1 or any(st["MixStrategy"] == "random_position" and ref.number_of(st, S) > S for st in run["strategies"]):
            continue                                                             # (refused configs: test_refusals)
        w_out, w_cnt = want(run)
        kw = {k: run[k] for k in ("cols", "item_in", "source", "order", "count", "seed", "users", "recall_names")}
        l_out, l_cnt = literal(run["strategies"], run["size"], run["remain"], run["ctx_size"], run["nq"], run["cap"], shrink=shrink, **kw)
        assert np.array_equal(l_out, w_out) and np.array_equal(l_cnt, w_cnt), run
        h_out, h_cnt = host(run)
        assert np.array_equal(h_out, w_out) and np.array_equal(h_cnt, w_cnt), run
        for q in range(run["nq"]):
            n = run["cap"] if run["count"] is None else int(run["count"][q])
            if n >= S:                                                           # |result| = S exactly, no duplicates
                assert w_cnt[q] == (n if run["remain"] else S) and len(set(w_out[q][:w_cnt[q]].tolist())) == w_cnt[q]
                placed += 1
        cases += run["nq"]
    assert not shrink                                                            # :152-156 is never taken
    assert placed > 5000                                                         # (the generator does reach the page-shaping path)


def _err(fn):
    with pytest.raises(_lib.PgError) as e:
        fn()
    return e.value.code, str(e.value)


def test_refusals_name_their_cause():
    INVALID, UNSUPPORTED = -1, -4
    src = np.zeros((1, 8), np.uint8)
    fix = lambda **kw: dict({"MixStrategy": "fix_position"}, **kw)                   # noqa: E731
    rnd = lambda **kw: dict({"MixStrategy": "random_position"}, **kw)                # noqa: E731
    code, msg = _err(lambda: pa.mix_compile([fix(Positions=[1, 0])]))
    assert code == INVALID and "position 0" in msg
    code, msg = _err(lambda: pa.mix_compile([rnd(Number=-1)]))
    assert code == INVALID and "negative number" in msg
    code, msg = _err(lambda: pa.mix_compile([rnd(NumberRate=-0.5)]))
    assert code == INVALID and "negative number_rate" in msg
    code, msg = _err(lambda: pa.mix_compile([fix(PositionField="f")], [("f", pa.F_F32)]))
    assert code == INVALID and "\"f\"" in msg and "int32 / int64" in msg
    code, msg = _err(lambda: pa.mix_compile([fix(PositionField="nope")], COLS))
    assert code == INVALID and "\"nope\"" in msg and "declared" in msg
    code, msg = _err(lambda: pa.mix_compile([{"MixStrategy": 7}]))
    assert code == INVALID and "unknown strategy type 7" in msg
    code, msg = _err(lambda: pa.mix_compile([rnd(Number=1)] * 9))
    assert code == UNSUPPORTED and "9 strategies" in msg
    code, msg = _err(lambda: pa.mix_compile([fix(Positions=[1] * 257)]))
    assert code == UNSUPPORTED and "257 positions" in msg
    code, msg = _err(lambda: pa.mix_compile([], size=4097))
    assert code == UNSUPPORTED and "4097" in msg
    code, msg = _err(lambda: pa.mix_compile([fix(Positions=[1], Conditions=[{"Name": "c", "Operator": "contains", "Type": "int", "Value": 1}])], COLS))
    assert code == UNSUPPORTED and "pg_cond_compile" in msg and "contains" in msg
    # at a call
    m = pa.mix_compile([rnd(Number=5, SourceMask=1)])
    try:
        code, msg = _err(lambda: m.sort_host(4, 1, 8, source=src))
        assert code == INVALID and "number 5" in msg and "4 slots" in msg
        code, msg = _err(lambda: m.sort_host(8, 1, 8))
        assert code == INVALID and "source" in msg
        code, msg = _err(lambda: m.sort_host(4097, 1, 8, source=src))
        assert code == UNSUPPORTED and "4097" in msg
        code, msg = _err(lambda: m.sort_host(8, 1, 16385, source=np.zeros((1, 16385), np.uint8)))
        assert code == UNSUPPORTED and "cap=16385" in msg
        code, msg = _err(lambda: m.sort_host(8, 257, 8, source=np.zeros((257, 8), np.uint8)))
        assert code == UNSUPPORTED and "nq=257" in msg
        out, cnt = m.sort_host(8, 1, 8, source=src)                                # still usable
        assert cnt[0] == 8 and sorted(out[0].tolist()) == list(range(8))
    finally:
        m.free()
    m = pa.mix_compile([rnd(NumberRate=1.5, SourceMask=1)])
    try:
        code, msg = _err(lambda: m.sort_host(8, 1, 8, source=src))
        assert code == INVALID and "number_rate 1.5" in msg
    finally:
        m.free()
    m = pa.mix_compile([fix(PositionField="p", Number=2, SourceMask=1)], COLS)
    try:
        code, msg = _err(lambda: m.sort_host(8, 1, 8, source=src))
        assert code == INVALID and "\"p\"" in msg and "missing" in msg
    finally:
        m.free()


def test_no_strategies_is_the_list_and_the_tail():
    for remain in (False, True):
        m = pa.mix_compile([], size=3, remain_item=remain)
        try:
            order = np.array([[4, 2, 0, 1, 3, 5]], dtype=np.uint32)
            out, cnt = m.sort_host(0, 1, 6, order=order, count=np.array([5], np.uint32))
            assert cnt[0] == (5 if remain else 3)
            assert out[0].tolist() == ([4, 2, 0, 1, 3, ref.EMPTY] if remain else [4, 2, 0] + [ref.EMPTY] * 3)
        finally:
            m.free()


# ---- (d) the host mirror's config (its sort runs on the device: tests/test_gpu_mixsort.py) ----------------------------------------
import copy                 # noqa: E402
import ctypes as C          # noqa: E402

from oracle import oracle as o      # noqa: E402

MIRROR_SORTS = [
    {"Name": "fix_r1", "SortType": "MultiRecallMixSort",
     "MixSortRules": [{"MixStrategy": "fix_position", "Positions": [1, 4, 6, 8, 10], "RecallNames": ["r1"]}]},
    {"Name": "skips_unknown", "SortType": "MultiRecallMixSort",
     "MixSortRules": [{"MixStrategy": "shuffle_position", "Positions": [0], "Number": -4, "RecallNames": ["r2"]},
                      {"MixStrategy": "fix_position", "Positions": [1, 4, 6, 8, 10], "RecallNames": ["r1"]}]},
    {"Name": "random_man", "SortType": "MultiRecallMixSort", "RemainItem": True, "Size": 12, "Seed": 77,
     "MixSortRules": [{"MixStrategy": "random_position", "NumberRate": 0.3,
                       "Conditions": [{"Name": "sex", "Type": "string", "Value": "man", "Operator": "equal"}]}]},
    {"Name": "page_mix", "SortType": "MultiRecallMixSort",
     "MixSortRules": [{"MixStrategy": "fix_position", "Positions": [2, 4, 4], "RecallNames": ["gpu_vector_recall"]},
                      {"MixStrategy": "fix_position", "PositionField": "slot", "Number": 3, "RecallNames": ["gpu_vector_recall"]}]},
]
MIRROR_CONFIG = {
    "RunMode": "product", "AlgoConfs": [], "RecallConfs": [],
    "SceneConfs": {"plain": {"default": {"RecallNames": ["gpu_vector_recall"]}}, "mixed": {"default": {"RecallNames": ["gpu_vector_recall"]}}},
    "SortNames": {"plain": ["ItemRankScore"], "mixed": ["ItemRankScore", "page_mix"]},
    "SortConfs": [{"Name": "host_mix", "SortType": "MultiRecallMixSort", "MixSortRules": [{"MixStrategy": "fix_position", "Positions": [0]}]}],
    "UserDefineConfs": {"pairec_gpu": {
        "Device": 0, "Table": {"Rows": 20000, "Dim": 128, "IdPrefix": "item_", "SyntheticSeed": o.SEED_TABLE},
        "Recalls": [{"Name": "gpu_vector_recall", "Kind": "vector", "RecallCount": 300, "RecallAlgo": "gpu_faiss", "ItemType": "video"}],
        "Algorithms": [{"Name": "gpu_faiss", "Kind": "faiss"}],
        "Sorts": MIRROR_SORTS}},
}


def mirror_lib():
    L = C.CDLL(os.environ.get("PH_HOST_LIB") or os.path.join(os.path.dirname(HERE), "pairec_amd", "libpairec_host.so"))
    L.ph_last_error.restype = C.c_char_p
    L.ph_parse_recconf.restype = C.c_char_p
    L.ph_parse_recconf.argtypes = [C.c_char_p]
    L.ph_engine_create.restype = C.c_void_p
    L.ph_engine_create.argtypes = [C.c_char_p]
    L.ph_engine_destroy.argtypes = [C.c_void_p]
    L.ph_set_user_vector.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    L.ph_engine_sort_scored.restype = C.c_char_p
    L.ph_engine_sort_scored.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    L.ph_recommend.restype = C.c_char_p
    L.ph_recommend.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p]
    return L


def test_mirror_config_parses_skips_unknown_strategies_and_keeps_sortconfs():
    """a SortConfs entry of the type stays a host-side name (even one the device would refuse); rules with an unknown MixStrategy
    are skipped as createMixStrategies skips them, whatever else they carry"""
    H = mirror_lib()
    r = H.ph_parse_recconf(json.dumps(MIRROR_CONFIG).encode())
    assert r, H.ph_last_error()
    assert json.loads(r)["gpu_sorts"] == len(MIRROR_SORTS)


@pytest.mark.parametrize("edit,words", [
    (lambda s: s[0]["MixSortRules"][0].update({"Positions": [3, 0]}), (b"MultiRecallMixSort", b"fix_r1", b"Positions")),
    (lambda s: s[0]["MixSortRules"][0].update({"Positions": [1] * 257}), (b"MultiRecallMixSort", b"257 Positions")),
    (lambda s: s[2]["MixSortRules"][0].update({"NumberRate": -0.1}), (b"MultiRecallMixSort", b"random_man", b"NumberRate")),
    (lambda s: s[2]["MixSortRules"][0].update({"Number": -1}), (b"MultiRecallMixSort", b"Number")),
    (lambda s: s[2].update({"Size": 4097}), (b"MultiRecallMixSort", b"Size")),
    (lambda s: s[0].update({"MixSortRules": s[0]["MixSortRules"] * 9}), (b"MultiRecallMixSort", b"9 MixSortRules")),
    (lambda s: s[2]["MixSortRules"][0]["Conditions"][0].update({"Type": "time"}), (b"MultiRecallMixSort", b"Conditions", b'"time"')),
])
def test_mirror_refused_config_names_its_key(edit, words):
    H = mirror_lib()
    cfg = copy.deepcopy(MIRROR_CONFIG)
    edit(cfg["UserDefineConfs"]["pairec_gpu"]["Sorts"])
    assert not H.ph_parse_recconf(json.dumps(cfg).encode())
    for w in words:
        assert w in H.ph_last_error(), H.ph_last_error()
