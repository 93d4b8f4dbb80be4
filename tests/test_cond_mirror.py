"""The host mirror's side of DESIGN.md 4.1p: `SortType: "BoostScoreSort"` in `UserDefineConfs.pairec_gpu.Sorts` (the reference's
keys: BoostScoreConditions[].Conditions / .Expression, BoostScoreConditionsFilterAll) and a `pairec_gpu.Filters` list with
`FilterType: "ItemStateFilter"` (FilterParams, FeatureStore) run per scene through `pairec_gpu.FilterNames`.  CPU: the config parse
and its refusals by name; SortConfs handling unchanged.  GPU: the reference's r1 / r2 case and its two round cases through ph_*
give the scores sort/boost_score_sort_test.go asserts; strings are dictionary-encoded per call; what cannot be served leaves Data
untouched and returns an error; the filter alone against cond_ref; and a config-driven scene — recall → ItemStateFilter →
BoostScoreSort → ItemRankScore — returns the page the Python composition of cond_ref gives."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

import cond_ref as ref
from oracle import oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "boost_score_sort.json")) as _f:
    BOOST_CASES = {c["name"]: c for c in json.load(_f)["cases"]}

ROWS = 20000
STATE = [{"Name": "status", "Operator": "equal", "Type": "int", "Value": 1},
         {"Operator": "bool", "Type": "or", "Configs": [{"Name": "stock", "Operator": "greater", "Type": "int", "Value": "user.min_stock"},
                                                         {"Name": "category", "Operator": "in", "Type": "int", "Value": [2, 5, 7]}]}]
SCENE_BOOST = [{"Conditions": [{"Name": "vip", "Domain": "user", "Operator": "equal", "Type": "int", "Value": 1}], "Expression": "score * (-1)"},
               {"Conditions": [], "Expression": "score * 3 + 0.5"}]
R1R2 = BOOST_CASES["boost_score_sort"]["config"]["BoostScoreConditions"]
CONFIG = {
    "RunMode": "product", "AlgoConfs": [], "RecallConfs": [],
    "SceneConfs": {"plain": {"default": {"RecallNames": ["gpu_vector_recall"]}}, "feed": {"default": {"RecallNames": ["gpu_vector_recall"]}}},
    "SortNames": {"plain": ["ItemRankScore"], "feed": ["scene_boost", "ItemRankScore"]},
    "UserDefineConfs": {"pairec_gpu": {
        "Device": 0, "Table": {"Rows": ROWS, "Dim": 128, "IdPrefix": "item_", "SyntheticSeed": o.SEED_TABLE},
        "Recalls": [{"Name": "gpu_vector_recall", "Kind": "vector", "RecallCount": 300, "RecallAlgo": "gpu_faiss", "ItemType": "video"}],
        "Algorithms": [{"Name": "gpu_faiss", "Kind": "faiss"}],
        "Filters": [{"Name": "state", "FilterType": "ItemStateFilter", "FeatureStore": "item_features", "FilterParams": STATE}],
        "FilterNames": {"feed": ["state"]},
        "Sorts": [{"Name": "r1r2", "SortType": "BoostScoreSort", "BoostScoreConditions": R1R2},
                  {"Name": "r1r2_all", "SortType": "BoostScoreSort", "BoostScoreConditions": R1R2 + [{"Conditions": [], "Expression": "score + price"}],
                   "BoostScoreConditionsFilterAll": True},
                  {"Name": "round2", "SortType": "BoostScoreSort", "BoostScoreConditions": BOOST_CASES["boost_score_sort_With_round"]["config"]["BoostScoreConditions"]},
                  {"Name": "round1", "SortType": "BoostScoreSort", "BoostScoreConditions": BOOST_CASES["boost_score_sort_With_round_v2"]["config"]["BoostScoreConditions"]},
                  {"Name": "scene_boost", "SortType": "BoostScoreSort", "BoostScoreConditions": SCENE_BOOST}]}},
}


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(os.environ.get("PH_HOST_LIB") or os.path.join(ROOT, "pairec_amd", "libpairec_host.so"))
    L.ph_last_error.restype = C.c_char_p
    L.ph_parse_recconf.restype = C.c_char_p
    L.ph_parse_recconf.argtypes = [C.c_char_p]
    L.ph_engine_create.restype = C.c_void_p
    L.ph_engine_create.argtypes = [C.c_char_p]
    L.ph_engine_destroy.argtypes = [C.c_void_p]
    L.ph_set_user_vector.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    L.ph_engine_set_feature_column.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
    L.ph_engine_sort_scored.restype = C.c_char_p
    L.ph_engine_sort_scored.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    L.ph_engine_filter.restype = C.c_char_p
    L.ph_engine_filter.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]
    L.ph_recommend.restype = C.c_char_p
    L.ph_recommend.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p]
    L.ph_recommend_ab.restype = C.c_char_p
    L.ph_recommend_ab.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p]
    return L


def gpu_conf(cfg):
    return cfg["UserDefineConfs"]["pairec_gpu"]


# ---- CPU: the config ----------------------------------------------------------------------------------------------------------

def test_config_parses_and_sortconfs_stay_as_they_are(H):
    r = H.ph_parse_recconf(json.dumps(CONFIG).encode())
    assert r, H.ph_last_error()
    assert json.loads(r)["gpu_sorts"] == 5
    cfg = copy.deepcopy(CONFIG)                                          # a SortConfs BoostScoreSort stays a host-side name
    cfg["SortConfs"] = [{"Name": "host_boost", "SortType": "BoostScoreSort", "BoostScoreConditions": [{"Conditions": [], "Expression": "score > 1"}]}]
    assert H.ph_parse_recconf(json.dumps(cfg).encode()), H.ph_last_error()


@pytest.mark.parametrize("edit,words", [
    (lambda g: g["Sorts"][0]["BoostScoreConditions"][0].update({"Expression": ""}), (b"BoostScoreSort", b"without an Expression")),
    (lambda g: g["Sorts"][0]["BoostScoreConditions"][0].update({"Expression": "score > 1"}), (b"BoostScoreSort", b"'>'")),
    (lambda g: g["Sorts"][0]["BoostScoreConditions"][0].update({"Expression": "log(score)"}), (b"BoostScoreSort", b'"log"')),
    (lambda g: g["Sorts"][0].update({"BoostScoreConditions": [R1R2[0]] * 9}), (b"BoostScoreSort", b"BoostScoreConditions")),
    (lambda g: g["Sorts"][0]["BoostScoreConditions"][0]["Conditions"][0].update({"Type": "time"}), (b"BoostScoreSort", b'"time"')),
    (lambda g: g["Sorts"][0]["BoostScoreConditions"][0].update({"Conditions": [R1R2[0]["Conditions"][0]] * 9}), (b"BoostScoreSort", b"9 operators")),
    (lambda g: g["Filters"][0].update({"FilterType": "ItemCustomFilter"}), (b"pairec_gpu.Filters", b"ItemCustomFilter")),
    (lambda g: g["Filters"][0].update({"FeatureStore": "holo_state"}), (b"pairec_gpu.Filters", b"holo_state")),
    (lambda g: g["Filters"][0]["FilterParams"][0].update({"Type": "string", "Value": "on"}), (b"pairec_gpu.Filters", b'"status"')),
    (lambda g: g["Filters"][0]["FilterParams"][0].update({"Value": "online"}), (b"pairec_gpu.Filters", b"not an integer")),
])
def test_config_refusals_by_name(H, edit, words):
    cfg = copy.deepcopy(CONFIG)
    edit(gpu_conf(cfg))
    assert not H.ph_parse_recconf(json.dumps(cfg).encode())
    for w in words:
        assert w in H.ph_last_error(), H.ph_last_error()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

class Eng:
    pass


@pytest.fixture(scope="module")
def eng(H):
    e = Eng()
    e.h = H.ph_engine_create(json.dumps(CONFIG).encode())
    assert e.h, H.ph_last_error()
    rng = np.random.default_rng(12)
    e.store = {"status": (rng.random(ROWS) < 0.7).astype(np.int32), "stock": rng.integers(0, 10, ROWS).astype(np.int32),
               "category": rng.integers(0, 10, ROWS).astype(np.int32)}
    for name, a in e.store.items():
        assert H.ph_engine_set_feature_column(e.h, name.encode(), a.ctypes.data_as(C.c_void_p), ROWS) == 0, H.ph_last_error()
    user = o.synth_rows(o.SEED_QUERY, 3, 1, 128)[0]
    H.ph_set_user_vector(e.h, b"u1", " ".join("%d:%s" % (i + 1, repr(float(v))) for i, v in enumerate(user)).encode())
    yield e
    H.ph_engine_destroy(e.h)


def sort_scored(H, eng, name, items, user=None):
    r = H.ph_engine_sort_scored(eng.h, name.encode(), json.dumps(items).encode(), json.dumps(user or {}).encode(), 10)
    return None if r is None else json.loads(r)["items"]


def items_of(case):
    return [{"id": it["Id"], "score": it["Score"], "properties": it["Properties"]} for it in case["items"]]


@pytest.mark.gpu
def test_the_reference_boost_cases_through_the_mirror(H, eng):
    out = sort_scored(H, eng, "r1r2", items_of(BOOST_CASES["boost_score_sort"]))
    assert [x["item_id"] for x in out] == [str(i) for i in range(20)]                     # order untouched
    assert out[0]["score"] == 0.0 and out[1]["score"] == 100.0 and out[10]["score"] == -100.0
    assert [x["score"] for x in out] == [i * 100.0 for i in range(10)] + [i * -10.0 for i in range(10, 20)]
    assert sort_scored(H, eng, "round2", items_of(BOOST_CASES["boost_score_sort_With_round"]))[0]["score"] == 0.93
    assert sort_scored(H, eng, "round1", items_of(BOOST_CASES["boost_score_sort_With_round_v2"]))[0]["score"] == 1.0
    assert sort_scored(H, eng, "r1r2", []) == []


@pytest.mark.gpu
def test_filter_all_strings_and_what_cannot_be_served(H, eng):
    items = [{"id": "a", "score": 1.0, "properties": {"recall_name": "r1", "price": 2.5}},
             {"id": "b", "score": 2.0, "properties": {"recall_name": "r2", "price": 4}},
             {"id": "c", "score": 3.0, "properties": {"recall_name": "somewhere else", "price": 0.25}}]
    out = sort_scored(H, eng, "r1r2_all", items)
    assert [x["score"] for x in out] == [1.0 * 100 + 2.5, 2.0 * -10 + 4, 3.0 + 0.25]      # both matching rules, in sequence
    # an item without a named property: an error, Data untouched (the caller ignores the error, as for every sort)
    lacking = copy.deepcopy(items)
    del lacking[1]["properties"]["price"]
    assert sort_scored(H, eng, "r1r2_all", lacking) is None
    assert b"BoostScoreSort" in H.ph_last_error() and b'"price"' in H.ph_last_error() and b"item b" in H.ph_last_error()
    wrong = copy.deepcopy(items)
    wrong[2]["properties"]["price"] = "cheap"
    assert sort_scored(H, eng, "r1r2_all", wrong) is None and b"not a number" in H.ph_last_error()
    many = [{"id": str(i), "score": 1.0, "properties": {"recall_name": "r1"}} for i in range(16385)]
    assert sort_scored(H, eng, "r1r2", many) is None and b"16385 items" in H.ph_last_error()
    # user properties reach the conditions: vip = 1 negates, anything else takes the second rule
    plain = [{"id": str(i), "score": float(i)} for i in range(5)]
    assert [x["score"] for x in sort_scored(H, eng, "scene_boost", plain, {"vip": 1})] == [-0.0, -1.0, -2.0, -3.0, -4.0]
    assert [x["score"] for x in sort_scored(H, eng, "scene_boost", plain, {"vip": 2})] == [i * 3 + 0.5 for i in range(5)]
    assert [x["score"] for x in sort_scored(H, eng, "scene_boost", plain)] == [i * 3 + 0.5 for i in range(5)]


def want_kept(eng, ids, user):
    rows = np.array([int(i[5:]) if i.startswith("item_") and int(i[5:]) < ROWS else ROWS for i in ids], dtype=np.uint64)
    cols, inside = ref.gather(eng.store, ROWS, rows)
    return [i for k, i in enumerate(ids) if ref.match(STATE, k, cols, inside, user)]


@pytest.mark.gpu
def test_item_state_filter_through_the_mirror(H, eng):
    rng = np.random.default_rng(3)
    ids = ["item_%d" % r for r in rng.choice(ROWS, 700, replace=False)] + ["stranger_1", "item_99999999"]
    rng.shuffle(ids)
    items = [{"id": i, "score": float(k)} for k, i in enumerate(ids)]
    for user in ({"min_stock": 6}, {"min_stock": 0}, {}):
        r = H.ph_engine_filter(eng.h, b"state", json.dumps(items).encode(), json.dumps(user).encode())
        assert r, H.ph_last_error()
        got = json.loads(r)["items"]
        want = want_kept(eng, ids, user)
        assert [x["item_id"] for x in got] == want and 0 < len(want) < len(ids)
        assert [x["score"] for x in got] == [float(ids.index(i)) for i in want]            # the items themselves, scores untouched
    assert json.loads(H.ph_engine_filter(eng.h, b"state", b"[]", b"{}"))["items"] == []
    assert H.ph_engine_filter(eng.h, b"nobody", b"[]", b"{}") is None


@pytest.mark.gpu
def test_config_driven_scene_equals_the_python_composition(H, eng):
    base = json.loads(H.ph_recommend(eng.h, b"u1", 300, b"plain"))["items"]              # the recall's 300 items, by score
    assert len(base) == 300
    ids, score = [x["item_id"] for x in base], np.array([x["score"] for x in base])
    for user in ({"vip": 1, "min_stock": 4}, {"vip": 0, "min_stock": 4}, {"min_stock": 8}):
        r = H.ph_recommend_ab(eng.h, b"u1", 40, b"feed", json.dumps({"_user_features": user}).encode())
        assert r, H.ph_last_error()
        got = json.loads(r)["items"]
        kept = want_kept(eng, ids, user)
        ks = np.array([score[ids.index(i)] for i in kept])
        boosted, _ = ref.boost(SCENE_BOOST, False, ks, {}, np.ones(len(kept), dtype=bool), user)
        order = np.argsort(-boosted, kind="stable")[:40]                               # (the scores are distinct: any order of ties would do)
        assert len(set(boosted.tolist())) == len(kept) and 40 < len(kept) < 300
        assert [x["item_id"] for x in got] == [kept[k] for k in order]
        assert [x["score"] for x in got] == [float(boosted[k]) for k in order]
