"""The host mirror's TrafficControlSort entry (pairec_gpu.Sorts, SortType "TrafficControlSort"): the config is
accepted in the reference's shape and a bad entry fails by name (no GPU needed); on the GPU the sort runs the targets'
ItemExpressions as class masks over the engine's item_features store and pg_traffic_sort, tags the items, and the alpha setter
changes the next request's order."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

import pairec_amd as pa

import traffic_cases as cases
import traffic_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 2000
TARGETS = [{"TrafficControlTargetId": "71", "ControlType": "Percent", "ItemExpression": "category == 3 || brand in (1, 2)", "Alpha": 6.0},
           {"TrafficControlTargetId": "72", "ControlType": "Quantity", "ItemExpression": "category < 2", "Alpha": -8.0},
           {"TrafficControlTargetId": 73, "ControlType": "Quantity", "Alpha": 0.0}]
CONFIG = {
    "RunMode": "product", "AlgoConfs": [], "RecallConfs": [],
    "SceneConfs": {"feed": {"default": {"RecallNames": ["u2i"]}}},
    "SortConfs": [{"Name": "host_traffic", "SortType": "TrafficControlSort"}],
    "UserDefineConfs": {"pairec_gpu": {
        "Device": 0, "Table": {"Rows": ROWS, "Dim": 128, "IdPrefix": "item_", "SyntheticSeed": 1},
        "Recalls": [{"Name": "u2i", "Kind": "vector", "RecallCount": 50, "RecallAlgo": "gpu_faiss", "ItemType": "video"}],
        "Algorithms": [{"Name": "gpu_faiss", "Kind": "faiss"}],
        "Sorts": [{"Name": "traffic", "SortType": "TrafficControlSort", "Targets": TARGETS, "PidEta": 0.05},
                  {"Name": "traffic_defaults", "SortType": "TrafficControlSort", "Targets": TARGETS[:1]},
                  {"Name": "traffic_no_column", "SortType": "TrafficControlSort",
                   "Targets": [{"TrafficControlTargetId": "1", "ControlType": "Percent", "ItemExpression": "colour == 3", "Alpha": 1.0}]}]}},
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
    L.ph_engine_set_feature_column.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
    L.ph_engine_sort_props.restype = C.c_char_p
    L.ph_engine_sort_props.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    L.ph_engine_set_traffic_alpha.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_double]
    return L


def test_config_accepts_the_entry(H):
    assert H.ph_parse_recconf(json.dumps(CONFIG).encode()), H.ph_last_error()


@pytest.mark.parametrize("edit,words", [
    (lambda s: s[0].update({"Targets": [dict(TARGETS[0], TrafficControlTargetId=str(i)) for i in range(9)]}),
     (b"pairec_gpu.Sorts", b"traffic", b"TrafficControlSort", b"9 Targets")),
    (lambda s: s[0]["Targets"][0].update({"ItemExpression": "category == 3 ? 1 : 2"}), (b"pairec_gpu.Sorts", b"traffic", b"ItemExpression", b"ternary")),
    (lambda s: s[0]["Targets"][1].update({"ItemExpression": "title == 'abc'"}), (b"pairec_gpu.Sorts", b"traffic", b"ItemExpression", b"string literal")),
    (lambda s: s[0]["Targets"][0].update({"TrafficControlTargetId": "seven"}), (b"pairec_gpu.Sorts", b"traffic", b"TrafficControlTargetId", b"seven")),
    (lambda s: s[0]["Targets"][0].update({"TrafficControlTargetId": "-2147483648"}), (b"pairec_gpu.Sorts", b"traffic", b"outside int32")),
    (lambda s: s[0]["Targets"][0].update({"Alpha": "high"}), (b"pairec_gpu.Sorts", b"traffic", b"Alpha is not a number")),
])
def test_a_bad_entry_fails_by_name(H, edit, words):
    cfg = copy.deepcopy(CONFIG)
    edit(cfg["UserDefineConfs"]["pairec_gpu"]["Sorts"])
    assert not H.ph_parse_recconf(json.dumps(cfg).encode())
    for w in words:
        assert w in H.ph_last_error(), H.ph_last_error()


@pytest.mark.gpu
def test_sort_through_the_mirror(H):
    h = H.ph_engine_create(json.dumps(CONFIG).encode())
    assert h, H.ph_last_error()
    try:
        rng = np.random.default_rng(16)
        cols = {"category": rng.integers(0, 6, ROWS).astype(np.int32), "brand": rng.integers(0, 5, ROWS).astype(np.int32)}
        for name, a in cols.items():
            assert H.ph_engine_set_feature_column(h, name.encode(), a.ctypes.data_as(C.c_void_p), ROWS) == 0, H.ph_last_error()
        ids = ["item_%d" % r for r in rng.choice(ROWS, 300, replace=False)] + ["stranger_1", "item_99999999"]
        rng.shuffle(ids)
        scores = rng.permutation(len(ids)).astype(np.float64) / len(ids) + 0.001           # distinct: the score order is defined
        items = [{"id": i, "score": float(s)} for i, s in zip(ids, scores)]
        n, size = len(items), 20
        tabs = cases.tables(pa)
        listed = np.argsort(-scores, kind="stable")
        rows = np.array([int(i[5:]) if i.startswith("item_") and int(i[5:]) < ROWS else ROWS for i in ids], dtype=np.int64)[listed]
        inside = rows < ROWS
        cat, brand = cols["category"][np.where(inside, rows, 0)], cols["brand"][np.where(inside, rows, 0)]
        member = (inside & ((cat == 3) | (brand == 1) | (brand == 2))).astype(np.uint8) | ((inside & (cat < 2)).astype(np.uint8) << 1) | 4
        targets = [(71, ref.PERCENT), (72, ref.QUANTITY), (73, ref.QUANTITY)]

        def expect(alphas, eta=0.05):
            o, cid, pos = ref.request(tabs, targets, size, 1, 1.0, 1.0, eta, list(scores[listed]), list(member), alphas)
            return [ids[listed[i]] for i in o], cid, pos

        def served(name=b"traffic"):
            r = H.ph_engine_sort_props(h, name, json.dumps(items).encode(), b"{}", size)
            assert r, H.ph_last_error()
            return json.loads(r)["items"]

        got = served()
        want, cid, pos = expect([6.0, -8.0, 0.0])
        assert [x["item_id"] for x in got] == want and want != [ids[i] for i in listed]
        by_id = {x["item_id"]: x["properties"] for x in got}
        for i in range(n):
            p = by_id[ids[listed[i]]]
            assert p["__traffic_control_id__"] == cid[i] and p["_ORIGIN_POSITION_"] == i + 1 and p["_NEW_POSITION_"] == pos[i]
        assert any(c == -71 for c in cid)
        # the setter: from the next request on the second target lifts its items instead of pulling them down, and the third
        # (no expression: every item) pulls down
        assert H.ph_engine_set_traffic_alpha(h, b"traffic", b"72", 40.0) == 0, H.ph_last_error()
        assert H.ph_engine_set_traffic_alpha(h, b"traffic", b"73", -30.0) == 0, H.ph_last_error()
        got2 = [x["item_id"] for x in served()]
        want2, _, _ = expect([6.0, 40.0, -30.0])
        assert got2 == want2 and got2 != want
        assert H.ph_engine_set_traffic_alpha(h, b"traffic", b"71", 0.0) == 0 and H.ph_engine_set_traffic_alpha(h, b"traffic", b"72", 0.0) == 0
        assert H.ph_engine_set_traffic_alpha(h, b"traffic", b"73", 0.0) == 0
        assert [x["item_id"] for x in served()] == [ids[i] for i in listed]                 # every alpha 0: the score order
        assert H.ph_engine_set_traffic_alpha(h, b"traffic", b"74", 1.0) != 0 and b'no target "74"' in H.ph_last_error()
        assert H.ph_engine_set_traffic_alpha(h, b"host_traffic", b"71", 1.0) != 0 and b"not find" in H.ph_last_error()
        # the Pid defaults: 1.0, 1.0, 1.6
        assert json.loads(H.ph_engine_sort_props(h, b"traffic_defaults", b"[]", b"{}", size))["items"] == []
        o, _, _ = ref.request(tabs, targets[:1], size, 1, 1.0, 1.0, 1.6, list(scores[listed]), list(member & 1), [6.0])
        assert [x["item_id"] for x in served(b"traffic_defaults")] == [ids[listed[i]] for i in o]
        assert H.ph_engine_sort_props(h, b"traffic_no_column", json.dumps(items).encode(), b"{}", size) is None
        assert b"TrafficControlSort" in H.ph_last_error() and b'"colour" is not a feature column' in H.ph_last_error()
    finally:
        H.ph_engine_destroy(h)
