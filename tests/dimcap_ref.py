"""The value cap (DimensionFieldUniqueFilter, one dimension of GroupWeightCountFilter's size limit) and DistinctIdSort, each stated
twice — no GPU, no library:

  array form   numpy over the whole list: an entry's occurrence index among the entries of its value decides (the first `limit`
               occurrences of a value are the kept ones), ids by the first matching rule of a match matrix;
  Go form      the reference's loops item by item over dicts and strings (filter/dimension_field_unique_filter.go:39-50,
               filter/group_weight_count_filter.go:290-301 for one dimension, sort/distinct_id_sort.go:56-67): an id is rendered as a
               string, null as "" — what StringProperty returns for a missing property.

Shared by tests/test_dimcap_cpu.py (the two agree with each other and with the library's host statements) and
tests/test_gpu_dimcap.py (the kernels agree with them)."""
import numpy as np

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
NAN = np.uint64(0x7FF8000000000000)
NULL_KEEP, NULL_VALUE = 0, 1
HASH_MUL = 0x9E3779B97F4A7C15


def live_mask(rows, count):
    """[nq][cap] bool: the real entries — in front of min(count[q], cap), row other than UINT64_MAX"""
    rows = np.asarray(rows, dtype=np.uint64)
    nq, cap = rows.shape
    n_valid = np.full(nq, cap) if count is None else np.minimum(np.asarray(count, dtype=np.int64), cap)
    return (np.arange(cap)[None, :] < n_valid[:, None]) & (rows != PAD)


def null_mask(keys, item_in, null_value):
    keys = np.asarray(keys, dtype=np.int64)
    null = np.zeros(keys.shape, dtype=bool) if item_in is None else (np.asarray(item_in) == 0)
    return null if null_value is None else (null | (keys == np.int64(null_value)))


# ---- array form ----------------------------------------------------------------------------------------------------------------
def keep_array(keys, item_in, rows, count, limit, null_mode, null_value):
    """[nq][cap] bool: kept iff real and (null under NULL_KEEP, or among the first `limit` occurrences of its value)"""
    keys = np.asarray(keys, dtype=np.int64)
    live, null = live_mask(rows, count), null_mask(keys, item_in, null_value)
    keep = np.zeros(keys.shape, dtype=bool)
    for q in range(keys.shape[0]):
        counted = live[q] & ~null[q] if null_mode == NULL_KEEP else live[q]
        if null_mode == NULL_KEEP:
            keep[q] = live[q] & null[q]
        idx = np.flatnonzero(counted)
        if idx.size == 0:
            continue
        k, isnull = np.where(null[q, idx], 0, keys[q, idx]), null[q, idx]
        order = np.lexsort((idx, k, isnull))                             # groups by (null, value), positions ascending inside
        ks, ns = k[order], isnull[order]
        start = np.ones(idx.size, dtype=bool)
        start[1:] = (ks[1:] != ks[:-1]) | (ns[1:] != ns[:-1])
        first = np.maximum.accumulate(np.where(start, np.arange(idx.size), 0))
        occ = np.arange(idx.size) - first
        keep[q, idx[order]] = occ < limit
    return keep


def compact(keep, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None):
    """the kept entries moved to the front with everything carried, padding behind as ItemStateFilter pads → (rows, score,
    source, planes_f64, source_mask, planes_f32, count) as Context.candidates_dimcap returns them"""
    rows = np.asarray(rows, dtype=np.uint64)
    nq, cap = rows.shape
    sb = np.ascontiguousarray(score, dtype=np.float64).view(np.uint64)
    p64 = None if planes_f64 is None else np.ascontiguousarray(planes_f64, dtype=np.float64).view(np.uint64)
    p32 = None if planes_f32 is None else np.ascontiguousarray(planes_f32, dtype=np.float32).view(np.uint32)
    o_rows, o_score = np.full((nq, cap), PAD, dtype=np.uint64), np.full((nq, cap), NAN, dtype=np.uint64)
    o_src = None if source is None else np.full((nq, cap), 0xFF, dtype=np.uint8)
    o_mask = None if source_mask is None else np.zeros((nq, cap), dtype=np.uint32)
    o_p64 = None if p64 is None else np.full(p64.shape, NAN, dtype=np.uint64)
    o_p32 = None if p32 is None else np.zeros(p32.shape, dtype=np.uint32)
    o_cnt = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        idx = np.flatnonzero(keep[q])
        k = idx.size
        o_rows[q, :k], o_score[q, :k] = rows[q, idx], sb[q, idx]
        if o_src is not None:
            o_src[q, :k] = np.asarray(source)[q, idx]
        if o_mask is not None:
            o_mask[q, :k] = np.asarray(source_mask)[q, idx]
        if o_p64 is not None:
            o_p64[:, q, :k] = p64[:, q, idx]
        if o_p32 is not None:
            o_p32[:, q, :k] = p32[:, q, idx]
        o_cnt[q] = k
    return (o_rows, o_score.view(np.float64), o_src, None if o_p64 is None else o_p64.view(np.float64), o_mask,
            None if o_p32 is None else o_p32.view(np.float32), o_cnt)


def dimcap(keys, item_in, limit, null_mode, null_value, rows, score, source=None, count=None, planes_f64=None, source_mask=None,
           planes_f32=None):
    return compact(keep_array(keys, item_in, rows, count, limit, null_mode, null_value), rows, score, source, count, planes_f64,
                   source_mask, planes_f32)


def distinct_ids_array(match, ids, live=None):
    """match [n_rules][n] bool, ids [n_rules] → [n] int64: the first matching rule's id, else position + 1; padding 0"""
    match = np.asarray(match, dtype=bool)
    n = match.shape[1]
    ids = np.asarray(ids, dtype=np.int64)
    out = np.where(match.any(axis=0), ids[np.argmax(match, axis=0)], np.arange(1, n + 1, dtype=np.int64))
    return out if live is None else np.where(live, out, 0)


# ---- Go form -------------------------------------------------------------------------------------------------------------------
def string_property(item, field):
    """Item.StringProperty: the property rendered as a string, "" where the item has none"""
    v = item["properties"].get(field)
    return "" if v is None else str(v)


def go_dimension_field_unique(items, field):
    """dimension_field_unique_filter.go:36-50"""
    new_items, uniq = [], {}
    for item in items:
        val = string_property(item, field)
        if val == "":
            new_items.append(item)
        else:
            if val not in uniq:
                uniq[val] = item
                new_items.append(item)
    return new_items


def go_group_weight_dimension(items, dimension, size_limit):
    """group_weight_count_filter.go:289-301 for one dimension, then :310-314"""
    items = list(items)
    group = {}
    for i, item in enumerate(items):
        if item is not None:
            value = string_property(item, dimension)
            if value == "":
                value = "__DEFAULT__"
            if len(group.get(value, [])) + 1 > size_limit:
                items[i] = None
            else:
                group.setdefault(value, []).append(item)
    return [item for item in items if item is not None]


def go_distinct_id_sort(items, conditions, evaluate):
    """distinct_id_sort.go:56-67; conditions: [(rule, distinct_id, distinct_id_name)], evaluate(rule, i, item) → (flag, err)"""
    for i, item in enumerate(items):
        distinct_id = i + 1
        for rule, cid, name in conditions:
            flag, err = evaluate(rule, i, item)
            if err is None and flag:
                item["properties"][name] = cid
                break
            else:
                item["properties"][name] = distinct_id
    return items


def keep_go(keys, item_in, rows, count, limit, null_mode, null_value):
    """keep_array's answer by the Go loops: the real entries of a request become items whose one property is the id as a string
    (none for a null entry); NULL_KEEP with limit 1 runs DimensionFieldUniqueFilter, NULL_VALUE the size limit of one dimension.
    (NULL_KEEP above limit 1 has no loop of its own in the reference: the null items are set aside, the rest goes through the
    size limit, and the survivors are put back in order.)"""
    keys = np.asarray(keys, dtype=np.int64)
    live, null = live_mask(rows, count), null_mask(keys, item_in, null_value)
    keep = np.zeros(keys.shape, dtype=bool)
    for q in range(keys.shape[0]):
        items = [{"pos": int(p), "properties": {} if null[q, p] else {"dim": str(int(keys[q, p]))}} for p in np.flatnonzero(live[q])]
        if null_mode == NULL_VALUE:
            kept = go_group_weight_dimension(items, "dim", limit)
        elif limit == 1:
            kept = go_dimension_field_unique(items, "dim")
        else:
            kept = [it for it in items if not it["properties"]] + go_group_weight_dimension([it for it in items if it["properties"]], "dim", limit)
        keep[q, [it["pos"] for it in kept]] = True
    return keep


# ---- the table's probe, for tests that build colliding keys ----------------------------------------------------------------------
def slots_of(cap):
    return max(2 * cap, 1024)


def first_slot(key, slots):
    """where the probe of `key` starts (include/pairec_gpu.h states it)"""
    return ((((int(key) & 0xFFFFFFFFFFFFFFFF) * HASH_MUL & 0xFFFFFFFFFFFFFFFF) >> 32) * slots) >> 32


def colliding_keys(cap, n, start=1):
    """n distinct positive keys whose probes all start at the slot of the first"""
    slots = slots_of(cap)
    ks = np.arange(start, start + 4 * n * slots, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = (((ks * np.uint64(HASH_MUL)) >> np.uint64(32)) * np.uint64(slots)) >> np.uint64(32)
    out = ks[h == h[0]][:n].astype(np.int64)
    assert out.size == n and all(first_slot(k, slots) == first_slot(start, slots) for k in out[:4])
    return out
