"""The hot table and the request grid shared by tests/test_hot_cpu.py (pg_hot_recall_host) and tests/test_gpu_hot.py (the device
calls): the smallest shapes at which the list recall's kernel can go wrong — lists at the wave, workgroup and tier edges, ties
across list boundaries, special scores, every source form, the three modes' branches, and one batch of 256 mixed requests."""
import functools

import numpy as np

import hot_ref as ref

ROWS, DIM, ROW_OFFSET = 70000, 64, 4_000_000_000      # (64: the narrowest table the library creates; only rows and generation matter)
U32MAX = 0xFFFFFFFF
N_TRIGGERS = 300
GROUP, GLOBAL, TOPIC = ref.GROUP, ref.GLOBAL, ref.TOPIC

# trigger indices of the crafted lists
T_EMPTY, T_ONE, T_63, T_64, T_65, T_1023, T_1024, T_1025, T_8191, T_8192, T_8193, T_MAX, T_EXTRA = range(13)
T_TIE_A, T_TIE_B, T_TIE_C, T_TIE_D, T_SPECIAL, T_SOURCES, T_UNSCORED, T_MIXED = range(13, 21)
T_SINGLES = 21                      # 256 triggers of one entry each: 21 .. 276
T_2000, T_3000, T_TOPIC_10, T_TOPIC_3, T_TOPIC_0 = 277, 278, 279, 280, 281
T_LATE = 285                        # uploaded by a second call; 282 .. 284 are skipped, 286 .. 299 never uploaded
SPECIAL = [-0.0, 0.0, 5e-324, -5e-324, 2.2250738585072009e-308, 1.7e308, -1.7e308, -1.0, -2.5, 16777216.0, 16777217.0, 16777218.0,
           0.0, -0.0, 1.0, 3.0000000000000004, 3.0, 9007199254740993.0, 9007199254740992.0]


def _random_list(rng, n, tie_pool=0):
    """n entries: rows anywhere in the table (duplicates allowed), scores with many ties when tie_pool > 0, sources mixed"""
    rows = rng.integers(0, ROWS, n, dtype=np.uint32)
    sc = rng.integers(0, tie_pool, n).astype(np.float64) if tie_pool else rng.normal(0, 1000, n)
    src = rng.integers(0, 127, n).astype(np.uint8)
    un = rng.random(n) < 0.1
    sc[un] = 0.0
    src[un] |= ref.UNSCORED
    return rows, sc, src


@functools.lru_cache(maxsize=None)
def table():
    """→ [(trig0, offsets, rows, scores, source)] the two uploads, and the whole CSR (offsets [N_TRIGGERS + 1], rows, scores, source)"""
    rng = np.random.default_rng(20260117)
    lists = {}
    for t, n in ((T_EMPTY, 0), (T_ONE, 1), (T_63, 63), (T_64, 64), (T_65, 65), (T_1023, 1023), (T_1024, 1024), (T_1025, 1025), (T_EXTRA, 1),
                 (T_2000, 2000), (T_3000, 3000), (T_TOPIC_10, 10), (T_TOPIC_3, 3), (T_TOPIC_0, 0), (T_LATE, 7)):
        lists[t] = _random_list(rng, n)
    for t, n in ((T_8191, 8191), (T_8192, 8192), (T_8193, 8193), (T_MAX, 65536)):
        lists[t] = _random_list(rng, n, tie_pool=997)           # integer scores: every value is shared by many entries
    for t, n, v in ((T_TIE_A, 5000, 7.0), (T_TIE_B, 5000, 7.0), (T_TIE_C, 40, -3.0), (T_TIE_D, 40, -3.0)):
        lists[t] = (rng.integers(0, ROWS, n, dtype=np.uint32), np.full(n, v), np.zeros(n, np.uint8))
    lists[T_SPECIAL] = (np.arange(100, 100 + len(SPECIAL), dtype=np.uint32), np.array(SPECIAL, np.float64), np.full(len(SPECIAL), 3, np.uint8))
    # sources 0, 1 and 126, each scored and unscored; rows at both ends of the table
    lists[T_SOURCES] = (np.array([0, ROWS - 1, 5, 6, 7, 8], np.uint32), np.array([2.0, 0.0, 1.0, 0.0, 3.0, 0.0]),
                        np.array([0, 0x80, 1, 0x81, 126, 0x80 | 126], np.uint8))
    lists[T_UNSCORED] = (rng.integers(0, ROWS, 300, dtype=np.uint32), np.zeros(300), np.full(300, 0x80, np.uint8))
    mixed = _random_list(rng, 301)
    mixed[1][:] = np.where(mixed[2] & ref.UNSCORED, 0.0, rng.random(301))   # scores in [0, 1): they interleave with the draws
    lists[T_MIXED] = mixed
    for i in range(256):
        lists[T_SINGLES + i] = (np.array([(i * 271) % ROWS], np.uint32), np.array([float(i % 17)]), np.array([i % 127], np.uint8))
    order = sorted(lists)
    off = np.zeros(N_TRIGGERS + 1, np.uint64)
    at = 0
    for t in range(N_TRIGGERS):
        off[t] = at
        at += len(lists[t][0]) if t in lists else 0
    off[N_TRIGGERS] = at
    rows = np.concatenate([lists[t][0] for t in order]).astype(np.uint32)
    sc = np.concatenate([lists[t][1] for t in order]).astype(np.float64)
    src = np.concatenate([lists[t][2] for t in order]).astype(np.uint8)
    # the uploads: triggers 0 .. 281 with offsets that start past 0, then trigger T_LATE alone
    first = off[:T_TOPIC_0 + 2].copy()
    n_first = int(first[-1])
    pad = 3
    up1 = (0, first + pad, np.concatenate([np.zeros(pad, np.uint32), rows[:n_first]]), np.concatenate([np.full(pad, np.nan), sc[:n_first]]),
           np.concatenate([np.full(pad, 0xFF, np.uint8), src[:n_first]]))
    up2 = (T_LATE, np.array([0, 7], np.uint64), rows[n_first:], sc[n_first:], src[n_first:])
    assert len(rows) == n_first + 7
    return (up1, up2), (off, rows, sc, src)


def _seq(a, b):
    return list(range(a, b))


# name → (mode, triggers [nq][...], values [nq][...] | None, seed [nq] | None, k)
@functools.lru_cache(maxsize=None)
def grid():
    g = {}
    absent = [U32MAX, N_TRIGGERS, N_TRIGGERS + 5000, 286, 299, 283]
    for m, mn in ((GROUP, "group"), (GLOBAL, "global"), (TOPIC, "topic")):
        v = (lambda trig: [[1.0] * len(t) for t in trig]) if m == TOPIC else (lambda trig: None)
        trig = [[], absent, [T_EMPTY], [T_EMPTY, U32MAX, T_TOPIC_0]]
        g["%s_empty_and_absent" % mn] = (m, trig, v(trig), None, 5)
        g["%s_n1_k1" % mn] = (m, [[T_ONE]], v([[T_ONE]]), None, 1)
        g["%s_k_above_n" % mn] = (m, [[T_63]], v([[T_63]]), None, 100)
        trig = [[T_EMPTY], [T_ONE], [T_63], [T_64], [T_65], [T_LATE]]
        g["%s_wave_edges" % mn] = (m, trig, v(trig), None, 70)
        trig = [[T_1023], [T_1024], [T_1025]]
        g["%s_workgroup_edges" % mn] = (m, trig, v(trig), [9, 8, 7], 1024)      # GLOBAL: n < k, n == k (stored order), n == k + 1 (sorted)
        trig = [[T_64, T_64], [T_SOURCES, T_ONE, T_SOURCES]]
        g["%s_trigger_twice" % mn] = (m, trig, v(trig), None, 200)
        trig = [_seq(T_SINGLES, T_SINGLES + 256)]
        g["%s_256_triggers" % mn] = (m, trig, v(trig), None, 300)
        g["%s_256_triggers_cut" % mn] = (m, trig, v(trig), None, 100)
        g["%s_sources" % mn] = (m, [[T_SOURCES]], v([[T_SOURCES]]), [77], 6)
    for m, mn in ((GROUP, "group"), (GLOBAL, "global")):
        trig = [[T_8191], [T_8192], [T_8193]]
        g["%s_tier_edge" % mn] = (m, trig, None, [1, 2, 3], 16384 if m == GROUP else 8192)   # GLOBAL: n == k stored, n == k + 1 sorted in scratch
        g["%s_tier_edge_k1" % mn] = (m, trig, None, None, 1)
        g["%s_max_entries" % mn] = (m, [[T_MAX]], None, [5], 16384)
        g["%s_ties_across_lists" % mn] = (m, [[T_TIE_C, T_TIE_D], [T_TIE_D, T_TIE_C, T_ONE]], None, None, 60)
        g["%s_ties_across_tier_edge" % mn] = (m, [[T_TIE_A, T_TIE_B]], None, None, 9000)
        g["%s_special_scores" % mn] = (m, [[T_SPECIAL], [T_SPECIAL, T_SPECIAL]], None, None, 30)
    # GLOBAL: draws
    for k in (300, 299):
        g["global_all_unscored_k%d" % k] = (GLOBAL, [[T_UNSCORED], [T_UNSCORED]], None, [0, 0xDEADBEEFCAFEF00D], k)
        g["global_all_unscored_noseed_k%d" % k] = (GLOBAL, [[T_UNSCORED]], None, None, k)
    g["global_mixed_stored"] = (GLOBAL, [[T_MIXED]], None, [0xFFFFFFFFFFFFFFFF], 301)
    g["global_mixed_sorted"] = (GLOBAL, [[T_MIXED], [T_MIXED, T_UNSCORED]], None, [0xFFFFFFFFFFFFFFFF, 12345], 300)
    g["group_mixed"] = (GROUP, [[T_MIXED, T_UNSCORED]], None, [4], 700)              # unscored entries are 0.0: the seed is not read
    # TOPIC: quotas
    trig = [[T_TOPIC_10, T_TOPIC_3, T_TOPIC_0, 299]]
    g["topic_zero_is_half"] = (TOPIC, [[T_TOPIC_10, T_3000]], [[0.0, 1.5]], None, 10)                 # 0.5 / 1.5: 2 and 7
    g["topic_quota_above_length"] = (TOPIC, trig, [[1.0, 6.0, 2.0, 1.0]], None, 10)                   # 1, 6 (list of 3), 2 (empty list), absent
    g["topic_quota_zero"] = (TOPIC, [[T_3000, T_TOPIC_10, T_2000]], [[1e-9, 3.0, 5e-324]], None, 10)
    g["topic_absent_counts_in_total"] = (TOPIC, [[T_TOPIC_10, U32MAX], [T_TOPIC_10]], [[1.0, 3.0], [1.0]], None, 8)
    g["topic_sum_below_k"] = (TOPIC, [[T_3000, T_2000, T_1025]], [[1.0, 1.0, 1.0]], None, 1000)       # 333 each: 999 < k
    g["topic_k1"] = (TOPIC, [[T_TOPIC_10], [T_TOPIC_10, T_TOPIC_3], [T_TOPIC_0, T_TOPIC_10]], [[2.0], [1.0, 1.0], [0.0, 7.0]], None, 1)
    g["topic_huge_values"] = (TOPIC, [[T_3000, T_2000], [T_3000, T_2000]], [[1.7e308, 1.7e308], [1.7e308, 1.0]], None, 100)   # total = inf; one share of 1
    g["topic_long_lists"] = (TOPIC, [[T_MAX, T_8193, T_TIE_A]], [[5.0, 3.0, 2.0]], None, 16384)
    # one batch of 256: empty, tiny, LDS tier and scratch tier in one call
    kinds = ([], [T_ONE], [T_1023, T_65], [T_8193, T_SINGLES + 3])
    trig = [list(kinds[q % 4]) + ([T_SINGLES + q] if q % 8 >= 4 else []) for q in range(256)]
    g["group_batch_256"] = (GROUP, trig, None, None, 128)
    g["global_batch_256"] = (GLOBAL, trig, None, list(range(1000, 1256)), 1088)       # n = 1088 and 1089 around k
    return g


@functools.lru_cache(maxsize=None)
def expected(name):
    """the case's answer by tests/hot_ref.py, computed once"""
    mode, trig, values, seed, k = grid()[name]
    off, rows, sc, src = table()[1]
    return ref.recall(ROWS, ROW_OFFSET, off, rows, sc, src, mode, trig, k, values, seed)


# requests beyond PG_HOT_MAX_ENTRIES: (triggers, the request the refusal names)
TOO_LONG = (([[T_MAX, T_EXTRA]], 0), ([[T_ONE], [T_MAX, T_ONE], [T_MAX, T_MAX]], 1))


def bad_uploads():
    """name → (offsets, rows, scores, source) for a table of ROWS rows: each must be refused with PG_ERR_INVALID"""
    ok = (np.array([0, 2, 3], np.uint64), np.array([1, 2, 3], np.uint32), np.array([1.0, 0.0, 2.0]), np.array([0, 0x80, 5], np.uint8))

    def edit(i, at, v):
        a = [x.copy() for x in ok]
        a[i][at] = v
        return tuple(a)

    return {
        "row_outside": edit(1, 2, ROWS),
        "nan_score": edit(2, 0, np.nan),
        "inf_score": edit(2, 2, -np.inf),
        "pad_source": edit(3, 0, 0xFF),
        "unscored_with_score": edit(2, 1, 0.25),
        "offsets_descend": (np.array([0, 3, 2], np.uint64),) + ok[1:],
        "list_too_long": (np.array([0, 65537], np.uint64), np.zeros(65537, np.uint32), np.zeros(65537), np.zeros(65537, np.uint8)),
    }
