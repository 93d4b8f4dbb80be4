"""A sequential restatement of MultiRecallMixSort's specification (include/pairec_gpu.h: pg_mix_sort_dev): plain
Python, one entry at a time, in the steps the header numbers.  tests/test_mixsort_cpu.py holds it against a literal transcription
of the Go loops; the host statement (pg_mix_sort_host) and the kernels are held against it by bits.

A strategy is the reference's MixSortConfig as JSON: {"MixStrategy", "Positions", "PositionField", "Number", "NumberRate",
"RecallNames" | "SourceMask", "Conditions"}; string values in conditions are dictionary ids already (cond_ref.py)."""
import numpy as np

import cond_ref

EMPTY = 0xFFFFFFFF
M64 = (1 << 64) - 1


def draw(seed, s, j):
    """the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 * (1 + s * 65536 + j), in uint64 arithmetic"""
    x = (int(seed) + 0x9E3779B97F4A7C15 * (1 + s * 65536 + j)) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def number_of(st, S):
    """number_s (mix_sort_strategy.go:121-176)"""
    if st["MixStrategy"] == "fix_position":
        if st.get("Positions"):
            return len(st["Positions"])
        return st.get("Number", 0) if st.get("Number", 0) > 0 else 0
    if st.get("NumberRate", 0.0) > 0:
        return int(float(S) * st["NumberRate"])
    return st.get("Number", 0) if st.get("Number", 0) > 0 else 0


def mix_list(strategies, S, n, member, pos_vals, seed=0, remain=False, draw_fn=draw):
    """One request over list positions 0 .. n-1.  member[s][j]: entry j is a member of strategy s; pos_vals[s][j]: the value of
    strategy s's position column at entry j (-1 = missing), or pos_vals[s] None → the list positions of the answer (count = its
    length)."""
    if n < S:                                                            # 1.
        return list(range(n))
    number = [number_of(st, S) for st in strategies]
    taken = [False] * n                                                  # 3.
    lists = []
    for s in range(len(strategies)):
        mine = []
        for j in range(n):
            if len(mine) >= number[s]:
                break
            if member[s][j] and not taken[j]:
                taken[j] = True
                mine.append(j)
        lists.append(mine)
    D = [j for j in range(n) if not taken[j]][:S]
    res = [None] * S
    for s, st in enumerate(strategies):                                  # 4.
        if st["MixStrategy"] != "fix_position":
            continue
        if st.get("Positions"):
            P = list(st["Positions"])
        elif st.get("PositionField"):
            P = [int(pos_vals[s][lists[s][j]]) for j in range(min(number[s], len(lists[s])))]
            P = [p for p in P if p > 0]
        else:
            P = []
        idx = 0
        for p in P:
            if p <= S and idx < len(lists[s]):
                res[p - 1] = lists[s][idx]
                idx += 1
    for s, st in enumerate(strategies):                                  # 5.
        if st["MixStrategy"] != "random_position":
            continue
        start = 0
        for j, e in enumerate(lists[s]):
            if all(r is not None for r in res):
                break
            step = S // number[s]
            end = min(start + draw_fn(seed, s, j) % step, S - 1)
            while res[end] is not None:
                end = (end + 1) % S
            res[end] = e
            start += step
    k = 0                                                                # 6.
    for slot in range(S):
        if res[slot] is None and k < len(D):
            res[slot] = D[k]
            k += 1
    inres = set(r for r in res if r is not None)                         # 7.
    rest = (j for j in range(n) if j not in inres)
    for slot in range(S):
        if res[slot] is None:
            res[slot] = next(rest)
    if remain:                                                           # 8.
        inres = set(res)
        res = res + [j for j in range(n) if j not in inres]
    return res


def source_mask(st, recall_names=()):
    mask = int(st.get("SourceMask", 0) or 0)
    for name in st.get("RecallNames") or ():
        if name in recall_names and list(recall_names).index(name) < 32:
            mask |= 1 << list(recall_names).index(name)
    return mask


def members(strategies, elems, cols, item_in, source, user, recall_names=()):
    """member[s][j] for the list whose entry j is element elems[j]; cols {name: element-aligned values}"""
    out = []
    for st in strategies:
        mask = source_mask(st, recall_names)
        conds = st.get("Conditions") or ()
        row = []
        for e in elems:
            src = int(source[e]) if source is not None else 0xFF
            m = src < 32 and (mask >> src) & 1 == 1
            if not m and conds:
                m = cond_ref.match(conds, e, cols, item_in, user or {})
            row.append(bool(m))
        out.append(row)
    return out


def mix_sort(strategies, size, remain, ctx_size, nq, cap, cols=None, item_in=None, source=None, order=None, count=None, seed=None, users=None,
             recall_names=()):
    """The whole answer on [nq][cap] arrays, as pg_mix_sort_host takes them → (out_order [nq][cap] uint32, out_count [nq] uint32)."""
    S = max(int(ctx_size), int(size))
    out = np.full((nq, cap), EMPTY, dtype=np.uint32)
    cnt = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        n = cap if count is None else min(int(count[q]), cap)
        elems = [int(order[q][j]) if order is not None else j for j in range(n)]
        cq = {k: np.asarray(v).reshape(nq, cap)[q] for k, v in (cols or {}).items()}
        iq = None if item_in is None else np.asarray(item_in).reshape(nq, cap)[q].astype(bool)
        sq = None if source is None else np.asarray(source).reshape(nq, cap)[q]
        mem = members(strategies, elems, cq, iq if iq is not None else np.ones(cap, bool), sq, None if users is None else users[q], recall_names)
        pos = []
        for st in strategies:
            f = st.get("PositionField")
            if st["MixStrategy"] == "fix_position" and not st.get("Positions") and f:
                pos.append([int(cq[f][e]) if (iq is None or iq[e]) else -1 for e in elems])
            else:
                pos.append(None)
        res = mix_list(strategies, S, n, mem, pos, 0 if seed is None else int(seed[q]), remain)
        out[q, :len(res)] = [elems[j] for j in res]
        cnt[q] = len(res)
    return out, cnt
