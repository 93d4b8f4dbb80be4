"""CPU restatement of the collaborative-filter recall's specification (include/pairec_gpu.h, "Collaborative-filter recall";
DESIGN.md 4.1l): a sequential loop with Python floats, literally.  No GPU, no library.

    for every trigger j of the request, in the order given (a row of UINT32_MAX or >= rows contributes nothing):
        for every entry e of the trigger's list, in stored order:
            term = float(np.float32 sim_e) * prefer_j               # an exact widening, then one rounding
            score[item] = term if the item is new else score[item] + term
    m = the largest score, found with > from 0;  normalize and m > 0:  score = score / m
    order: score descending, then row ascending;  with a list: its ids dropped;  the first k;  padding UINT64_MAX / -inf
"""
import numpy as np

U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


class SimLists:
    """the similarity table on the host: CSR over `rows` local rows (rows never uploaded have empty lists)"""

    def __init__(self, rows, row_offset=0):
        self.rows, self.row_offset = int(rows), int(row_offset)
        self.lists = {}                               # row -> (neighbours [int], similarities [float, widened from float32])

    def upload(self, offsets, nbr, sim, row0=0):
        nbr = np.asarray(nbr, dtype=np.uint32)
        sim = np.asarray(sim, dtype=np.float32)
        for i in range(len(offsets) - 1):
            b, e = int(offsets[i]), int(offsets[i + 1])
            self.lists[row0 + i] = (nbr[b:e].tolist(), [float(x) for x in sim[b:e]])

    def length(self, row):
        return len(self.lists[row][0]) if row in self.lists else 0


def accumulate(sl, triggers, prefer):
    """item -> score after the request's triggers, in the specification's order"""
    score = {}
    for r, p in zip(triggers, prefer):
        r, p = int(r), float(p)
        if r >= sl.rows or r not in sl.lists:
            continue
        nb, sm = sl.lists[r]
        for item, s in zip(nb, sm):
            term = s * p
            if item in score:
                score[item] = score[item] + term
            else:
                score[item] = term
    return score


def ordered(score, normalize):
    """[(row, score)] in the answer's order"""
    m = 0.0
    for s in score.values():
        if s > m:
            m = s
    if normalize and m > 0:
        score = {i: s / m for i, s in score.items()}
    return sorted(score.items(), key=lambda kv: (-kv[1], kv[0]))


def cf_recall(sl, triggers, prefer, k, normalize=True, lists=None):
    """triggers[q], prefer[q] → (rows [nq][k] uint64 global ids, scores [nq][k] float64, counts [nq] uint32)"""
    nq = len(triggers)
    rows = np.full((nq, k), U64MAX, dtype=np.uint64)
    scores = np.full((nq, k), -np.inf, dtype=np.float64)
    counts = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        ans = ordered(accumulate(sl, triggers[q], prefer[q]), normalize)
        if lists is not None:
            seen = set(int(x) for x in lists[q])
            ans = [(i, s) for i, s in ans if sl.row_offset + i not in seen]      # dropping, then cutting
        ans = ans[:k]
        for j, (i, s) in enumerate(ans):
            rows[q, j] = sl.row_offset + i
            scores[q, j] = s
        counts[q] = len(ans)
    return rows, scores, counts
