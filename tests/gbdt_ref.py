"""PG_MODEL_GBDT restated in plain numpy over POINTER trees (what pa.pack_gbdt takes, not what it makes): values and compares in
float32, the margin a float64 chain in tree order, the sigmoid in float64."""
import numpy as np


def gbdt_margins(trees, base, x, le=False):
    """x [n][n_feat] float32 -> float64 margins.  trees: mappings of feature, threshold, left, right, missing_left, value."""
    x = np.asarray(x, dtype=np.float32)
    rows = np.arange(x.shape[0])
    margin = np.full(x.shape[0], np.float64(np.float32(base)))
    for tr in trees:
        feat, left, right = (np.asarray(tr[k], dtype=np.int64) for k in ("feature", "left", "right"))
        thr, miss = np.asarray(tr["threshold"], dtype=np.float32), np.asarray(tr["missing_left"]) != 0
        node = np.zeros(x.shape[0], dtype=np.int64)
        while (left[node] >= 0).any():
            inner = left[node] >= 0
            v = x[rows, np.where(inner, feat[node], 0)]
            go_left = ((v <= thr[node]) if le else (v < thr[node])) | (np.isnan(v) & miss[node])
            node = np.where(inner, np.where(go_left, left[node], right[node]), node)
        margin += np.asarray(tr["value"], dtype=np.float32)[node].astype(np.float64)
    return margin


def gbdt_scores(margin, objective):
    """objective 1: the margin rounded to float32; objective 0: the float64 sigmoid (the kernel rounds it once more)"""
    return margin.astype(np.float32) if objective else 1.0 / (1.0 + np.exp(-margin))
