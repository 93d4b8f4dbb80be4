"""The PG_MODEL_MHA specification (include/pairec_gpu.h) in numpy, written the naive way: per candidate the logits against every
valid position, np.exp after subtracting the global max, a plain weighted sum, Wo and three dense layers.  Nothing is folded,
permuted or streamed, so agreement with it checks the loader's orders (rank_model.hpp: pack_mha) as well as the kernels
(rank_mha.hip)."""
import numpy as np

from oracle import oracle as o


def mha_scores(w, d_user, n_head, table, user_vecs, seqs, cand_rows, req_offsets, dtype=np.float64, bf16_points=False):
    """scores [n_out][n_items].  w: the blob's arrays by name (wq, bq, wk, wv, bv, wo, w1, b1, w2, b2, w3 [h2][n_out], b3).
    dtype float32 evaluates the same formula in single precision; bf16_points rounds exactly the BF16 form's points, once each:
    e as Wq's operand and Wq, q, K and V as stored, the unnormalised p as the P.V operand (the sum l takes the unrounded p), the
    normalised o and Wo — and the points of the PG_PREC_BF16 trunk behind it: w1, w2, and [e | pooled] and h1
    as operands.  The K/V projection, the sums, the max, the exponent, pooled as staged and the user vector are not rounded."""
    t = lambda a: np.asarray(a, dtype=dtype)   # noqa: E731
    op = (lambda a: t(o.f32_to_bf16_round(a))) if bf16_points else t
    table, rows = t(table), table.shape[0]
    wq, wk, wv, wo = op(w["wq"]), t(w["wk"]), t(w["wv"]), op(w["wo"])
    bq, bv, w1, b1, w2, b2 = t(w["bq"]), t(w["bv"]), op(w["w1"]), t(w["b1"]), op(w["w2"]), t(w["b2"])
    w3, b3 = t(w["w3"]).reshape(w2.shape[1], -1), t(w["b3"]).reshape(-1)
    d_att = wq.shape[1]
    d_h = d_att // n_head
    out = np.zeros((b3.shape[0], len(cand_rows)), dtype=dtype)
    for r in range(len(req_offsets) - 1):
        i0, i1 = int(req_offsets[r]), int(req_offsets[r + 1])
        s = table[[x for x in list(seqs[r])[:512] if x < rows]]                # an entry past the table is left out of the softmax
        e = table[np.minimum(np.asarray(cand_rows[i0:i1], dtype=np.int64), rows - 1)]              # [n][64]
        pooled = np.zeros_like(e)
        if len(s) and len(e):
            q, K, V = op(op(e) @ wq + bq), op(s @ wk), op(s @ wv + bv)
            heads = []
            for h in range(n_head):
                c = slice(h * d_h, (h + 1) * d_h)
                a = (q[:, c] @ K[:, c].T) / dtype(np.sqrt(d_h))                                      # [n][L]
                p = np.exp(a - a.max(axis=1, keepdims=True))
                heads.append((op(p) @ V[:, c]) / p.sum(axis=1, keepdims=True))
            pooled = op(np.concatenate(heads, axis=1)) @ wo
        x = np.concatenate([np.broadcast_to(t(user_vecs[r]), (e.shape[0], d_user)), op(e), op(pooled)], axis=1)
        hid = np.maximum(op(np.maximum(x @ w1 + b1, 0)) @ w2 + b2, 0) @ w3 + b3
        out[:, i0:i1] = (1 / (1 + np.exp(-hid))).T
    return out
