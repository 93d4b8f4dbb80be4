"""The PG_MODEL_DCN specification (include/pairec_gpu.h) in numpy, written the naive way: x_0 = [user | item] in the blob's order,
every cross layer a dense product, an element-wise product and a residual, the head two dense layers, a dot and a sigmoid.
Nothing is reordered, padded or packed, so agreement with it checks the loader's orders (rank_model.hpp: pack_dcn) as well as the
kernel (rank_dcn.hip)."""
import numpy as np

from oracle import oracle as o


def dcn_scores(w, d_user, table, user_vecs, cand_rows, req_offsets, dtype=np.float64, bf16=False):
    """scores [n_out][n_items].  w: the blob's arrays by name (wc [L][D][D], bc [L][D], w1 [D][h1], b1, w2 [h1][h2], b2,
    w3 [h2][n_out], b3).  dtype float32 evaluates the same formula in single precision; bf16 applies the BF16 form's rounding
    points — the candidate row as layer 0's operand, every weight matrix, x_l (l >= 1), x_L and h1 as operands, once each."""
    rnd = o.f32_to_bf16_round if bf16 else (lambda a: a)
    t = lambda a: np.asarray(a, dtype=dtype)   # noqa: E731
    op = (lambda a: t(rnd(a))) if bf16 else (lambda a: a)   # noqa: E731  (a matrix operand: rounded from its fp32 value)
    table, rows = t(table), table.shape[0]
    wc, w1, w2 = t(rnd(w["wc"])), t(rnd(w["w1"])), t(rnd(w["w2"]))
    bc, b1, b2, w3, b3 = t(w["bc"]), t(w["b1"]), t(w["b2"]), t(w["w3"]).reshape(w2.shape[1], -1), t(w["b3"]).reshape(-1)
    out = np.zeros((w3.shape[1], len(cand_rows)), dtype=dtype)
    for r in range(len(req_offsets) - 1):
        i0, i1 = int(req_offsets[r]), int(req_offsets[r + 1])
        e = table[np.minimum(np.asarray(cand_rows[i0:i1], dtype=np.int64), rows - 1)]           # past the table: the last row
        u = np.broadcast_to(t(user_vecs[r]), (e.shape[0], d_user))
        x0 = np.concatenate([u, e], axis=1)
        x = x0
        for l in range(wc.shape[0]):
            xin = np.concatenate([u, op(e)], axis=1) if l == 0 else op(x)                        # (the user half stays fp32)
            x = x0 * (xin @ wc[l] + bc[l]) + x
        h1 = np.maximum(op(x) @ w1 + b1, 0)
        h2 = np.maximum(op(h1) @ w2 + b2, 0)
        out[:, i0:i1] = (1 / (1 + np.exp(-(h2 @ w3 + b3)))).T
    return out
