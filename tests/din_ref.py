"""The PG_MODEL_DIN specification (include/pairec_gpu.h) in numpy, written the naive way: z_l is built per (candidate, position),
the activation unit is two dense layers, the pooling a weighted sum, the trunk three dense layers and a sigmoid.  Nothing is
folded, so agreement with it checks the loader's fold (rank_model.hpp) as well as the kernel (rank_din.hip)."""
import numpy as np

from oracle import oracle as o


def din_scores(w, d_user, table, user_vecs, seqs, cand_rows, req_offsets, dtype=np.float64, bf16_inputs=False):
    """scores [n_out][n_items].  w: the blob's arrays by name (wa, ba, wa2, ba2, w1, b1, w2, b2, w3 [h2][n_out], b3 [n_out]).
    dtype float32 evaluates the same formula in single precision; bf16_inputs rounds what enters the trunk's first layer from
    the attention side — e, s_l and the attention weights a_l — to bf16 (the two CPU evaluations the tests' bars come from)."""
    rnd = o.f32_to_bf16_round if bf16_inputs else (lambda a: a)
    t = lambda a: np.asarray(a, dtype=dtype)   # noqa: E731
    table = t(rnd(table))
    rows, d = table.shape
    wa, ba, wa2, ba2 = t(w["wa"]), t(w["ba"]), t(w["wa2"]), dtype(w["ba2"])
    w1, b1, w2, b2 = t(w["w1"]), t(w["b1"]), t(w["w2"]), t(w["b2"])
    w3, b3 = t(w["w3"]).reshape(w2.shape[1], -1), t(w["b3"]).reshape(-1)
    out = np.zeros((b3.shape[0], len(cand_rows)), dtype=dtype)
    for r in range(len(req_offsets) - 1):
        s = table[[x for x in list(seqs[r])[:64] if x < rows]]                 # rows outside the table contribute nothing
        for i0 in range(int(req_offsets[r]), int(req_offsets[r + 1]), 4096):
            i1 = min(i0 + 4096, int(req_offsets[r + 1]))
            e = table[np.minimum(np.asarray(cand_rows[i0:i1], dtype=np.int64), rows - 1)]        # [n][d]
            pooled = np.zeros_like(e)
            if len(s):
                eb, sb = e[:, None, :], s[None, :, :]
                z = np.concatenate([eb + 0 * sb, sb + 0 * eb, eb - sb, eb * sb], axis=2)        # [n][L][4 d]
                a = np.maximum(z @ wa + ba, 0) @ wa2 + ba2                                      # [n][L]
                pooled = t(rnd(a)) @ s
            x = np.concatenate([np.broadcast_to(t(user_vecs[r]), (e.shape[0], d_user)), e, pooled], axis=1)
            h = np.maximum(np.maximum(x @ w1 + b1, 0) @ w2 + b2, 0) @ w3 + b3
            out[:, i0:i1] = (1 / (1 + np.exp(-h))).T
    return out
