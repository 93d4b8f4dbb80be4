"""The PG_MODEL_MMOE specification (include/pairec_gpu.h) in numpy, written the naive way: every expert a dense layer, every gate
a max-subtracted softmax, the mix a weighted sum, every tower a dense layer, a dot and a sigmoid.  Nothing is permuted or packed,
so agreement with it checks the loader's row orders (rank_model.hpp) as well as the kernel (rank_mmoe.hip)."""
import numpy as np

from oracle import oracle as o


def mmoe_scores(w, d_user, table, user_vecs, cand_rows, req_offsets, dtype=np.float64, bf16=False):
    """scores [n_task][n_items].  w: the blob's arrays by name (we [E][din][h_e], be, wg [T][din][E], bg, wt [T][h_e][h_t], bt,
    wo [T][h_t], bo [T]).  dtype float32 evaluates the same formula in single precision; bf16 applies the BF16 form's rounding
    points — the candidate row, every weight matrix and each m_t, once each (the two CPU evaluations the tests' bars come from)."""
    rnd = o.f32_to_bf16_round if bf16 else (lambda a: a)
    t = lambda a: np.asarray(a, dtype=dtype)   # noqa: E731
    table = t(rnd(table))
    rows = table.shape[0]
    we, wg, wt = t(rnd(w["we"])), t(rnd(w["wg"])), t(rnd(w["wt"]))
    be, bg, bt, wo, bo = t(w["be"]), t(w["bg"]), t(w["bt"]), t(w["wo"]), t(w["bo"]).reshape(-1)
    out = np.zeros((wt.shape[0], len(cand_rows)), dtype=dtype)
    for r in range(len(req_offsets) - 1):
        i0, i1 = int(req_offsets[r]), int(req_offsets[r + 1])
        e = table[np.minimum(np.asarray(cand_rows[i0:i1], dtype=np.int64), rows - 1)]           # past the table: the last row
        x = np.concatenate([np.broadcast_to(t(user_vecs[r]), (e.shape[0], d_user)), e], axis=1)  # [n][din]
        a = np.maximum(np.einsum("nd,kdh->knh", x, we) + be[:, None, :], 0)                      # [E][n][h_e]
        z = np.einsum("nd,tdk->tnk", x, wg) + bg[:, None, :]                                     # [T][n][E]
        g = np.exp(z - z.max(axis=2, keepdims=True))
        g = g / g.sum(axis=2, keepdims=True)
        m = t(rnd(np.einsum("tnk,knh->tnh", g, a)))                                              # [T][n][h_e]
        h = np.maximum(np.einsum("tnh,thj->tnj", m, wt) + bt[:, None, :], 0)                     # [T][n][h_t]
        out[:, i0:i1] = 1 / (1 + np.exp(-(np.einsum("tnj,tj->tn", h, wo) + bo[:, None])))
    return out
