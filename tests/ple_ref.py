"""The PG_MODEL_PLE specification (include/pairec_gpu.h) in numpy, written the naive way: every expert a dense layer over its
group's input, every gate a max-subtracted softmax over the experts it may see, every mix a weighted sum, every tower a dense
layer, a dot and a sigmoid.  Nothing is permuted or packed, so agreement with it checks the loader's row orders (rank_model.hpp)
as well as the kernel (rank_ple.hip)."""
import numpy as np

from oracle import oracle as o


def ple_scores(w, d_user, table, user_vecs, cand_rows, req_offsets, dtype=np.float64, bf16=False, trace=None):
    """scores [n_task][n_items].  w: {"levels": [per level the blob's arrays by name: we_t [T][E_t][in][h_e], we_s [E_s][in][h_e],
    be_t, be_s, wg_t [T][in][E_t + E_s], bg_t and, below the last level, wg_s [in][T E_t + E_s], bg_s], "wt" [T][h_e][h_t], "bt",
    "wo" [T][h_t], "bo" [T]}.  dtype float32 evaluates the same formula in single precision; bf16 applies the BF16 form's rounding
    points — the candidate row, every weight matrix, each x1_g and each x_t in front of its tower, once each (the two CPU
    evaluations the tests' bars come from).  trace: a dict that receives the largest |gate logit| of every level."""
    rnd = o.f32_to_bf16_round if bf16 else (lambda a: a)
    t = lambda a: np.asarray(a, dtype=dtype)   # noqa: E731
    table = t(rnd(table))
    rows = table.shape[0]
    levels = w["levels"]
    wt, bt, wo, bo = t(rnd(w["wt"])), t(w["bt"]), t(w["wo"]), t(w["bo"]).reshape(-1)
    T = wt.shape[0]
    out = np.zeros((T, len(cand_rows)), dtype=dtype)

    def mix(x, wg, bg, acts, level):
        z = x @ t(rnd(wg)) + t(bg)                                                  # [n][k]
        if trace is not None:
            trace[level] = max(trace.get(level, 0.0), float(np.abs(z).max(initial=0.0)))
        g = np.exp(z - z.max(axis=1, keepdims=True))
        g = g / g.sum(axis=1, keepdims=True)
        return np.einsum("nk,knh->nh", g, np.concatenate(acts, axis=0))

    for r in range(len(req_offsets) - 1):
        i0, i1 = int(req_offsets[r]), int(req_offsets[r + 1])
        e = table[np.minimum(np.asarray(cand_rows[i0:i1], dtype=np.int64), rows - 1)]           # past the table: the last row
        x = np.concatenate([np.broadcast_to(t(user_vecs[r]), (e.shape[0], d_user)), e], axis=1)  # [n][din]
        xs = [x] * (T + 1)
        for lv, w_l in enumerate(levels):
            dense = lambda x_g, we, be: np.maximum(np.einsum("nd,kdh->knh", x_g, t(rnd(we))) + t(be)[:, None, :], 0)   # noqa: E731
            a = [dense(xs[g], w_l["we_t"][g], w_l["be_t"][g]) for g in range(T)] + [dense(xs[T], w_l["we_s"], w_l["be_s"])]
            new = [mix(xs[g], w_l["wg_t"][g], w_l["bg_t"][g], [a[g], a[T]], lv) for g in range(T)]
            if lv + 1 < len(levels):
                new.append(mix(xs[T], w_l["wg_s"], w_l["bg_s"], a, lv))
            xs = [t(rnd(v)) for v in new]
        for g in range(T):
            h = np.maximum(xs[g] @ wt[g] + bt[g], 0)
            out[g, i0:i1] = 1 / (1 + np.exp(-(h @ wo[g] + bo[g])))
    return out
