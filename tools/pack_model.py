#!/usr/bin/env python3
"""pack_model.py — exported rank-model weights (.npz) → the blob pg_model_load takes (include/pairec_gpu.h, "rank: model
predict").  Stand-alone: numpy only, runs wherever the model was trained.

What it replaces on the reference's side: pairec never sees weights — RankConf names an algorithm whose AlgoConfs entry
points at a PAI-EAS / TF-Serving endpoint (algorithm/eas/model.go:38-120: Url, Auth, Processor, ResponseFuncName …) that
holds the SavedModel.  Here the same model's Dense kernels are loaded into HBM, so the deployment step "push the model to
EAS" becomes "pack the kernels, hand the blob to pg_model_load / ph_engine_load_dnn3[_multi]".

Input: an .npz whose arrays are the layers' kernels exactly as a framework saves them — row-major [in][out] fp32 (Keras
`dense.kernel`, PyTorch `linear.weight.T`) — and their biases:

  DNN3 (score = sigmoid(w3 . relu(W2' relu(W1' [user || item_row] + b1) + b2) + b3)):
      w1 [d_user + d_item][h1]   b1 [h1]   w2 [h1][h2]   b2 [h2]   w3 [h2] or [h2][1]   b3 scalar or [1]
  DNN3, several outputs on one trunk (probs_ctr / probs_cvr …: EasyrecResponse.multiValModule, easyrec_response.go:35-70):
      … w3 [h2][n_out]   b3 [n_out]        (n_out 2..8; the algorithm's "Outputs" list names them in this order)
  DIN (PG_MODEL_DIN: attention of each candidate over the user's behaviour sequence, pooled, then the trunk above on
  [user || item_row || pooled]; chosen when the file holds `wa`):
      wa [4*64][att_h] (row blocks e, s, e-s, e*s; att_h 16 or 32)   ba [att_h]   wa2 [att_h] or [att_h][1]   ba2 scalar
      w1 [d_user + 128][h1] (rows: user, item row, pooled)   b1, w2, b2 as above   w3 [h2] or [h2][n_out]   b3 [n_out]
  MMoE (PG_MODEL_MMOE: E gated experts and one tower per task; chosen when the file holds `we`):
      we [E][d_user + d_item][h_e]   be [E][h_e]   wg [T][d_user + d_item][E]   bg [T][E]
      wt [T][h_e][h_t]   bt [T][h_t]   wo [T][h_t] or [T][h_t][1]   bo [T]
      ((E, h_e) one of (2,128) (4,64) (4,128) (8,64); T 1..4; h_t 32 or 64; task t is the algorithm's t-th "Outputs" name)
  PLE (PG_MODEL_PLE: one or two extraction levels of T task groups and a shared group of experts; chosen when the file holds
  `we1_t`; level l = 1, 2 — level 2's arrays only in a two-level model, wg{l}_s / bg{l}_s only below the last level):
      we{l}_t [T][E_t][in][h_e]   we{l}_s [E_s][in][h_e]   be{l}_t [T][E_t][h_e]   be{l}_s [E_s][h_e]   (in = d_user + d_item, then h_e)
      wg{l}_t [T][in][E_t + E_s]   bg{l}_t [T][E_t + E_s]   wg{l}_s [in][T E_t + E_s]   bg{l}_s [T E_t + E_s]
      wt, bt, wo, bo as an MMoE's   (T 1..3; E_t, E_s 1 or 2; h_e 64, or 128 with one level; h_t 32 or 64)
  DCN-v2 (PG_MODEL_DCN: stacked full-rank cross layers x_{l+1} = x_0 * (Wc_l' x_l + bc_l) + x_l, then the trunk above on x_L;
  chosen when the file holds `wc`):
      wc [L][D][D] (D = d_user + d_item <= 256; L 1..3)   bc [L][D]
      w1 [D][h1]   b1, w2, b2 as above ((h1, h2) 128-128 or 256-128)   w3 [h2] or [h2][n_out]   b3 [n_out] (n_out 1..4)
  MHA (PG_MODEL_MHA: multi-head softmax attention of each candidate over the user's behaviour sequence of up to 512 rows, pooled
  through wo, then the trunk above on [user || item_row || pooled]; chosen when the file holds `wq`):
      wq [64][d_att]   bq [d_att]   wk [64][d_att]   wv [64][d_att]   bv [d_att]   wo [d_att][64]   n_head (integer array, or --n-head)
      ((d_att, n_head) one of (64,1) (64,2) (128,2) (128,4); a key bias cancels in the softmax and an output bias belongs in b1)
      w1 [d_user + 128][h1] (rows: user, item row, pooled)   b1, w2, b2 as above   w3 [h2] or [h2][n_out]   b3 [n_out]
  GBDT (PG_MODEL_GBDT: a PS-SMART / xgboost forest; chosen when the file holds `tree_ptr`).  Pointer trees, every array the
  concatenation over trees, tree t's nodes at [tree_ptr[t], tree_ptr[t + 1]) with its root first and child indices local to it:
      feature, threshold, left, right (left < 0: a leaf), missing_left, value   tree_ptr [n_tree + 1]
      n_user_feat, n_item_feat, base, objective (0 logistic, 1 identity), le (optional, 1: PMML lessOrEqual splits) as scalars
      (trees at most 8 deep; a feature indexes [user features | item columns]; no --d-user)
  MIND (PG_MODEL_MIND: a multi-interest user model, the behaviour sequence routed into K capsules; chosen when the file holds
  `routing_init`):
      s [64][64]   routing_init [K][256] (the fixed routing-logit init; K 1..8)   wc [64][h1]   wu [d_user][h1]   b1 [h1]
      w2 [h1][d_out]   b2 [d_out]   n_iter (1..4) and normalize (0 | 1) as scalars   (h1 128 or 256; d_out 64 or 128; no --d-user)
  --d-user N says where the user half of w1 ends (or an integer array `d_user` inside the file); d_item = the table's dim
  (64 or 128).  --map w1=dense/kernel,b1=dense/bias,… renames arrays.  Supported hidden shapes: see the header.

  python tools/pack_model.py model.npz --d-user 128 --out model.blob      → prints kind, shape, bytes
"""
import argparse
import struct
import sys

import numpy as np

DNN3_SHAPES = {(128, 128), (256, 128), (256, 256), (512, 256), (1024, 512)}
KIND_DNN3, KIND_DNN3_MULTI, KIND_DIN, KIND_MMOE, KIND_DCN, KIND_MHA, KIND_PLE, KIND_GBDT, KIND_MIND = 1, 3, 4, 5, 6, 8, 9, 10, 11
MMOE_SHAPES = {(2, 128), (4, 64), (4, 128), (8, 64)}
DCN_HEADS = {(128, 128), (256, 128)}
MHA_SHAPES = {(64, 1), (64, 2), (128, 2), (128, 4)}


def _f32(a, shape=None, what=""):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (what, tuple(a.shape), tuple(shape)))
    if not np.all(np.isfinite(a)):
        raise ValueError("%s holds non-finite values" % what)
    return a


def pack_dnn3_arrays(w1, b1, w2, b2, w3, b3, d_user):
    """→ (kind, blob): PG_MODEL_DNN3 for one output, PG_MODEL_DNN3_MULTI for several (w3 [h2][n_out])."""
    w1 = np.asarray(w1)
    w2 = np.asarray(w2)
    if w1.ndim != 2 or w2.ndim != 2:
        raise ValueError("w1 / w2 must be 2-D [in][out] kernels")
    din, h1 = w1.shape
    if w2.shape[0] != h1:
        raise ValueError("w2 has shape %s: its input width must be w1's output width %d (a [out][in] kernel, e.g. PyTorch's "
                         "linear.weight, has to be transposed)" % (tuple(w2.shape), h1))
    h2 = w2.shape[1]
    d_user = int(d_user)
    d_item = din - d_user
    if not 1 <= d_user <= 4096 or d_item not in (64, 128):
        raise ValueError("w1 has %d input rows: with d_user = %d the item half is %d wide (the table's dim: 64 or 128)" % (din, d_user, d_item))
    if (h1, h2) not in DNN3_SHAPES:
        raise ValueError("hidden widths %d-%d have no kernel (supported: %s)" % (h1, h2, sorted(DNN3_SHAPES)))
    w1, w2 = _f32(w1, what="w1"), _f32(w2, (h1, h2), "w2")
    b1, b2 = _f32(np.reshape(b1, -1), (h1,), "b1"), _f32(np.reshape(b2, -1), (h2,), "b2")
    w3 = np.asarray(w3, dtype=np.float32)
    if w3.ndim == 1:
        w3 = w3.reshape(-1, 1)
    if w3.ndim != 2 or w3.shape[0] != h2:
        raise ValueError("w3 has shape %s, expected [%d] or [%d][n_out]" % (tuple(np.shape(w3)), h2, h2))
    n_out = w3.shape[1]
    b3 = _f32(np.reshape(b3, -1), (n_out,), "b3")
    w3 = _f32(w3, what="w3")
    if n_out == 1:
        blob = (struct.pack("<4I", d_user, d_item, h1, h2) + w1.tobytes() + b1.tobytes() + w2.tobytes() + b2.tobytes() +
                w3.reshape(-1).tobytes() + b3.tobytes())
        return KIND_DNN3, blob
    if not 2 <= n_out <= 8:
        raise ValueError("%d outputs (a multi-output DNN3 has 2..8)" % n_out)
    blob = (struct.pack("<5I", d_user, d_item, h1, h2, n_out) + w1.tobytes() + b1.tobytes() + w2.tobytes() + b2.tobytes() +
            w3.tobytes() + b3.tobytes())
    return KIND_DNN3_MULTI, blob


def pack_din_arrays(wa, ba, wa2, ba2, w1, b1, w2, b2, w3, b3, d_user):
    """→ (KIND_DIN, blob): the activation unit's arrays in front of the trunk's, the trunk checked as a 128-wide DNN3."""
    wa = np.asarray(wa)
    if wa.ndim != 2 or wa.shape[0] != 256 or wa.shape[1] not in (16, 32):
        raise ValueError("wa has shape %s, expected [256][att_h] with att_h 16 or 32 (a 64-wide item table)" % (tuple(wa.shape),))
    att_h = wa.shape[1]
    kind, trunk = pack_dnn3_arrays(w1, b1, w2, b2, w3, b3, d_user)
    d_user_, d_item, h1, h2 = struct.unpack("<4I", trunk[:16])
    if d_item != 128:
        raise ValueError("w1 has %d rows behind the user's %d: a DIN's are 128 (item row, pooled)" % (d_item, d_user_))
    n_out = 1 if kind == KIND_DNN3 else struct.unpack("<I", trunk[16:20])[0]
    att = (_f32(wa, what="wa").tobytes() + _f32(np.reshape(ba, -1), (att_h,), "ba").tobytes() +
           _f32(np.reshape(wa2, -1), (att_h,), "wa2").tobytes() + _f32(np.reshape(ba2, -1), (1,), "ba2").tobytes())
    return KIND_DIN, struct.pack("<6I", d_user_, 64, h1, h2, n_out, att_h) + att + trunk[16 if kind == KIND_DNN3 else 20:]


def pack_mha_arrays(wq, bq, wk, wv, bv, wo, n_head, w1, b1, w2, b2, w3, b3, d_user):
    """→ (KIND_MHA, blob): the attention's arrays in front of the trunk's, the trunk checked as a 128-wide DNN3."""
    wq, n_head = np.asarray(wq), int(n_head)
    if wq.ndim != 2 or wq.shape[0] != 64 or (wq.shape[1], n_head) not in MHA_SHAPES:
        raise ValueError("wq has shape %s with %d heads, expected [64][d_att] with (d_att, n_head) one of %s (a 64-wide item table)" %
                         (tuple(wq.shape), n_head, sorted(MHA_SHAPES)))
    d_att = wq.shape[1]
    kind, trunk = pack_dnn3_arrays(w1, b1, w2, b2, w3, b3, d_user)
    d_user_, d_item, h1, h2 = struct.unpack("<4I", trunk[:16])
    if d_item != 128:
        raise ValueError("w1 has %d rows behind the user's %d: an MHA's are 128 (item row, pooled)" % (d_item, d_user_))
    n_out = 1 if kind == KIND_DNN3 else struct.unpack("<I", trunk[16:20])[0]
    att = b"".join(a.tobytes() for a in (_f32(wq, what="wq"), _f32(np.reshape(bq, -1), (d_att,), "bq"), _f32(wk, (64, d_att), "wk"),
                                         _f32(wv, (64, d_att), "wv"), _f32(np.reshape(bv, -1), (d_att,), "bv"), _f32(wo, (d_att, 64), "wo")))
    return KIND_MHA, struct.pack("<7I", d_user_, 64, h1, h2, n_out, d_att, n_head) + att + trunk[16 if kind == KIND_DNN3 else 20:]


def pack_mmoe_arrays(we, be, wg, bg, wt, bt, wo, bo, d_user):
    """→ (KIND_MMOE, blob, description)"""
    we, wt = np.asarray(we), np.asarray(wt)
    if we.ndim != 3 or wt.ndim != 3:
        raise ValueError("we / wt must be 3-D: [E][in][h_e] and [T][h_e][h_t] (one [in][out] kernel per expert / task)")
    (n_e, din, h_e), (n_t, _, h_t) = we.shape, wt.shape
    d_user = int(d_user)
    d_item = din - d_user
    if not 1 <= d_user <= 4096 or d_item not in (64, 128):
        raise ValueError("we has %d input rows: with d_user = %d the item half is %d wide (the table's dim: 64 or 128)" % (din, d_user, d_item))
    if (n_e, h_e) not in MMOE_SHAPES or not 1 <= n_t <= 4 or h_t not in (32, 64):
        raise ValueError("%d experts x %d, %d towers x %d have no kernel (experts: %s; 1..4 tasks; tower width 32 or 64)" %
                         (n_e, h_e, n_t, h_t, sorted(MMOE_SHAPES)))
    parts = [_f32(we, what="we"), _f32(be, (n_e, h_e), "be"), _f32(wg, (n_t, din, n_e), "wg"), _f32(bg, (n_t, n_e), "bg"),
             _f32(wt, (n_t, h_e, h_t), "wt"), _f32(bt, (n_t, h_t), "bt"), _f32(np.reshape(wo, (n_t, -1)), (n_t, h_t), "wo"),
             _f32(np.reshape(bo, -1), (n_t,), "bo")]
    blob = struct.pack("<6I", d_user, d_item, n_e, h_e, n_t, h_t) + b"".join(a.tobytes() for a in parts)
    return KIND_MMOE, blob, "PG_MODEL_MMOE [%d+%d] -> %d experts x %d -> %d towers x %d, %d bytes" % (d_user, d_item, n_e, h_e, n_t, h_t, len(blob))


def pack_ple_arrays(levels, wt, bt, wo, bo, d_user):
    """levels: per extraction level a mapping we_t, we_s, be_t, be_s, wg_t, bg_t (and wg_s, bg_s below the last) → (KIND_PLE, blob, description)"""
    wt, we_t, we_s = np.asarray(wt), np.asarray(levels[0]["we_t"]), np.asarray(levels[0]["we_s"])
    if wt.ndim != 3 or we_t.ndim != 4 or we_s.ndim != 3:
        raise ValueError("we1_t / we1_s / wt must be [T][E_t][in][h_e], [E_s][in][h_e] and [T][h_e][h_t]")
    (n_t, e_t, din, h_e), e_s, h_t, n_l, d_user = we_t.shape, we_s.shape[0], wt.shape[2], len(levels), int(d_user)
    d_item = din - d_user
    if not 1 <= d_user <= 4096 or d_item not in (64, 128):
        raise ValueError("we1_t has %d input rows: with d_user = %d the item half is %d wide (the table's dim: 64 or 128)" % (din, d_user, d_item))
    if (not 1 <= n_t <= 3 or e_t not in (1, 2) or e_s not in (1, 2) or n_l not in (1, 2) or h_e not in ((64, 128) if n_l == 1 else (64,)) or
            h_t not in (32, 64) or (n_t * e_t + e_s) * h_e > 512):
        raise ValueError("%d levels of %d x %d task and %d shared experts x %d, towers x %d have no kernel (1..3 tasks; 1 or 2 experts per group; "
                         "width 64, or 128 with one level; tower width 32 or 64; all experts x width <= 512)" % (n_l, n_t, e_t, e_s, h_e, h_t))
    parts = []
    for l, lv in enumerate(levels):
        n_in, n = (h_e if l else din), "%d_" % (l + 1)
        parts += [_f32(lv["we_t"], (n_t, e_t, n_in, h_e), "we" + n + "t"), _f32(lv["we_s"], (e_s, n_in, h_e), "we" + n + "s"),
                  _f32(lv["be_t"], (n_t, e_t, h_e), "be" + n + "t"), _f32(lv["be_s"], (e_s, h_e), "be" + n + "s"),
                  _f32(lv["wg_t"], (n_t, n_in, e_t + e_s), "wg" + n + "t"), _f32(lv["bg_t"], (n_t, e_t + e_s), "bg" + n + "t")]
        if l + 1 < n_l:
            parts += [_f32(lv["wg_s"], (n_in, n_t * e_t + e_s), "wg" + n + "s"), _f32(np.reshape(lv["bg_s"], -1), (n_t * e_t + e_s,), "bg" + n + "s")]
    parts += [_f32(wt, (n_t, h_e, h_t), "wt"), _f32(bt, (n_t, h_t), "bt"), _f32(np.reshape(wo, (n_t, -1)), (n_t, h_t), "wo"), _f32(np.reshape(bo, -1), (n_t,), "bo")]
    blob = struct.pack("<8I", d_user, d_item, n_t, e_t, e_s, h_e, n_l, h_t) + b"".join(a.tobytes() for a in parts)
    return KIND_PLE, blob, "PG_MODEL_PLE [%d+%d] -> %d levels of %d x %d + %d experts x %d -> %d towers x %d, %d bytes" % (
        d_user, d_item, n_l, n_t, e_t, e_s, h_e, n_t, h_t, len(blob))


def pack_dcn_arrays(wc, bc, w1, b1, w2, b2, w3, b3, d_user):
    """→ (KIND_DCN, blob, description)"""
    wc, w1, w2 = np.asarray(wc), np.asarray(w1), np.asarray(w2)
    if wc.ndim != 3 or wc.shape[1] != wc.shape[2] or w1.ndim != 2 or w2.ndim != 2:
        raise ValueError("wc must be [L][D][D] (one square [in][out] kernel per cross layer), w1 and w2 2-D")
    (n_l, d, _), h1, h2 = wc.shape, w1.shape[1], w2.shape[1]
    d_user = int(d_user)
    d_item = d - d_user
    if d_user < 1 or d_item not in (64, 128) or d > 256:
        raise ValueError("wc is %d wide: with d_user = %d the item half is %d wide (the table's dim: 64 or 128; at most 256 in all)" % (d, d_user, d_item))
    w3 = np.reshape(w3, (h2, -1))
    n_out = w3.shape[1]
    if not 1 <= n_l <= 3 or (h1, h2) not in DCN_HEADS or not 1 <= n_out <= 4:
        raise ValueError("%d cross layers, head %d-%d, %d outputs have no kernel (1..3 layers; heads: %s; 1..4 outputs)" %
                         (n_l, h1, h2, n_out, sorted(DCN_HEADS)))
    parts = [_f32(wc, what="wc"), _f32(bc, (n_l, d), "bc"), _f32(w1, (d, h1), "w1"), _f32(b1, (h1,), "b1"), _f32(w2, (h1, h2), "w2"),
             _f32(b2, (h2,), "b2"), _f32(w3, what="w3"), _f32(np.reshape(b3, -1), (n_out,), "b3")]
    blob = struct.pack("<6I", d_user, d_item, n_l, h1, h2, n_out) + b"".join(a.tobytes() for a in parts)
    return KIND_DCN, blob, "PG_MODEL_DCN [%d+%d], %d cross layers -> %d -> %d -> %d, %d bytes" % (d_user, d_item, n_l, h1, h2, n_out, len(blob))


def pack_gbdt_trees(trees, n_user, n_item, base, objective, le=False):
    """trees: per tree a mapping feature, threshold, left, right, missing_left, value → (KIND_GBDT, blob, description); every tree
    completed to the forest's depth — an early leaf copied beneath itself, over nodes (feature 0, threshold +inf)"""
    def levels(t):
        left, right = np.asarray(trees[t]["left"], dtype=np.int64), np.asarray(trees[t]["right"], dtype=np.int64)
        cur, out = np.zeros(1, dtype=np.int64), []
        while True:
            out.append(cur)
            inner = left[cur] >= 0
            if not inner.any():
                return out
            if len(out) > 8:
                raise ValueError("tree %d is deeper than 8" % t)
            cur = np.stack([np.where(inner, left[cur], cur), np.where(inner, right[cur], cur)], axis=1).reshape(-1)
    if not (0 <= n_user <= 64 and 0 <= n_item <= 64 and n_user + n_item >= 1 and 1 <= len(trees) <= 4096 and objective in (0, 1)):
        raise ValueError("%d + %d features, %d trees, objective %d have no kernel (0..64 + 0..64 features, 1..4096 trees, objective 0 or 1)" %
                         (n_user, n_item, len(trees), objective))
    depth = max([1] + [len(levels(t)) - 1 for t in range(len(trees))])
    parts = [struct.pack("<5If", n_user, n_item, len(trees), depth, objective, base)]
    for t, tr in enumerate(trees):
        feat, miss, left = (np.asarray(tr[k], dtype=np.int64) for k in ("feature", "missing_left", "left"))
        thr = np.asarray(tr["threshold"], dtype=np.float32)
        if le:
            thr = np.nextafter(thr, np.float32(np.inf))
        lv = levels(t)
        while len(lv) <= depth:
            lv.append(np.repeat(lv[-1], 2))
        cur = np.concatenate(lv[:depth])
        inner = left[cur] >= 0
        if np.any(inner & ((feat[cur] < 0) | (feat[cur] >= n_user + n_item))):
            raise ValueError("tree %d splits on a feature outside 0..%d" % (t, n_user + n_item - 1))
        if np.any(np.isnan(thr[cur][inner])):
            raise ValueError("tree %d has a NaN threshold" % t)
        parts += [np.where(inner, feat[cur] | ((miss[cur] != 0).astype(np.int64) << 31), 0).astype(np.uint32).tobytes(),
                  np.where(inner, thr[cur], np.float32(np.inf)).astype(np.float32).tobytes(), _f32(np.asarray(tr["value"])[lv[depth]], what="value").tobytes()]
    blob = b"".join(parts)
    return KIND_GBDT, blob, "PG_MODEL_GBDT [%d+%d] features, %d trees of depth %d, objective %d, %d bytes" % (n_user, n_item, len(trees), depth, objective, len(blob))


def pack_mind_arrays(s, b0, wc, wu, b1, w2, b2, n_iter, normalize):
    """→ (KIND_MIND, blob, description); every matrix [in][out]"""
    b0, wc, wu, w2 = np.asarray(b0), np.asarray(wc), np.asarray(wu), np.asarray(w2)
    if b0.ndim != 2 or wc.ndim != 2 or wu.ndim != 2 or w2.ndim != 2:
        raise ValueError("routing_init, wc, wu and w2 are matrices")
    K, h1, d_user, d_out = b0.shape[0], wc.shape[1], wu.shape[0], w2.shape[1]
    if not (1 <= K <= 8 and h1 in (128, 256) and 1 <= d_user <= 1024 and d_out in (64, 128) and 1 <= n_iter <= 4 and normalize in (0, 1)):
        raise ValueError("%d interests, h1 %d, d_user %d, d_out %d, %d iterations, normalize %d have no kernel (1..8 interests; h1 128 or 256; "
                         "d_user 1..1024; d_out 64 or 128; 1..4 iterations; normalize 0 or 1)" % (K, h1, d_user, d_out, n_iter, normalize))
    parts = [_f32(s, (64, 64), "s"), _f32(b0, (K, 256), "routing_init"), _f32(wc, (64, h1), "wc"), _f32(wu, (d_user, h1), "wu"),
             _f32(np.asarray(b1).reshape(-1), (h1,), "b1"), _f32(w2, (h1, d_out), "w2"), _f32(np.asarray(b2).reshape(-1), (d_out,), "b2")]
    blob = struct.pack("<6I", d_user, d_out, K, n_iter, h1, normalize) + b"".join(p.tobytes() for p in parts)
    return KIND_MIND, blob, "PG_MODEL_MIND d_user %d, %d interests of %d, %d iterations, h1 %d, normalize %d, %d bytes" % (
        d_user, K, d_out, n_iter, h1, normalize, len(blob))


def pack_npz(path_or_mapping, d_user=None, rename=None, n_head=None):
    """Load the arrays (an .npz path or a mapping name → array) and pack them; → (kind, blob, description)."""
    z = np.load(path_or_mapping) if isinstance(path_or_mapping, (str, bytes)) else path_or_mapping
    rename = rename or {}

    def get(name):
        key = rename.get(name, name)
        if key not in z:
            raise KeyError("array \"%s\" not in the file (have: %s)" % (key, ", ".join(sorted(z.keys()))))
        return z[key]
    if rename.get("tree_ptr", "tree_ptr") in z:
        ptr = np.asarray(get("tree_ptr"), dtype=np.int64)
        names = ("feature", "threshold", "left", "right", "missing_left", "value")
        trees = [{k: np.asarray(get(k))[ptr[t]:ptr[t + 1]] for k in names} for t in range(len(ptr) - 1)]
        scalar = lambda n: np.asarray(get(n)).reshape(-1)[0]   # noqa: E731
        return pack_gbdt_trees(trees, int(scalar("n_user_feat")), int(scalar("n_item_feat")), float(scalar("base")), int(scalar("objective")),
                               bool(scalar("le")) if rename.get("le", "le") in z else False)
    if rename.get("routing_init", "routing_init") in z:
        scalar = lambda n: int(np.asarray(get(n)).reshape(-1)[0])   # noqa: E731
        return pack_mind_arrays(*[get(n) for n in ("s", "routing_init", "wc", "wu", "b1", "w2", "b2")], scalar("n_iter"), scalar("normalize"))
    if d_user is None:
        d_user = int(np.asarray(get("d_user")).reshape(-1)[0])
    if rename.get("we1_t", "we1_t") in z:
        n_l = 2 if rename.get("we2_t", "we2_t") in z else 1
        levels = [{k: get("%s%d_%s" % (k[:2], l + 1, k[3])) for k in ("we_t", "we_s", "be_t", "be_s", "wg_t", "bg_t") + (("wg_s", "bg_s") if l + 1 < n_l else ())}
                  for l in range(n_l)]
        return pack_ple_arrays(levels, *[get(n) for n in ("wt", "bt", "wo", "bo")], d_user)
    if rename.get("we", "we") in z:
        return pack_mmoe_arrays(*[get(n) for n in ("we", "be", "wg", "bg", "wt", "bt", "wo", "bo")], d_user)
    trunk = [get(n) for n in ("w1", "b1", "w2", "b2", "w3", "b3")]
    if rename.get("wc", "wc") in z:
        return pack_dcn_arrays(get("wc"), get("bc"), *trunk, d_user)
    if rename.get("wq", "wq") in z:
        if n_head is None:
            n_head = int(np.asarray(get("n_head")).reshape(-1)[0])
        kind, blob = pack_mha_arrays(*[get(n) for n in ("wq", "bq", "wk", "wv", "bv", "wo")], n_head, *trunk, d_user)
    elif rename.get("wa", "wa") in z:
        kind, blob = pack_din_arrays(get("wa"), get("ba"), get("wa2"), get("ba2"), *trunk, d_user)
    else:
        kind, blob = pack_dnn3_arrays(*trunk, d_user)
    w1, w2 = get("w1"), get("w2")
    n_out = int(np.asarray(get("b3")).size)
    desc = "%s [%d+%d]-%d-%d-%d, %d bytes" % ({KIND_DNN3: "PG_MODEL_DNN3", KIND_DNN3_MULTI: "PG_MODEL_DNN3_MULTI", KIND_DIN: "PG_MODEL_DIN", KIND_MHA: "PG_MODEL_MHA"}[kind],
                                              d_user, w1.shape[0] - d_user, w1.shape[1], w2.shape[1], n_out, len(blob))
    return kind, blob, desc


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("npz")
    ap.add_argument("--d-user", type=int, default=None)
    ap.add_argument("--n-head", type=int, default=None, help="PG_MODEL_MHA: the number of heads (or an integer array n_head in the file)")
    ap.add_argument("--map", default="", help="w1=dense/kernel,b1=dense/bias,…")
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    rename = dict(kv.split("=", 1) for kv in a.map.split(",") if kv)
    try:
        kind, blob, desc = pack_npz(a.npz, a.d_user, rename, a.n_head)
    except (KeyError, ValueError) as e:
        sys.stderr.write("pack_model: %s\n" % e)
        return 2
    with open(a.out, "wb") as f:
        f.write(blob)
    print("%s -> %s (pg_model_kind %d)" % (desc, a.out, kind))
    return 0


if __name__ == "__main__":
    sys.exit(main())
