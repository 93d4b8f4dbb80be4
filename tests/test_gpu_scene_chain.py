"""GPU tests of a scene's device stages chained on ONE stream without host synchronisation (include/pairec_gpu.h: every `_dev`
stage is "enqueued on the context's stream, no synchronisation", its outputs plug into the next stage "as they are"), against the
composed reference of tests/scene_chain_ref.py, by bits, after EVERY stage:

  pg_fanin_merge_dev → pg_item_state_filter_dev → pg_candidates_trim_dev → pg_candidates_blend_dev → pg_candidates_dimcap_dev →
  pg_candidates_classcut_dev → pg_candidates_trim2_dev → pg_boost_scores_dev (in place) → pg_sort_scores_dev → pg_distinct_ids_dev →
  pg_mix_sort_dev → pg_ssd_sort_dev, and pg_diversity_rules_features_dev from trim2's lists.

Every stage writes into device buffers of its own, pre-filled with 0xA5 and followed by a guard region; every input a predecessor
does not produce (segment offsets, enable bytes, seeds, user slots, a carried fp32 plane) is uploaded before the first stage is
enqueued; nothing is downloaded and synchronize() is not called until the last stage of the last batch is enqueued.  Then every
output array of every stage is compared with the reference, padding included — so "every output element is written exactly once"
holds for the padding too — and a failure names batch, stage, array, request and slot.

What each case makes collide (slots: csrc/common.hpp pg::ScratchSlot):
  a  behind a stall     every host-side enqueue precedes the device's first kernel: whatever a stage's host code does too early.
                        Thirteen stages reuse kSlotWork (the sorts inside trim / blend / classcut / trim2, the score sort, SSD's
                        grid) and each its own slot, back to back.
  b  sync per stage     the same chain with the hazards removed: (a) failing where (b) passes is a bug of ordering.
  c  small, large, small on a fresh context, one stall: the large batch makes scratch_reserve free and reallocate kSlotWork (SSD's
                        9.1 MiB of prepared embeddings; the first small batch's SSD has 139 KiB of it and has not run) and makes
                        kSlotDimcap; every other slot stays inside its first granule at these shapes and is overwritten
                        (tests/scene_chain_cases.py lists the sizes).
  d  interleaved        A.stage1, B.stage1, A.stage2, …: stage N's slot (kSlotTrim, kSlotBlend, kSlotDimcap, kSlotClasscut,
                        kSlotTrim2, kSlotMix, kSlotSsdStage, kSlotDiversity, kSlotDiversityPlanes, kSlotFanin, kSlotWork) is
                        overwritten by batch B before A's stage N + 1 runs.
  e  tickets            a recommend ticket in front of and behind the chain: kSlotWork, kSlotStatus, kSlotPipe and the recall's
                        slots serve the pipeline between the chain's stages' uses.
  f  shared sets        one filter Cond, one boost Cond, one DistinctId Cond, one Classcut and one Mix used first — their table
                        uploads — by two threads on two contexts of device 0 at once, three chains each without waiting."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import pairec_amd as pa
import scene_chain_cases as cases
import scene_chain_ref as ref
from oracle import oracle as o
from pairec_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64
STALL_MS = 20
N_SRC = 3


class Sets:
    """the compiled sets of one scene"""

    def __init__(self, w, cfg):
        self.filt = pa.Cond(cfg.filter, cases.DECL)
        self.boost = pa.Cond(cfg.boost, cases.DECL, boost=True)
        self.distinct = pa.Cond(cfg.distinct, cases.DECL)
        self.cc = pa.Classcut([(e, t, c) for e, (t, c) in zip(w.class_exprs, cfg.class_rules)], cases.DECL, cases.RECALLS)
        self.mix = pa.Mix(cfg.mix, cases.DECL, size=cfg.mix_size, remain_item=cfg.mix_remain, recall_names=cases.RECALLS)

    def free(self):
        for s in (self.filt, self.boost, self.distinct, self.cc, self.mix):
            s.free()


class World:
    pass


@pytest.fixture(scope="module")
def world(ctx):
    """the table, the store, the three shapes' batches with their references (computed once, never changed) and compiled sets"""
    w = World()
    w.host = cases.world()
    w.table = pa.Table(ctx, cases.TABLE_ROWS, cases.TABLE_DIM)
    w.table.fill_synthetic(cases.TABLE_SEED)
    w.fs = pa.Features(ctx, cases.STORE_ROWS)
    for name, dt in cases.DECL:
        w.fs.set_column(name, dt, w.host.store[name], default=float(w.host.defaults.get(name, 0)))
    ctx.synchronize()
    w.batch, w.want, w.sets = {}, {}, {}
    for shape in cases.SHAPES:
        w.batch[shape] = cases.batch(shape, cases.BATCH_SEEDS[shape])
        w.want[shape] = ref.run(w.host, w.batch[shape])
        w.sets[shape] = Sets(w.host, w.batch[shape].cfg)
    yield w
    for s in w.sets.values():
        s.free()
    w.fs.destroy()
    w.table.destroy()


class DevChain:
    """one batch's device buffers and its stages as a list of enqueue calls.  The constructor allocates and uploads everything
    (every upload synchronises the stream: it belongs in front of a stall); stages() enqueues nothing until its entries are called"""

    def __init__(self, ctx, w, shape, sets=None, label=None):
        self.ctx, self.w, self.shape, self.label = ctx, w, shape, label or shape
        self.b, self.want, self.sets = w.batch[shape], w.want[shape], sets or w.sets[shape]
        self.bufs, self.out = [], {}
        b = self.b
        # the outputs are sized by the reference's widths: they must be the library's own, or a stage would write past a buffer
        width = {st: self.want[st]["rows"].shape[1] for st in ref.LIST_STAGES}
        assert width["fanin"] == width["filter"] == b.cap and width["dimcap"] == width["blend"]
        assert (pa.trim_out_cap(b.cfg.trim, width["filter"]), pa.blend_out_cap(b.cfg.blend, width["trim"]), self.sets.cc.out_cap(width["dimcap"]),
                pa.trim2_out_cap(b.cfg.trim2, width["classcut"])) == (width["trim"], width["blend"], width["classcut"], width["trim2"])
        self.src = [(self.put(r), self.put(s), r.shape[1], s.dtype == np.float64) for r, s in b.sources]
        self.p32 = self.put(b.p32)
        self.users = {k: tuple(self.put(a) for a in getattr(self.sets, k).pack_user(b.users)) for k in ("filt", "boost", "distinct", "mix")}
        self.seeds, self.enable = self.put(b.seeds), self.put(b.enable)
        oc = self.want["trim2"]["rows"].shape[1]
        self.seg = self.put(np.arange(b.nq + 1, dtype=np.uint32) * np.uint32(oc))
        for stage in ref.STAGES:
            for name, a in self.want[stage].items():
                if name.startswith("_") or a is None or (stage, name) == ("boost", "score"):
                    continue
                self.out[stage, name] = (self.put(np.full(a.nbytes + GUARD, 0xA5, np.uint8)), a)
        self.out["boost", "score"] = (self.out["trim2", "score"][0], self.want["boost"]["score"])      # the one in-place form

    def put(self, a):
        self.bufs.append(self.ctx.to_device(a))
        return self.bufs[-1]

    def free(self):
        for p in self.bufs:
            self.ctx.free(p)
        self.bufs = []

    def d(self, stage, name):
        return self.out[stage, name][0]

    def list_in(self, stage):
        """the nine list inputs of a stage that follows list stage `stage`, in the ABI's order"""
        p32, n32 = (self.p32, 1) if stage == "fanin" else (self.d(stage, "planes_f32"), 1)
        return (self.d(stage, "rows"), self.d(stage, "score"), self.d(stage, "source"), self.d(stage, "count"), self.d(stage, "planes_f64"), N_SRC,
                self.d(stage, "source_mask"), p32, n32)

    def list_out(self, stage):
        return tuple(self.d(stage, n) for n in ref.LIST_ARRAYS)

    def stages(self):
        ctx, w, b, cfg, s = self.ctx, self.w, self.b, self.b.cfg, self.sets
        nq = b.nq
        cap = {st: self.want[st]["rows"].shape[1] for st in ref.LIST_STAGES}
        oc = cap["trim2"]
        t2 = lambda n: self.d("trim2", n)                                                 # noqa: E731
        ssd = {k: v for k, v in cfg.ssd.items() if k not in ("gamma", "topn", "window")}

        def sort():
            _lib.check(ctx.L.pg_sort_scores_dev(ctx.h, t2("score"), self.seg, nq, nq * oc, oc, 1, self.d("sort", "order")))
        return [
            ("fanin", lambda: ctx.fanin_merge_dev(self.src, nq, *[self.d("fanin", n) for n in ("rows", "score", "source", "planes_f64", "source_mask", "count")])),
            ("filter", lambda: ctx.item_state_filter_dev(s.filt, w.fs, nq, cap["fanin"], *self.list_in("fanin"), *self.users["filt"], *self.list_out("filter"))),
            ("trim", lambda: ctx.candidates_trim_dev(cfg.trim, nq, cap["filter"], *self.list_in("filter"), *self.list_out("trim"))),
            ("blend", lambda: ctx.candidates_blend_dev(cfg.blend, nq, cap["trim"], *self.list_in("trim"), *self.list_out("blend"))),
            ("dimcap", lambda: ctx.candidates_dimcap_dev(cfg.dimcap, w.fs, nq, cap["blend"], *self.list_in("blend"), *self.list_out("dimcap"))),
            ("classcut", lambda: ctx.candidates_classcut_dev(s.cc, w.fs, nq, cap["dimcap"], *self.list_in("dimcap"), *self.list_out("classcut"))),
            ("trim2", lambda: ctx.candidates_trim2_dev(cfg.trim2, nq, cap["classcut"], *self.list_in("classcut"), *self.list_out("trim2"))),
            ("boost", lambda: ctx.boost_scores_dev(s.boost, w.fs, False, nq, oc, t2("rows"), t2("score"), t2("count"), *self.users["boost"], t2("score"),
                                                   self.d("boost", "rule"))),
            ("sort", sort),
            ("distinct", lambda: ctx.distinct_ids_dev(s.distinct, w.fs, cfg.distinct_ids, nq, oc, t2("rows"), t2("count"), *self.users["distinct"],
                                                      self.d("distinct", "ids"))),
            ("mix", lambda: ctx.mix_sort_dev(s.mix, w.fs, cfg.ctx_size, nq, oc, t2("rows"), t2("source"), self.d("sort", "order"), t2("count"), self.seeds,
                                             *self.users["mix"], self.d("mix", "order"), self.d("mix", "count"))),
            ("ssd", lambda: ctx.ssd_sort_dev(w.table, nq, oc, self.d("mix", "order"), t2("rows"), t2("score"), t2("source"), self.d("mix", "count"),
                                             self.enable, cfg.ssd["gamma"], cfg.ssd["topn"], cfg.ssd["window"], self.d("ssd", "pos"), self.d("ssd", "count"),
                                             self.d("ssd", "rows"), self.d("ssd", "quality"), **ssd)),
            ("diversity", lambda: ctx.diversity_rules_features_dev(cfg.div, w.fs, cases.DIV_COLS, nq, oc, t2("rows"), t2("count"), t2("source"),
                                                                   self.enable, self.d("diversity", "order"))),
        ]

    def enqueue(self, sync_each=False):
        for _, call in self.stages():
            call()
            if sync_each:
                self.ctx.synchronize()

    def fetch(self):
        """every output of every stage → a result in the reference's form (the stream is synchronised by now); a write into a
        guard region fails here"""
        got = {st: {} for st in ref.STAGES}
        for (stage, name), (p, a) in self.out.items():
            raw = np.empty(a.nbytes + GUARD, np.uint8)
            self.ctx.d2h(raw, p)
            assert np.all(raw[a.nbytes:] == 0xA5), "batch %s: stage %s wrote behind its output %s" % (self.label, stage, name)
            got[stage][name] = raw[:a.nbytes].view(a.dtype).reshape(a.shape)
        del got["trim2"]["score"]
        return got

    def check(self, note=""):
        diff = ref.first_difference(self.fetch(), self.want, absent=ref.IN_PLACE)
        assert diff is None, ref.describe(diff, self.label) + note


def run_chains(ctx, chains, order=None, stall=True):
    """enqueue the chains' stages in `order` (default: chain after chain) behind one stall, synchronise once, check them all"""
    calls = order if order is not None else [c for ch in chains for _, c in ch.stages()]
    if stall:
        ctx.debug_stall(STALL_MS)
    t0 = time.perf_counter()
    for call in calls:
        call()
    t_enqueue = time.perf_counter() - t0
    ctx.synchronize()
    return t_enqueue


# ---- b, a -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["mid", "small", "large"])
def test_synchronize_after_every_stage(ctx, world, shape):
    """case b.  It stands in front of case a so that, in file order, the module's compiled sets have had their first use — the one
    synchronous upload — and the session context's slots their growth before a chain is enqueued behind a stall: then nothing in
    case a's enqueues can wait for the device"""
    ch = DevChain(ctx, world, shape)
    try:
        ch.enqueue(sync_each=True)
        ch.check(" (a synchronize() after every stage: no ordering hazard is left)")
    finally:
        ch.free()


@pytest.mark.parametrize("shape", ["mid", "small", "large"])
def test_chained_behind_a_stall(ctx, world, shape):
    """case a"""
    ch = DevChain(ctx, world, shape)
    try:
        t_enqueue = run_chains(ctx, [ch])
        print("%s: %d stages enqueued in %.1f ms behind a %d ms stall" % (shape, len(ch.stages()), 1e3 * t_enqueue, STALL_MS))
        diff = ref.first_difference(ch.fetch(), ch.want, absent=ref.IN_PLACE)
        if diff is not None:                                             # is it the order?  the same chain, a synchronize() per stage
            again = DevChain(ctx, world, shape)
            try:
                again.enqueue(sync_each=True)
                d2 = ref.first_difference(again.fetch(), again.want, absent=ref.IN_PLACE)
            finally:
                again.free()
            note = ("; with a synchronize() after every stage the chain is correct: a bug of ORDERING between enqueued stages" if d2 is None
                    else "; with a synchronize() after every stage it fails too (%s): not an ordering bug" % ref.describe(d2, shape))
            pytest.fail(ref.describe(diff, shape) + note)
    finally:
        ch.free()


# ---- c ----------------------------------------------------------------------------------------------------------------------------
def test_slots_grow_under_a_batch_in_flight(world):
    with pa.Context(0) as fresh:                                         # every slot empty: the small batch makes them, the large one grows them
        chains = [DevChain(fresh, world, shape, label="%d (%s)" % (i, shape)) for i, shape in enumerate(("small", "large", "small"))]
        try:
            run_chains(fresh, chains)
            for ch in chains:
                ch.check()
        finally:
            for ch in chains:
                ch.free()


# ---- d ----------------------------------------------------------------------------------------------------------------------------
def test_two_batches_interleaved_stage_by_stage(ctx, world):
    a, b = DevChain(ctx, world, "mid", label="A (mid)"), DevChain(ctx, world, "small", label="B (small)")
    try:
        order = [call for pair in zip(a.stages(), b.stages()) for _, call in pair]
        assert len(order) == 2 * len(ref.STAGES)
        run_chains(ctx, [a, b], order)
        a.check()
        b.check()
    finally:
        a.free()
        b.free()


# ---- e ----------------------------------------------------------------------------------------------------------------------------
class Ticket:
    """one pg_recommend_dnn3_begin call's buffers: 2 requests, k = 50, on the scene's table"""
    NQ, K = 2, 50
    OUT = (("rows", np.uint64), ("recall", np.float32), ("rank", np.float32), ("fused", np.float64), ("order", np.uint32))

    def __init__(self, ctx, queries):
        self.ctx = ctx
        self.d_q = ctx.to_device(queries)
        self.bufs = [ctx.to_device(np.full(self.NQ * self.K * np.dtype(dt).itemsize, 0xA5, np.uint8)) for _, dt in self.OUT]
        self.bufs.append(ctx.to_device(np.full(16, 0xA5, np.uint8)))
        self.tk = C.c_void_p()

    def begin(self, world, model, expr):
        _lib.check(self.ctx.L.pg_recommend_dnn3_begin(self.ctx.h, world.table.h, model.h, expr.h, b"gpu_dnn", self.d_q, self.NQ, self.K, *self.bufs,
                                                      C.byref(self.tk)))

    def end(self):
        _lib.check(self.ctx.L.pg_recommend_end(self.ctx.h, self.tk, None))

    def fetch(self):
        out = []
        for (_, dt), p in zip(self.OUT + (("count", np.uint32),), self.bufs):
            a = np.empty(self.NQ if len(out) == len(self.OUT) else (self.NQ, self.K), dt)
            self.ctx.d2h(a, p)
            out.append(a.view(np.uint8).copy())
        return out

    def free(self):
        for p in [self.d_q] + self.bufs:
            self.ctx.free(p)


def test_a_recommend_ticket_on_either_side(ctx, world):
    wts = o.Dnn3Weights()
    model = pa.RankModel(ctx, pa.MODEL_DNN3, pa.PREC_BF16X3, pa.pack_dnn3(wts.w1, wts.b1, wts.w2, wts.b2, wts.w3, wts.b3, cases.TABLE_DIM))
    expr = pa.Expr("${gpu_dnn}")
    q = o.synth_rows(o.SEED_QUERY, 0, 2 * Ticket.NQ, cases.TABLE_DIM)
    alone = [Ticket(ctx, q[:Ticket.NQ]), Ticket(ctx, q[Ticket.NQ:])]
    mixed = [Ticket(ctx, q[:Ticket.NQ]), Ticket(ctx, q[Ticket.NQ:])]
    ch = DevChain(ctx, world, "mid")
    try:
        for t in alone:                                                  # the same two calls made alone
            t.begin(world, model, expr)
            t.end()
        want = [t.fetch() for t in alone]
        assert all(int(w[5].view(np.uint32).min()) == Ticket.K for w in want)
        ctx.debug_stall(STALL_MS)
        mixed[0].begin(world, model, expr)
        ch.enqueue()
        mixed[1].begin(world, model, expr)
        mixed[0].end()
        mixed[1].end()
        ctx.synchronize()
        for i, t in enumerate(mixed):
            for (name, _), g, x in zip(Ticket.OUT + (("count", None),), t.fetch(), want[i]):
                assert np.array_equal(g, x), "ticket %d: %s differs from the same call made alone" % (i, name)
        ch.check(" (a recommend ticket was enqueued in front of and behind the chain)")
    finally:
        ch.free()
        for t in alone + mixed:
            t.free()
        expr.free()
        model.destroy()


# ---- f ----------------------------------------------------------------------------------------------------------------------------
def test_shared_sets_two_contexts_two_threads(world):
    """one process, two threads, a context of device 0 each; the sets are new, so their first use — the table uploads — happens in
    both threads at once"""
    sets = Sets(world.host, world.batch["mid"].cfg)
    ctxs = [pa.Context(0), pa.Context(0)]
    chains = [[DevChain(c, world, "mid", sets=sets, label="thread %d run %d (mid)" % (t, i)) for i in range(3)] for t, c in enumerate(ctxs)]
    errors = []
    gate = threading.Barrier(2)

    def work(t):
        try:
            gate.wait(timeout=30)
            run_chains(ctxs[t], chains[t])
        except BaseException as e:                                       # noqa: B902 — reported by the main thread
            errors.append((t, e))
    try:
        threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        for per_thread in chains:
            for ch in per_thread:
                ch.check()
        for per_thread in chains:
            for ch in per_thread:
                ch.free()
        chains = []
        sets.free()                                                      # (waits for the device: nothing of the six chains is in flight)
        sets = None
        for t, c in enumerate(ctxs):                                     # the contexts serve on: a chain over the module's sets
            ch = DevChain(c, world, "small", label="after the free, context %d" % t)
            try:
                run_chains(c, [ch])
                ch.check()
            finally:
                ch.free()
    finally:
        for per_thread in chains:
            for ch in per_thread:
                ch.free()
        if sets is not None:
            sets.free()
        for c in ctxs:
            c.close()
