"""The grid of Bloom filter cases shared by tests/test_bloom_cpu.py (the library's host statements) and tests/test_gpu_bloom.py (the
kernels), each against tests/bloom_ref.py.  A case is: empty slots → Add of one set of lists → the slots' bytes → Exists and the
filter over a second set of lists.  Sizes sit on the kernels' edges: key lengths on murmur3's block and tail paths, m on the word
and the 256-byte stride edge, cap on a wave, a probe workgroup of 256 and a compaction chunk of 1 024, nq 1 / 3 / 256."""
import numpy as np

import bloom_ref as ref

U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
HUGE = np.uint64((1 << 40) + 5)                 # a row far outside every key store here
KEY_LENS = (0, 1, 3, 4, 5, 8, 63, 64)
EXPLICIT_SEEDS = [0, 0xFFFFFFFF, 2, 0x9747B28C, 1, 0x80000000, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41]
N_SLOTS = 5                                     # slots 1 and 3 are written, 0, 2 and 4 are their neighbours
MAXP = 8                                        # PG_TRIM_MAX_PLANES


def key_store(rng, n):
    """n keys: every length of KEY_LENS in turn first, then random lengths 0 .. 64, random bytes"""
    keys = []
    for i in range(n):
        L = KEY_LENS[i % len(KEY_LENS)] if i < 8 * len(KEY_LENS) else int(rng.integers(0, ref.MAX_KEY + 1))
        keys.append(rng.integers(0, 256, L).astype(np.uint8).tobytes())
    return keys


def slots_of(nq, n_slots):
    """a slot per request: written ones (slot 1 named by several requests), no slot, a slot >= n_slots"""
    pat = [1, ref.NO_SLOT, 3, n_slots + 2, 1, n_slots]
    return np.array([pat[q % len(pat)] for q in range(nq)], dtype=np.uint32)


def lists_of(rng, nq, cap, key_rows, carry, with_count):
    """(rows, score, source, count, planes_f64, source_mask, planes_f32): rows inside and outside the key store, padding rows in
    the middle of a list; carry: "none" | "some" | "all" optional arrays"""
    rows = rng.integers(0, key_rows + 40, (nq, cap)).astype(np.uint64)
    rows[rng.random((nq, cap)) < 0.03] = HUGE
    rows[rng.random((nq, cap)) < 0.06] = U64MAX
    count = None
    if with_count:
        count = rng.integers(0, cap + 3, nq).astype(np.uint32)
        count[0] = max(1, cap - cap // 7)
        if nq > 1:
            count[1] = cap + 5
        if nq > 2:
            count[2] = 0
    score = np.round(rng.standard_normal((nq, cap)), 4)
    score.view(np.uint64)[0, cap // 2] = 0x7FF8000000000123              # a NaN with a payload travels as bits
    if carry == "none":
        return (rows, score, None, count, None, None, None)
    n = MAXP if carry == "all" else 2
    return (rows, score, rng.integers(0, 8, (nq, cap)).astype(np.uint8), count, rng.standard_normal((n, nq, cap)),
            rng.integers(0, 256, (nq, cap)).astype(np.uint32), rng.standard_normal((n, nq, cap)).astype(np.float32))


class Case:
    def __init__(self, name, m, k, nq, cap, carry="some", with_count=True, seeds=None, n_slots=N_SLOTS, key_rows=300):
        self.name, self.m, self.k, self.nq, self.cap, self.n_slots, self.key_rows = name, m, k, nq, cap, n_slots, key_rows
        self.carry, self.with_count = carry, with_count
        self.seeds = None if seeds is None else list(seeds[:k])

    def build(self):
        rng = np.random.default_rng((self.m * 1000003 + self.k * 101 + self.nq * 7 + self.cap) % (1 << 32))
        self.keys = key_store(rng, self.key_rows)
        self.locs = ref.locations(self.keys, self.m, self.k, self.seeds)
        self.slots = slots_of(self.nq, self.n_slots)
        # what is added: about a third of the store per request, with padding and outside rows among them
        self.add_lists = lists_of(rng, self.nq, self.cap, self.key_rows, "none", self.with_count)
        self.add_lists[0][:] = np.where(self.add_lists[0] < np.uint64(self.key_rows), self.add_lists[0] // np.uint64(3) * np.uint64(3), self.add_lists[0])
        self.lists = lists_of(rng, self.nq, self.cap, self.key_rows, self.carry, self.with_count)
        return self

    def expected(self):
        """→ (bitsets [n_slots][nbytes] after the add, exists [nq][cap], the filter's outputs)"""
        bs = ref.new_bitsets(self.m, self.n_slots)
        ref.add(self.locs, self.n_slots, bs, self.add_lists[0], self.slots, self.add_lists[3])
        ex = ref.exists(self.locs, self.n_slots, bs, self.lists[0], self.slots, self.lists[3])
        flt = ref.bloom_filter(self.locs, self.n_slots, bs, self.slots, *self.lists)
        return bs, ex, flt


def grid():
    g = []
    # m on its edges (every location 0; the word edge; the stride edge; the reference test's size), k and the seeds along
    for m, k, seeds in ((1, 1, None), (31, 4, None), (32, 4, EXPLICIT_SEEDS), (33, 7, None), (2048, 4, None), (2049, 16, EXPLICIT_SEEDS),
                        (18706, 4, None), (18706, 16, None), (6235225, 7, EXPLICIT_SEEDS)):
        g.append(Case("m%d_k%d%s" % (m, k, "_seeds" if seeds else ""), m, k, 3, 257, carry="some", with_count=(m % 2 == 0), seeds=seeds))
    # cap on a wave, a probe workgroup, a compaction chunk, the largest; carried arrays present and absent; d_count absent
    for cap, carry, with_count in ((1, "all", True), (63, "none", True), (64, "some", False), (65, "all", True), (255, "none", False),
                                   (256, "some", True), (1025, "all", True), (16384, "some", True)):
        g.append(Case("cap%d_%s" % (cap, carry), 18706, 4, 2, cap, carry=carry, with_count=with_count))
    for nq in (1, 256):
        g.append(Case("nq%d" % nq, 2049, 7, nq, 65, carry="all", with_count=True))
    return g


GRID = grid()
IDS = [c.name for c in GRID]
