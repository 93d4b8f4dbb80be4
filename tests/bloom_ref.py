"""User2ItemExposureBloomFilter restated in Python — no GPU, no library:

  murmur3      murmur3_x86_32 with a seed (spaolacci/murmur3 New32WithSeed), one key at a time and vectorised over keys of one length;
  locations    bloom_test.go:17-29: location j of key d = murmur3(d, seed_j) % m, the seeds the primes of bloom_test.go:14;
  bitset       a Redis string per slot: bit N is byte N >> 3, mask 0x80 >> (N & 7) (SETBIT / GETBIT, redis_bitset.go:31-108);
  exists / add / filter over the candidate-list arrays: a padding entry (row UINT64_MAX, a position at or behind count[q]) is
               never kept and never added, a row outside the key store has no key (Exists false, Add skips it), a slot >= n_slots
               — NO_SLOT among them — is a user without history.  The filter keeps the entries whose Exists is false
               (user_item_exposure_bloom_filter.go:92-98); what moves and what pads is dimcap_ref.compact's, ItemStateFilter's.

`bitsets` is anything indexed by slot that gives a uint8 array of ceil(m / 8) bytes: a 2-D array, or a dict of the slots a test
touches (a filter of forty 128 MiB slots is not held whole).

Shared by tests/test_bloom_cpu.py (the library's host statements agree with it) and tests/test_gpu_bloom.py (the kernels do)."""
import numpy as np

import dimcap_ref

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_SLOT = 0xFFFFFFFF
MAX_KEY, MAX_K = 64, 16
PRIMES = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53]
C1, C2 = 0xCC9E2D51, 0x1B873593
M32 = 0xFFFFFFFF


def murmur3(data: bytes, seed: int = 0) -> int:
    h = seed & M32
    n = len(data)
    for i in range(0, n - n % 4, 4):
        k = int.from_bytes(data[i:i + 4], "little")
        k = (k * C1) & M32
        k = ((k << 15) | (k >> 17)) & M32
        k = (k * C2) & M32
        h ^= k
        h = ((h << 13) | (h >> 19)) & M32
        h = (h * 5 + 0xE6546B64) & M32
    if n % 4:
        k = int.from_bytes(data[n - n % 4:], "little")
        k = (k * C1) & M32
        k = ((k << 15) | (k >> 17)) & M32
        k = (k * C2) & M32
        h ^= k
    h ^= n
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def _rotl(x, r):
    return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & np.uint64(M32)


def murmur3_same_length(keys: np.ndarray, seed: int) -> np.ndarray:
    """keys uint8 [n][L] → uint32 [n] (64-bit arithmetic masked to 32 bits)"""
    n, L = keys.shape
    u = np.uint64
    h = np.full(n, seed & M32, dtype=u)
    words = np.zeros((n, (L + 3) // 4 * 4), dtype=np.uint8)
    words[:, :L] = keys
    w = words.view("<u4").astype(u)

    def mix(k):
        k = (k * u(C1)) & u(M32)
        k = _rotl(k, 15)
        return (k * u(C2)) & u(M32)
    for i in range(L // 4):
        h ^= mix(w[:, i])
        h = _rotl(h, 13)
        h = (h * u(5) + u(0xE6546B64)) & u(M32)
    if L % 4:
        h ^= mix(w[:, L // 4])
    h ^= u(L)
    h ^= h >> u(16)
    h = (h * u(0x85EBCA6B)) & u(M32)
    h ^= h >> u(13)
    h = (h * u(0xC2B2AE35)) & u(M32)
    return (h ^ (h >> u(16))).astype(np.uint32)


def seeds_of(k, seeds=None):
    return list(PRIMES[:k]) if seeds is None else [int(s) & M32 for s in seeds]


def locations(keys, m, k, seeds=None) -> np.ndarray:
    """keys: a list of bytes objects → int64 [n][k]: the k bit numbers of every key"""
    out = np.zeros((len(keys), k), dtype=np.int64)
    lens = np.array([len(x) for x in keys], dtype=np.int64)
    for L in np.unique(lens):
        idx = np.flatnonzero(lens == L)
        arr = np.frombuffer(b"".join(keys[i] for i in idx), dtype=np.uint8).reshape(idx.size, int(L)) if L else np.zeros((idx.size, 0), np.uint8)
        for j, s in enumerate(seeds_of(k, seeds)):
            out[idx, j] = murmur3_same_length(arr, s).astype(np.int64) % int(m)
    return out


def nbytes(m):
    return (int(m) + 7) // 8


def new_bitsets(m, n_slots):
    return np.zeros((n_slots, nbytes(m)), dtype=np.uint8)


def set_bits(bits, locs):
    """SETBIT for every location (int64, any shape) in one slot's bytes"""
    locs = np.asarray(locs, dtype=np.int64).reshape(-1)
    np.bitwise_or.at(bits, locs >> 3, (0x80 >> (locs & 7)).astype(np.uint8))


def get_bits(bits, locs):
    """GETBIT → bool, the shape of locs"""
    locs = np.asarray(locs, dtype=np.int64)
    return (bits[locs >> 3] & (0x80 >> (locs & 7)).astype(np.uint8)) != 0


def _probe_mask(key_rows, n_slots, rows, count, slots):
    """→ (live [nq][cap], probe [nq][cap]): the real entries, and those among them with a key and a slot"""
    rows = np.asarray(rows, dtype=np.uint64)
    live = dimcap_ref.live_mask(rows, count)
    has_slot = (np.asarray(slots, dtype=np.int64) < n_slots)[:, None]
    return live, live & (rows < np.uint64(key_rows)) & has_slot


def exists(locs, n_slots, bitsets, rows, slots, count=None) -> np.ndarray:
    """locs: locations() of the whole key store → uint8 [nq][cap]"""
    rows = np.asarray(rows, dtype=np.uint64)
    live, probe = _probe_mask(locs.shape[0], n_slots, rows, count, slots)
    out = np.zeros(rows.shape, dtype=np.uint8)
    for q in range(rows.shape[0]):
        idx = np.flatnonzero(probe[q])
        if idx.size:
            out[q, idx] = get_bits(bitsets[int(slots[q])], locs[rows[q, idx].astype(np.int64)]).all(axis=1)
    return out


def add(locs, n_slots, bitsets, rows, slots, count=None) -> None:
    rows = np.asarray(rows, dtype=np.uint64)
    live, probe = _probe_mask(locs.shape[0], n_slots, rows, count, slots)
    for q in range(rows.shape[0]):
        idx = np.flatnonzero(probe[q])
        if idx.size:
            set_bits(bitsets[int(slots[q])], locs[rows[q, idx].astype(np.int64)])


def keep(locs, n_slots, bitsets, rows, slots, count=None) -> np.ndarray:
    live = dimcap_ref.live_mask(rows, count)
    return live & (exists(locs, n_slots, bitsets, rows, slots, count) == 0)


def bloom_filter(locs, n_slots, bitsets, slots, rows, score, source=None, count=None, planes_f64=None, source_mask=None, planes_f32=None):
    """→ (rows, score, source, planes_f64, source_mask, planes_f32, count) as Context.bloom_filter returns them"""
    return dimcap_ref.compact(keep(locs, n_slots, bitsets, rows, slots, count), rows, score, source, count, planes_f64, source_mask, planes_f32)


def masked_write(m, data) -> np.ndarray:
    """what a slot holds after pg_bloom_slot_write of `data`: the bytes, zeros behind them, the bits at or above m cleared"""
    out = np.zeros(nbytes(m), dtype=np.uint8)
    d = np.asarray(data, dtype=np.uint8).reshape(-1)
    out[:d.size] = d
    if m % 8:
        out[-1] &= (0xFF00 >> (m % 8)) & 0xFF
    return out


def estimate(n, p):
    """EstimateParameters, bloom.go:40-45"""
    import math
    m = math.ceil(float(n) * math.log(p) / math.log(1.0 / math.pow(2.0, math.log(2.0))))
    return int(m), int(math.log(2.0) * m / float(n) + 0.5)


def decimal_keys(ids):
    return [str(int(i)).encode() for i in ids]
