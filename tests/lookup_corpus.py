"""Hand-made indices and query batches for the lookup stage (the end of kasa_batch_sort_and_range: tile_bounds_kernel,
lookup_tile_kernel or -- debug flag 2 -- lookup_kernel, the tile_suffix kernels), with a plain reference of what the stage
leaves per sorted query.  The inputs of tests/test_lookup_corpus_cpu.py (which checks that the corpus is what it claims and
that the reference agrees with the oracle) and tests/test_gpu_lookup_corpus.py (which feeds it to the device through
kasa_batch_set_queries).  Pure numpy and kasa_amd/formats.py: no device, no reference tree.

A case is one index (formats.make_index), one batch of queries handed in shuffled order with their payload, and the level
windows (k_high, k_low) to run it under.  The payload is a permutation of the query numbers (every query its own read: a
wrong order of equal keys shows) except in the open-group family, whose payload is the read of a few long reads.

The constants restate kasa_hip.hip's: a tile of TILE sorted queries per workgroup, four consecutive queries per thread, the
tile's index span staged on chip up to LSPAN records, a prefix trie of RANGE_LETTERS letters, '^' = letter 30.

Families:
  main    every neighbour geometry at every shared length, equal keys in a row, repeated queries, '^' at every position
          relative to a match of every length; with a block of filler entries the same queries meet unstaged tiles
  span    a run of index entries inside one prefix-table bucket and a tile of queries inside that bucket: spans of
          LSPAN - 1 .. LSPAN + 2, the span's start even and odd, the last run reaching the last record
  ends    indices of 1, 2, 3 and some 300 entries; queries below, on and above the first and last key, key 0 and the largest
          key; batches of 1, 3, 4, 5, 1023, 1024, 1025 and 2049 queries
  open    groups that stay open over tiles (and over a chunk of 1024 tiles) of queries that match nothing: compared
          through the scores, whose float32 summation order follows the flush positions
"""
from __future__ import annotations

import bisect
import functools
from dataclasses import dataclass, field

import numpy as np

from kasa_amd import formats

HAT = 30
TILE, ITEMS, LSPAN, RANGE_LETTERS = 1024, 4, 1536, 6
CHUNK_TILES = 1024                                      # tiles per chunk of the tile_suffix kernels
WINDOWS = {12: [(12, 7), (12, 12), (9, 7), (7, 7), (12, 5), (12, 3)], 25: [(25, 7), (25, 18), (25, 25), (12, 7)]}
BATCH_SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 2049]
SPAN_EDGE = [LSPAN - 1, LSPAN, LSPAN + 1, LSPAN + 2]
N_TAXA = 46                                             # content entries of the hand-made indices (0 = non_unique)
M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------
# keys: Python integers <-> the arrays the library takes
# ------------------------------------------------------------------------------------------------
def pack(letters) -> int:
    v = 0
    for x in letters:
        v = (v << 5) | int(x)
    return v


def sub(base, *pairs):
    """`base` with letter j (counted from 1) set to v for every (j, v)"""
    out = list(base)
    for j, v in pairs:
        out[j - 1] = v
    return out


def is_wide(keys: np.ndarray) -> bool:
    return keys.dtype == formats.KEY128_DTYPE


def key_ints(keys: np.ndarray) -> list:
    if is_wide(keys):
        return [(h << 64) | l for l, h in zip(keys["lo"].tolist(), keys["hi"].tolist())]
    return keys.tolist()


def keys_from_ints(values, wide: bool) -> np.ndarray:
    if not wide:
        return np.array(values, dtype=np.uint64).reshape(-1)
    out = np.zeros(len(values), dtype=formats.KEY128_DTYPE)
    out["lo"] = np.array([v & M64 for v in values], dtype=np.uint64).reshape(-1)
    out["hi"] = np.array([v >> 64 for v in values], dtype=np.uint64).reshape(-1)
    return out


def shared_letters(a: int, b: int, letters: int) -> int:
    x = a ^ b
    return letters if x == 0 else (5 * letters - x.bit_length()) // 5


def first_hat(q: int, letters: int) -> int:
    """the first letter (from 1) of q that is '^', 0: none"""
    for k in range(1, letters + 1):
        if (q >> (5 * (letters - k))) & 31 == HAT:
            return k
    return 0


def stable_sort(q: np.ndarray, payload: np.ndarray):
    """what the query sort must leave: keys ascending, equal keys in the order they came in"""
    order = formats.key_order(q)                        # (np.lexsort: stable)
    return q[order], payload[order]


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
@dataclass
class Lookup:
    depth: np.ndarray        # u8: the deepest matched level, 0: none
    rep: np.ndarray          # u32: an index position that shares the matched prefix (meaningful where depth > 0)
    lo: np.ndarray           # i64: the first index entry >= q
    la: np.ndarray           # i64: letters shared with idx[lo], 0 at lo == n
    lb: np.ndarray           # i64: letters shared with idx[lo - 1], 0 at lo == 0

    @property
    def L(self):
        return np.maximum(self.la, self.lb)


def lookup_reference(idx_kmers: np.ndarray, sorted_queries: np.ndarray, k_high: int, k_low: int, letters: int) -> Lookup:
    """From the definition, query by query: lo = the first index entry >= q; la, lb = the letters q shares with idx[lo] and with
    idx[lo - 1] (0 where there is none); L = max(la, lb) and the representative is lo, or lo - 1 where lb is larger; no match
    below the trie's 6 letters; the depth is L capped at k_high, cut to k - 1 by the first '^' at a letter k of k_low .. depth,
    and 0 when that leaves less than k_low."""
    n = int(idx_kmers.shape[0])
    if is_wide(idx_kmers):
        idx, qs = key_ints(idx_kmers), key_ints(sorted_queries)
        los = [bisect.bisect_left(idx, q) for q in qs]
    else:
        idx, qs = idx_kmers.tolist(), sorted_queries.tolist()
        los = np.searchsorted(idx_kmers, sorted_queries, side="left").tolist()
    nq = len(qs)
    depth, rep = np.zeros(nq, dtype=np.uint8), np.zeros(nq, dtype=np.uint32)
    la_, lb_ = np.zeros(nq, dtype=np.int64), np.zeros(nq, dtype=np.int64)
    for p, (q, lo) in enumerate(zip(qs, los)):
        la = shared_letters(q, idx[lo], letters) if lo < n else 0
        lb = shared_letters(q, idx[lo - 1], letters) if lo > 0 else 0
        L = max(la, lb)
        d = 0
        if L >= RANGE_LETTERS:
            d = min(L, k_high)
            for k in range(k_low, d + 1):
                if (q >> (5 * (letters - k))) & 31 == HAT:
                    d = k - 1
                    break
            if d < k_low:
                d = 0
        depth[p], rep[p], la_[p], lb_[p] = d, (lo if la >= lb else lo - 1) & 0xFFFFFFFF, la, lb
    return Lookup(depth, rep, np.asarray(los, dtype=np.int64), la_, lb_)


def _bit_length(v: np.ndarray) -> np.ndarray:
    """bit length of every uint64 (exact: the halves are integers a float64 holds, frexp's exponent is their bit length)"""
    hi, lo = (v >> np.uint64(32)).astype(np.float64), (v & np.uint64(0xFFFFFFFF)).astype(np.float64)
    return np.where(hi > 0, 32 + np.frexp(hi)[1], np.frexp(lo)[1]).astype(np.int64)


def lookup_reference_vectorised(idx_kmers: np.ndarray, sorted_queries: np.ndarray, k_high: int, k_low: int) -> Lookup:
    """lookup_reference for 64-bit keys without a Python loop over the queries (the batch of a million queries)"""
    letters, n = 12, int(idx_kmers.shape[0])
    q = sorted_queries
    lo = np.searchsorted(idx_kmers, q, side="left").astype(np.int64)
    shared = lambda other: (5 * letters - _bit_length(q ^ other)) // 5
    la = np.where(lo < n, shared(idx_kmers[np.minimum(lo, n - 1)]), 0)
    lb = np.where(lo > 0, shared(idx_kmers[np.maximum(lo - 1, 0)]), 0)
    L = np.maximum(la, lb)
    d = np.where(L >= RANGE_LETTERS, np.minimum(L, k_high), 0)
    for k in range(k_high, k_low - 1, -1):              # descending: the smallest k with a '^' has the last word
        hat = ((q >> np.uint64(5 * (letters - k))) & np.uint64(31)) == np.uint64(HAT)
        d = np.where(hat & (k <= d), k - 1, d)
    d = np.where(d < k_low, 0, d)
    rep = np.where(la >= lb, lo, lo - 1) & 0xFFFFFFFF
    return Lookup(d.astype(np.uint8), rep.astype(np.uint32), lo, la.astype(np.int64), lb.astype(np.int64))


def table_bits(n: int) -> int:
    tb = 8
    while tb < 28 and (1 << (tb + 1)) <= n:
        tb += 1
    return tb


def span_of_tiles(idx_kmers: np.ndarray, sorted_queries: np.ndarray) -> np.ndarray:
    """Per tile of TILE sorted queries (span, parity of the span's start, the span reaches the index end, the span starts at
    0), as the prefix table fixes them: buckets of the top tb key bits; the span starts one record before the bucket of the
    tile's first query (at 0 at the least) and ends one record after the bucket of its last query (at n at the most)."""
    n, nq = int(idx_kmers.shape[0]), int(sorted_queries.shape[0])
    bits = 125 if is_wide(idx_kmers) else 60
    tb = table_bits(n)
    bucket = lambda keys: formats.key_shr(keys, bits - tb)
    ib = bucket(idx_kmers)
    first = np.arange(0, nq, TILE)
    last = np.minimum(first + TILE - 1, nq - 1)
    start = np.searchsorted(ib, bucket(sorted_queries[first]), side="left").astype(np.int64)
    end = np.searchsorted(ib, bucket(sorted_queries[last]), side="right").astype(np.int64)
    ilo, ihi = np.maximum(start - 1, 0), np.minimum(end + 1, n)
    return np.stack((ihi - ilo, ilo & 1, (ihi == n).astype(np.int64), (ilo == 0).astype(np.int64)), axis=1)


def tile_next_reference(sorted_queries: np.ndarray, depth: np.ndarray, k_high: int, k_low: int) -> np.ndarray:
    """[level k_high - k][tile]: the first position behind the tile that closes the groups of level k, or the number of queries
    (64-bit keys).  A position closes them when it begins a new 6-letter range (it shares less than 6 letters with the query
    before it) or a new matched group of level k (it shares fewer than k letters with the query before it and matches k or
    more).  Only to show what the open-group cases are; the device hands these positions to nobody."""
    q, nq = sorted_queries, int(sorted_queries.shape[0])
    ql = np.zeros(nq, dtype=np.int64)
    ql[1:] = (60 - _bit_length(q[1:] ^ q[:-1])) // 5
    n_tiles = (nq + TILE - 1) // TILE
    out = np.zeros((k_high - k_low + 1, n_tiles), dtype=np.int64)
    for k in range(k_high, k_low - 1, -1):
        at = np.flatnonzero((ql < RANGE_LETTERS) | ((ql < k) & (depth >= k)))
        nxt = np.searchsorted(at, (np.arange(n_tiles) + 1) * TILE, side="left")
        out[k_high - k] = np.where(nxt < at.shape[0], at[np.minimum(nxt, at.shape[0] - 1)], nq)
    return out


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    family: str
    index: str                      # cases of one `index` name share their index (one DeviceIndex)
    ix: formats.Index
    q: np.ndarray                   # the queries as handed in: shuffled
    payload: np.ndarray             # uint32 per query
    n_reads: int
    windows: list                   # (k_high, k_low) to look the batch up under
    score_windows: list = field(default_factory=list)    # ... and to score it under
    runs: list = field(default_factory=list)             # span family: the spans as designed, per tile

    @property
    def letters(self) -> int:
        return self.ix.K

    @property
    def wide(self) -> bool:
        return self.ix.K > 12

    @property
    def n(self) -> int:
        return int(self.q.shape[0])

    @functools.cached_property
    def sorted(self):
        return stable_sort(self.q, self.payload)

    @functools.cached_property
    def spans(self) -> np.ndarray:
        return span_of_tiles(self.ix.kmer, self.sorted[0])


def content(n_taxa: int = N_TAXA) -> formats.Content:
    return formats.Content(["non_unique"] + ["T%d" % t for t in range(1, n_taxa)], (np.arange(n_taxa, dtype=np.uint32) * np.uint32(10)))


def _index(entries, wide: bool, n_taxa: int = N_TAXA) -> formats.Index:
    """entries: (key as an integer, taxon 1 .. n_taxa - 1)"""
    c = content(n_taxa)
    return formats.make_index(keys_from_ints([e[0] for e in entries], wide), c.taxids[np.array([e[1] for e in entries], dtype=np.int64)], c)


def _shuffled(name, family, index, ix, queries, seed, windows, score_windows=(), payload=None, n_reads=None, runs=()):
    wide = ix.K > 12
    q = queries if isinstance(queries, np.ndarray) else keys_from_ints(queries, wide)
    rng = np.random.default_rng(seed)
    order = rng.permutation(q.shape[0])
    if payload is None:
        payload, n_reads = rng.permutation(q.shape[0]).astype(np.uint32), int(q.shape[0])
    else:
        payload = np.asarray(payload, dtype=np.uint32)[order]
    return Case(name, family, index, ix, np.ascontiguousarray(q[order]), np.ascontiguousarray(payload), int(n_reads), list(windows), list(score_windows), list(runs))


# ---- main ---------------------------------------------------------------------------------------
MANY_TAXA = 40                                          # taxa of the k-mer that fills a row of equal keys
REPEATS = {"exact": 2, "above": 5, "many exact": 600, "many above": 600}
HAT_PAIRS = {12: [(3, 9), (7, 8), (8, 12)], 25: [(3, 9), (7, 8), (8, 12), (13, 14), (18, 25), (7, 20)]}


def _filler(K):
    """1700 entries that begin with letter 15: between the comb's 10 and the 20 of the '^' family"""
    return [pack([15, a, b, c] + [1] * (K - 4)) for a in range(1, 13) for b in range(1, 13) for c in range(1, 13)][:1700]


@functools.lru_cache(maxsize=None)
def _main_index(K: int, filler: bool):
    """The comb: B = 10 10 10 ... is not in the index, but per letter j the entries B with an 8 and B with a 12 at j are.  A
    query that leaves B at letter j then has its neighbours at known shared lengths (see _main_queries)."""
    B = [10] * K
    e = []
    for j in range(1, K + 1):
        for t in ((1, 2) if j == 3 else (1 + j % 5,)):
            e.append((pack(sub(B, (j, 8))), t))
        many = range(1, 1 + MANY_TAXA) if j == 9 else range(2, 3 + MANY_TAXA) if (K == 25 and j == 20) else (2 + j % 7,)
        for t in many:
            e.append((pack(sub(B, (j, 12))), t))
    if K == 25:                                                          # the seam of the two words is inside letter 13
        e.append((pack(sub(B, (13, 26))), 3))
        e.append((pack(sub([11] * K, (13, 8))), 4))
    e += [(pack([20] * K), 5), (pack([20] * K), 6)]                     # the plain entry of the '^' family
    for h in range(1, K + 1):
        e.append((pack(sub([22] * K, (h, HAT))), 7 + h % 3))            # entries that hold a '^' themselves
    for h1, h2 in HAT_PAIRS[K]:
        e.append((pack(sub([22] * K, (h1, HAT), (h2, HAT))), 11))
    if filler:
        e += [(k, 12) for k in _filler(K)]
    return _index(e, K > 12)


def _main_queries(K: int, filler: bool, phase: int):
    B, P, P2 = [10] * K, [20] * K, [22] * K
    q = [0] * phase                                                      # moves every other query `phase` places up
    for j in range(1, K + 1):
        q.append(pack(sub(B, (j, 9))))                                   # between the 8 and the next entry: la == lb == j - 1
        q += [pack(sub(B, (j, 8))), pack(sub(B, (j, 12)))]              # exact
        if j < K:
            q.append(pack(sub(B, (j, 8), (j + 1, 5))))                  # just below the 8: la == j > lb
            q.append(pack(sub(B, (j, 12), (j + 1, 15))))                # just above the 12: lb == j > la
    if K == 25:
        q += [pack(sub(B, (13, 27))), pack(sub(B, (13, 24))), pack(sub(B, (13, 26))), pack(sub([11] * K, (13, 24))), pack(sub([11] * K, (13, 9))),
              pack(sub([11] * K, (13, 20)))]
    q += [pack(sub(B, (5, 8)))] * (REPEATS["exact"] - 1) + [pack(sub(B, (4, 12), (5, 15)))] * (REPEATS["above"] - 1)
    q += [pack(sub(B, (9, 12)))] * (REPEATS["many exact"] - 1) + [pack(sub(B, (9, 12), (10, 15)))] * (REPEATS["many above"] - 1)
    if K == 25:
        q += [pack(sub(B, (20, 12)))] * 300
    # '^' later than the match: the plain entry's first D letters, then the query leaves it -- with a '^' (h == D + 1) or without
    for D in range(K + 1):
        if D == K:
            q.append(pack(P))
            continue
        for h in [0] + list(range(D + 1, K + 1)):
            x = HAT if h == D + 1 else (19 if D % 2 else 21)
            l = P[:D] + [x] + [21] * (K - D - 1)
            if h > D + 1:
                l[h - 1] = HAT
            q.append(pack(l))
    for D, h1, h2 in ((7, 9, 11), (6, 7, 12), (8, 9, 10), (K - 3, K - 1, K)):      # two '^' behind the match
        q.append(pack(sub(P[:D] + [21] * (K - D), (h1, HAT), (h2, HAT))))
    # '^' inside the match: the first D >= h letters of the entry with a '^' at h
    for h in range(1, K + 1):
        e = sub(P2, (h, HAT))
        for D in range(h, K + 1):
            q.append(pack(e if D == K else e[:D] + [21 if D % 2 else 23] + [21] * (K - D - 1)))
    for h1, h2 in HAT_PAIRS[K]:
        e = sub(P2, (h1, HAT), (h2, HAT))
        for D in range(h2, K + 1):
            q.append(pack(e if D == K else e[:D] + [23] + [21] * (K - D - 1)))
    if filler:
        f = _filler(K)
        q += f[::40] + [k + 1 for k in f[5::170]] + [k - 1 for k in f[7::170]]
    return q


def main_case(K: int, filler: bool, phase: int) -> Case:
    name = "main%d%s%s" % (64 if K == 12 else 128, "+filler" if filler else "", " phase %d" % phase if phase else "")
    windows = WINDOWS[K] if phase == 0 else WINDOWS[K][:1]
    score = WINDOWS[K][:1] if phase == 0 else []
    return _shuffled(name, "main", name.split(" ")[0], _main_index(K, filler), _main_queries(K, filler, phase), 100 + phase, windows, score)


# ---- span ---------------------------------------------------------------------------------------
SPAN_RUNS = {"a": [(LSPAN - 1, 0), (LSPAN + 1, 1), (LSPAN, 1)],        # (span, parity of its start); the last run ends the index
             "b": [(LSPAN, 1), (LSPAN + 2, 0), (LSPAN - 1, 1)],
             "c": [(LSPAN + 1, 0), (LSPAN + 2, 1), (LSPAN, 0)]}
SPAN_LAST_QUERIES = {"a": 700, "b": TILE, "c": 1001}


def _run_letters(rng, X, R, K):
    """R different entries of one prefix-table bucket (tb <= 12: the first two letters and two bits of the third), in few
    6-letter ranges"""
    seen = {}
    while len(seen) < R:
        l = [X, 7, int(rng.integers(8, 10))] + rng.integers(1, 3, size=3).tolist() + rng.integers(1, 21, size=K - 6).tolist()
        seen.setdefault(pack(l), l)
    return [seen[k] for k in sorted(seen)]


def _run_queries(rng, run, n, K):
    """n queries inside the run's bucket: on entries, and leaving an entry at some letter from the fourth on; drawn from four
    windows of the run, so that the lower bounds of neighbouring queries lie far apart where a window ends"""
    X, R = run[0][0], len(run)
    out = [pack([X, 7, 8] + [0] * (K - 3)), pack([X, 7, 15] + [31] * (K - 3))]      # below and above the whole run
    windows = [(0, 200, 301), (300, 500, 202), (700, 720, 51), (1000, R, 1 << 30)]
    for a, b, cnt in windows:
        for _ in range(min(cnt, n - len(out))):
            e = run[int(rng.integers(a, b))]
            if rng.random() < 0.4:
                out.append(pack(e))
                continue
            c = int(rng.integers(4, K + 1))
            x = int(rng.choice([0, 21, HAT, (e[c - 1] + 1) % 22]))
            tail = [HAT if rng.random() < 0.05 else int(v) for v in rng.integers(1, 21, size=K - c)]
            out.append(pack(e[:c - 1] + [x if x != e[c - 1] else 31] + tail))
    assert len(out) == n
    return out


def span_case(which: str, K: int) -> Case:
    rng = np.random.default_rng(200 + ord(which) + K)
    runs = SPAN_RUNS[which]
    entries, queries, count = [], [], 0
    for j, (span, parity) in enumerate(runs):
        last = j == len(runs) - 1
        X = 3 + 3 * j
        pad = 1 if j == 0 else 0
        if K == 12 and (count + pad - 1) % 2 != parity:      # (the staging of 16-byte keys has no shift: no parity to meet)
            pad += 1
        entries += [(pack([X - 1, 1 + i] + [4] * (K - 2)), 1) for i in range(pad)]
        run = _run_letters(rng, X, span - 1 if last else span - 2, K)
        entries += [(pack(l), 1 + i % 3) for i, l in enumerate(run)]
        count += pad + len(run)
        queries += _run_queries(rng, run, SPAN_LAST_QUERIES[which] if last else TILE, K)
    ix = _index(entries, K > 12)
    assert ix.n == count
    name = "span%d %s" % (64 if K == 12 else 128, which)
    return _shuffled(name, "span", name, ix, queries, 300 + ord(which), WINDOWS[K][:1], WINDOWS[K][:1] if which == "a" else [], runs=runs)


# ---- ends ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ends_entries(K: int, n: int):
    if n <= 3:
        return [[16] * K, [16] * 7 + [17] * (K - 7), [17] * K][:n]
    rng = np.random.default_rng(400 + K)
    seen = {}
    while len(seen) < n:
        l = rng.integers(1, 4, size=8).tolist() + rng.integers(1, 21, size=K - 8).tolist()
        seen.setdefault(pack(l), l)
    return [seen[k] for k in sorted(seen)]


@functools.lru_cache(maxsize=None)
def _ends_index(K: int, n: int):
    e = _ends_entries(K, n)
    two = e[::7] if n > 3 else []                                                # (of the larger index every seventh k-mer under two taxa)
    return _index([(pack(l), 1 + i % 4) for i, l in enumerate(e)] + [(pack(l), 5) for l in two], K > 12)


def ends_case(K: int, n: int, batch: int) -> Case:
    rng = np.random.default_rng(500 + K + n + batch)
    e = _ends_entries(K, n)
    first, last = pack(e[0]), pack(e[-1])
    q = [last + 1, first - 1, first, last, (1 << (5 * K)) - 1, 0][:batch]          # above, below, on the ends; the top and the bottom bucket
    while len(q) < batch:
        l = e[int(rng.integers(0, len(e)))]
        c = int(rng.integers(1, K + 2))                                            # leaves the entry at letter c (K + 1: not at all)
        q.append(pack(l if c > K else l[:c - 1] + [int(rng.choice([0, 21, HAT, 31]))] + [HAT if rng.random() < 0.05 else int(v) for v in rng.integers(1, 21, size=K - c)]))
    name = "ends%d n%d b%d" % (64 if K == 12 else 128, n, batch)
    return _shuffled(name, "ends", "ends%d n%d" % (K, n), _ends_index(K, n), q, 600 + batch, WINDOWS[K][:1])


ENDS = [(1, 1), (1, 3), (2, 4), (3, 5), (301, 5), (301, 1023), (301, 1024), (301, 1025), (301, 2049)]     # (index entries, batch)


# ---- open ---------------------------------------------------------------------------------------
# One 6-letter range Z.  Under the seventh letters 1, 10, 20 (and 31) the index holds four k-mers each, under two or three
# taxa; the matched queries of reads 0 .. 5 lie there.  Between them lie stretches of queries with seventh letters the index
# does not have: they share Z with it and nothing more (L == 6: no match at k_low = 7), so no position of a stretch closes a
# group at any level.  The early block matches deep (up to 12), the middle block at most 9 letters, the late block begins
# shallow: the early block's groups of the levels 10 .. 12 stay open over the middle block and close in the late one, behind
# the flush of the middle block's groups -- an order that only the tiles' next special positions carry.
OPEN_Z = [5] * 6
OPEN_ENTRIES = [([1, 1, 1, 1, 1], (1, 2)), ([1, 1, 1, 1, 2], (1, 3)), ([1, 1, 2, 1, 1], (2, 3, 4)), ([2, 1, 1, 1, 1], (1, 2, 3))]
OPEN_DEEP = [[1, 1, 1, 1, 1], [1, 1, 1, 1, 2], [1, 1, 1, 1, 3], [1, 1, 1, 3, 3], [1, 1, 2, 1, 1], [1, 1, 2, 1, 3], [1, 1, 3, 1, 1], [1, 3, 1, 1, 1],
             [2, 1, 1, 1, 1], [2, 3, 1, 1, 1], [3, 1, 1, 1, 1]]
OPEN_SHALLOW = [[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [1, 1, 0, 0, 0], [1, 3, 1, 1, 1], [2, 0, 0, 0, 0], [3, 1, 1, 1, 1]]
OPEN_READS, OPEN_MATCHED_READS = 40, 6
OPEN_LAYOUTS = {  # stretch lengths (None: so that the middle block begins a tile); a matched query as the batch's last one
    "open6": dict(s1=3 * TILE + 500, s2=1500, s3=1500, final=False),
    "open6 edges": dict(s1=None, s2=1300, s3=1100, final=True),
    "open1k": dict(s1=(CHUNK_TILES + 1) * TILE + 300, s2=1500, s3=600, final=False),
}


@functools.lru_cache(maxsize=None)
def _open_index():
    e = [(pack([4] * 12), 5), (pack([6] * 12), 5)]                                # (the range is not at an end of the index)
    for a in (1, 10, 20, 31):
        for tail, taxa in OPEN_ENTRIES:
            e += [(pack(OPEN_Z + [a] + tail), t) for t in taxa]
    return _index(e, False, 6)


def _open_block(a, tails):
    """(key, read): every query of the block for three of the reads 0 .. 5"""
    return [(pack(OPEN_Z + [a] + t), (i + s) % OPEN_MATCHED_READS) for i, t in enumerate(tails) for s in (0, 1, 3)]


def open_case(name: str) -> Case:
    lay = OPEN_LAYOUTS[name]
    rng = np.random.default_rng(700 + len(name))
    early, middle = _open_block(1, OPEN_DEEP), _open_block(10, OPEN_SHALLOW)
    late = _open_block(20, OPEN_SHALLOW[:1] + OPEN_DEEP)
    s1 = lay["s1"] if lay["s1"] is not None else 2 * TILE - len(early)
    keys, reads = [], []

    def matched(block):
        keys.append(np.array([k for k, _ in block], dtype=np.uint64)); reads.append(np.array([r for _, r in block], dtype=np.uint32))

    def stretch(n, sevenths):
        k = np.uint64(pack(OPEN_Z) << 30) | (rng.choice(np.array(sevenths, dtype=np.uint64), size=n) << np.uint64(25)) | rng.integers(0, 1 << 25, size=n, dtype=np.uint64)
        keys.append(k); reads.append(rng.integers(0, OPEN_READS, size=n).astype(np.uint32))

    matched(early); stretch(s1, [4, 5, 6]); matched(middle); stretch(lay["s2"], [14, 15]); matched(late); stretch(lay["s3"], [25])
    if lay["final"]:
        matched([(pack(OPEN_Z + [31, 1, 1, 1, 1, 1]), 2)])
    return _shuffled(name, "open", "open", _open_index(), np.concatenate(keys), 800 + len(name), [(12, 7)], [(12, 7)],
                     payload=np.concatenate(reads), n_reads=OPEN_READS)


# ---- the list -----------------------------------------------------------------------------------
def _builders():
    b = {}
    for K in (12, 25):
        w = 64 if K == 12 else 128
        for filler in (False, True):
            for phase in range(4 if not filler else 1):
                b["main%d%s%s" % (w, "+filler" if filler else "", " phase %d" % phase if phase else "")] = functools.partial(main_case, K, filler, phase)
        for which in SPAN_RUNS:
            b["span%d %s" % (w, which)] = functools.partial(span_case, which, K)
        for n, batch in ENDS:
            b["ends%d n%d b%d" % (w, n, batch)] = functools.partial(ends_case, K, n, batch)
    for name in OPEN_LAYOUTS:
        b[name] = functools.partial(open_case, name)
    return b


_BUILDERS = _builders()
LARGE = "open1k"
SCORED = ["main64", "main64+filler", "span64 a", "main128", "main128+filler", "span128 a"] + list(OPEN_LAYOUTS)     # the cases with score_windows


def case_names(large: bool = True) -> list:
    return [n for n in _BUILDERS if large or n != LARGE]


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def reference(name: str, k_high: int, k_low: int) -> Lookup:
    """the reference of a case under a window, computed once (the vectorised form for the batch of a million queries)"""
    c = case(name)
    if name == LARGE:
        return lookup_reference_vectorised(c.ix.kmer, c.sorted[0], k_high, k_low)
    return lookup_reference(c.ix.kmer, c.sorted[0], k_high, k_low, c.letters)
