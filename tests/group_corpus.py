"""Hand-made indices and query batches for the group stage (kasa_batch_group: group2_kernel, its second launch, group_kernel
with walk_segments and coop_walk, the pool's retry loop), with a plain reference of the event record the stage leaves per
sorted query, a decoder of what kasa_batch_records_fetch returns and an encoder of the reference into the same layout.  The
inputs of tests/test_group_corpus_cpu.py (the corpus is what it claims, decode(encode(reference)) is the reference, the
reference replayed event by event is the sequential oracle) and tests/test_gpu_group_corpus.py (the device under every route
of group_stage).  Pure numpy, kasa_amd/formats.py and tests/lookup_corpus.py: no device, no reference tree.

A case is one index, one batch handed in shuffled with every query its own read, and the level windows to group it under.
Every case is laid out in SORTED order (Layout): the keys are made so that they sort as they are added, which is what lets a
case say "this leader stands at position 1023 and the query that closes its groups at 1024".

Keys.  A cluster c owns one 6-letter range Z(c); its representative is R = Z + 10 10 10 ...; near(R, s, side, i) is the i-th key
that shares exactly s letters with R and lies left (smaller) or right of it.  Sorted, the entries left and right of R share
fewer and fewer letters with it the farther they lie: the list a query at R walks.  Between the clusters lie filler queries
that share three letters with the cluster before them and match nothing; inside a range, stretch queries (seventh letter 20,
which no entry has) share the range and nothing more.

Families (the names of DESIGN 8l):
  walk       one list of N entries beyond the representative per tile, N = WALK_N, all left / all right / both sides; two
             such leaders in a tile's first wavefront and one in its last; whole: the list is the whole index
  count      lists of 254, 255, 256 and 300 segments; one level of 6, 7, 8, 255, 256 taxa over levels of one; INL and INL + 1
  split      runs of one taxon with every dup from 5 to K - 1, entries and representatives that yield no segment, equal keys
  order      two entries per shared length and side: ties of kLast on both sides, F_k up and down in k, ties of F, 8 / 10 / 19 events
  flush      the closing query of a leader's levels in its lane pair, a later lane, the next wavefront, the next tile, nowhere
  followers  runs of equal (representative, depth) of FOLLOWER_RUNS queries from an even and an odd position, with a pool block;
             the same representative at depths cut by a '^'
  hits       groups of HIT_GROUPS equal queries (the last one past the 16 hit bits of a group key)
  span       tiles whose representatives span G2_SPAN and GSPAN - 1, + 0, + 1 entries with the margins; a walk that leaves the
             staged span; walks of 95, 96, 97 entries beyond the first and the last representative
  park       tiles whose leaders walk at most G2_STEPS entries each and together park PARK_EDGES segments
  pool       300 wavefronts that each lead a list of 250 segments: the first pool is too small
  ends       batches of 1, 2, 127 .. 129, 1023 .. 1025, 2049 queries; indices of 1, 2, 3 entries; a batch that matches nothing
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from tests import lookup_corpus as lc

# ------------------------------------------------------------------------------------------------
# kasa_hip.hip's constants, by the names they have there (tests/test_group_corpus_cpu.py reads them out of the file)
# ------------------------------------------------------------------------------------------------
TILE = 1024                       # sorted queries per workgroup
WAVE = 128                        # ... per wavefront: 64 lanes, GITEMS = 2 consecutive queries each
RANGE_LETTERS = 6
G2_STEPS = 40                     # group2_kernel: entries a leader's walk may visit beyond its representative; more: the tile is listed
LONG_STEPS, LONG_STEPS_CROWDED = 48, 8      # group_kernel<COOP>: entries a lane walks before its wavefront takes the list (coop_walk)
COOP_CHUNK = 64                   # coop_walk: entries per step, one per lane
INL = {8: 4, 16: 8}               # RecTraits<8|16>::INL: segments inside the record; a longer list keeps INL - 1 and a pool offset
SEG0 = {8: 4, 16: 8}              # RecTraits::SEG0: the first segment word
OBITS = {8: 3, 16: 5}             # RecTraits::OBITS: bits per event of the order field
REC_SPLIT, REC_SAT = 1 << 29, 1 << 30
POOL_SIZES = 4                    # words of exact level sizes in the pool block of a REC_SAT record
NSEG_CAP, SIZE_CAP = 255, 7       # word [3] of a narrow record: "255 or more" segments, "7 or more" taxa of a level
# group2_kernel parks, per leader, the segments beyond the FOURTH (n - INL of a list of n > INL); more than G2_OVF of them in a
# tile: the tile is listed.  G2_OVF holds for its six-level form (64-bit keys, six levels); the general form (any other level
# count up to eight, and 128-bit keys) has half of it.  The second launch (six levels, 64-bit keys, at most a quarter of the
# tiles listed) has four times G2_OVF.
G2_OVF = 1024
# group_kernel parks, per leader, the segments from the fourth on (n - (INL - 1) of a list of n >= INL, narrow records); more
# than GOVF of them in a tile: the tile's lists are walked a second time
GOVF = 1024
G2_SPAN, GSPAN, GMARGIN = 1792, 3072, 96    # index entries staged per tile: the representatives and GMARGIN beyond each end

HAT = lc.HAT
WINDOWS = lc.WINDOWS
N_TAXA = 302                      # content entries: lists of 300 distinct taxa exist
shared_letters, pack = lc.shared_letters, lc.pack


def rec_words(k_high: int, k_low: int) -> int:
    return 8 if k_high - k_low + 1 <= 8 else 16


def g2_ovf(n_levels: int, wide_keys: bool, second: bool = False) -> int:
    return (G2_OVF if (n_levels == 6 and not wide_keys) else G2_OVF // 2) * (4 if second else 1)


# ------------------------------------------------------------------------------------------------
# the record of one query, as the reference computes it and as the decoder reads it
# ------------------------------------------------------------------------------------------------
@dataclass
class Rec:
    p: int                       # sorted position
    d: int                       # deepest matched level, 0: none (then nothing else is set)
    fmax: int = 0
    order: tuple = ()            # lv = k_high - k of the events in flush order
    segs: tuple = ()             # (taxon, kFirst, kLast) in list order
    sizes3: tuple = ()           # narrow records: |T_k| per lv = 0 .. nK - 1, capped at 7
    sizes: tuple = ()            # exact |T_k| per lv (the reference: always; the decoder: where REC_SAT is set, else sizes3)
    split: bool = False
    sat: bool = False
    F: tuple = ()                # reference only: F_k for k = k_low .. d
    walk: tuple = (0, 0)         # reference only: entries of the kLow-group left and right of the representative
    rep: int = 0                 # reference only
    block: tuple = None          # decoder only: [begin, end) of the pool block, None: no block
    block_nseg: int = None       # decoder only: the block's first word

    def fields(self, wide: bool):
        """what a decoded record and the reference must agree in"""
        if self.d == 0:
            return {"d": 0}
        f = {"d": self.d, "p": self.p, "Fmax": self.fmax, "order": self.order, "nseg": len(self.segs), "segments": self.segs, "REC_SPLIT": self.split}
        if not wide:
            f.update({"sizes (3 bits)": self.sizes3, "REC_SAT": self.sat})
            if self.sat:
                f["sizes (exact)"] = self.sizes
        return f


def dup_letters(idx: list, tax: list, letters: int) -> list:
    """per index entry the letters it shares with the nearest earlier entry of its taxon, 0: there is none"""
    last, out = {}, []
    for i, t in enumerate(tax):
        out.append(shared_letters(idx[last[t]], idx[i], letters) if t in last else 0)
        last[t] = i
    return out


def reference(case, k_high: int, k_low: int) -> list:
    """One Rec per sorted query, from the definitions of DESIGN 3 and 3b in plain loops over Python integers.
    d and the representative: lookup_corpus.lookup_reference.  A position is special for level k when it begins a new 6-letter
    range or opens a new matched level-k group (it shares fewer than k letters with the query before it and matches k or more);
    F_k(p) = the next special position behind p, nQ at the end.  The events of p: the levels k_low .. d by (F, k).  The segments:
    every index entry that shares the kLow-group's letters (k_low, 6 at the least) with the query gives (taxon, kFirst, kLast),
    kLast = min(d, letters shared with the query), kFirst = k_low where the entry shares fewer than 6 letters with the nearest
    earlier entry of its taxon, else max(that + 1, k_low); no segment where kFirst > kLast; the representative first, then by
    kLast descending, left of the representative before right, nearest first."""
    K = case.letters
    look = lc.lookup_reference(case.ix.kmer, case.sorted[0], k_high, k_low, K)
    qs, idx, tax = lc.key_ints(case.sorted[0]), lc.key_ints(case.ix.kmer), case.ix.tax.tolist()
    nq, n, n_lv, wide = len(qs), len(idx), k_high - k_low + 1, rec_words(k_high, k_low) == 16
    d, rep = look.depth.tolist(), look.rep.tolist()
    ql = [0] + [shared_letters(qs[p - 1], qs[p], K) for p in range(1, nq)]
    F = {}
    for k in range(k_low, k_high + 1):
        col, nxt = [0] * nq, nq
        for p in range(nq - 1, -1, -1):
            col[p] = nxt
            if ql[p] < RANGE_LETTERS or (ql[p] < k and d[p] >= k):
                nxt = p
        F[k] = col
    dup, g_low = dup_letters(idx, tax, K), max(k_low, RANGE_LETTERS)

    def segments(q, dq, j):
        items = []

        def one(i, side, dist):
            k_last = min(dq, shared_letters(q, idx[i], K))
            k_first = k_low if dup[i] < RANGE_LETTERS else max(dup[i] + 1, k_low)
            if k_first <= k_last:
                items.append((-k_last, side, dist, tax[i], k_first))
        one(j, -1, 0)
        i = j - 1
        while i >= 0 and shared_letters(q, idx[i], K) >= g_low:
            one(i, 0, j - i)
            i -= 1
        left = j - 1 - i
        i = j + 1
        while i < n and shared_letters(q, idx[i], K) >= g_low:
            one(i, 1, i - j)
            i += 1
        items.sort()
        segs = tuple((t, kf, -nkl) for nkl, _, _, t, kf in items)
        sizes = tuple(sum(1 for _, kf, kl in segs if kf <= k_high - lv <= kl) for lv in range(n_lv))
        for lv in range(n_lv):                                            # a taxon is in T_k once
            at = [t for t, kf, kl in segs if kf <= k_high - lv <= kl]
            assert len(at) == len(set(at)), (case.name, q, lv)
        return segs, sizes, any(kf > k_low for _, kf, _ in segs), (left, i - j - 1)

    cache, out = {}, []
    for p in range(nq):
        if d[p] == 0:
            out.append(Rec(p, 0))
            continue
        if qs[p] not in cache:
            cache[qs[p]] = segments(qs[p], d[p], rep[p])
        segs, sizes, split, walk = cache[qs[p]]
        ev = sorted((F[k][p], k) for k in range(k_low, d[p] + 1))
        out.append(Rec(p, d[p], ev[-1][0], tuple(k_high - k for _, k in ev), segs, () if wide else tuple(min(s, SIZE_CAP) for s in sizes), sizes, split,
                       (not wide) and max(sizes) >= SIZE_CAP, tuple(F[k][p] for k in range(k_low, d[p] + 1)), walk, rep[p]))
    return out


# ------------------------------------------------------------------------------------------------
# the layout of the header comment "event records" of kasa_hip.hip, read and written
#   [0] p   [1] Fmax   [2] d | order << 5 (narrow) | REC_SPLIT | REC_SAT (narrow)   [3] nseg (narrow: low byte, 255 = "255 or
#   more", and |T_k| of lv = 0 .. 7 above it, 3 bits each, 7 = "7 or more")
#   narrow: [4..7] up to 4 segments, else 3 and [7] = the pool offset    wide: [4..7] order, 5 bits per event; [8..15] up to 8
#   segments, else 7 and [15] = the pool offset
#   pool block: {nseg, [4 words of exact sizes, 16 bits per level, with REC_SAT], the segments from INL - 1 on}
#   segment: taxon | kFirst << 22 | kLast << 27
# ------------------------------------------------------------------------------------------------
def _seg_word(s) -> int:
    return s[0] | (s[1] << 22) | (s[2] << 27)


def _seg_of(w: int):
    return (w & ((1 << 22) - 1), (w >> 22) & 31, w >> 27)


def decode_one(w: list, pool, rw: int, k_high: int, k_low: int) -> Rec:
    d = w[2] & 31
    if d == 0:
        return Rec(w[0], 0)
    n_ev, n_lv, inl, seg0 = d - k_low + 1, k_high - k_low + 1, INL[rw], SEG0[rw]
    if rw == 8:
        order_bits, n = (w[2] >> 5) & 0xFFFFFF, w[3] & 255
        sat = bool(w[2] & REC_SAT)
        sizes3 = tuple((w[3] >> (8 + 3 * lv)) & 7 for lv in range(n_lv))
    else:
        order_bits, n, sat, sizes3 = w[4] | (w[5] << 32) | (w[6] << 64) | (w[7] << 96), w[3], False, ()
    order = tuple((order_bits >> (OBITS[rw] * e)) & ((1 << OBITS[rw]) - 1) for e in range(n_ev))
    sizes, block, block_nseg = sizes3, None, None
    if n <= inl:
        segs = [w[seg0 + i] for i in range(n)]
    else:
        off = w[seg0 + inl - 1]
        block_nseg = int(pool[off])
        if rw == 8 and n == NSEG_CAP:
            n = block_nseg
        skip = POOL_SIZES if sat else 0
        if sat:
            sizes = tuple((int(pool[off + 1 + (lv >> 1)]) >> (16 * (lv & 1))) & 0xFFFF for lv in range(n_lv))
        begin = off + 1 + skip
        block = (off, begin + n - (inl - 1))
        segs = [w[seg0 + i] for i in range(inl - 1)] + pool[begin:block[1]].tolist()
    return Rec(w[0], d, w[1], order, tuple(_seg_of(s) for s in segs), sizes3, sizes, bool(w[2] & REC_SPLIT), sat, block=block, block_nseg=block_nseg)


def decode(rec: np.ndarray, pool: np.ndarray, rw: int, k_high: int, k_low: int, rows=None) -> list:
    """What Context.records() returns -> one Rec per record (of `rows`), with every pool block's extent"""
    rows = range(rec.shape[0]) if rows is None else rows
    return [decode_one(rec[p].tolist(), pool, rw, k_high, k_low) for p in rows]


def encode(recs: list, rw: int, k_high: int, k_low: int):
    """The reference in the device's layout: (rec u32[nQ, rw], pool u32[]); every list its own pool block, from word 1 on"""
    out = np.zeros((len(recs), rw), dtype=np.uint32)
    pool = [0]
    for r in recs:
        w = [0] * rw
        w[0] = r.p
        if r.d:
            order = 0
            for e, lv in enumerate(r.order):
                order |= lv << (OBITS[rw] * e)
            n, inl, seg0 = len(r.segs), INL[rw], SEG0[rw]
            w[1], w[2] = r.fmax, r.d | (REC_SPLIT if r.split else 0)
            if rw == 8:
                w[2] |= (order << 5) | (REC_SAT if r.sat else 0)
                w[3] = min(n, NSEG_CAP) | (sum(s << (3 * lv) for lv, s in enumerate(r.sizes3)) << 8)
            else:
                w[3] = n
                for i in range(4):
                    w[4 + i] = (order >> (32 * i)) & 0xFFFFFFFF
            words = [_seg_word(s) for s in r.segs]
            if n <= inl:
                w[seg0:seg0 + n] = words
            else:
                w[seg0:seg0 + inl - 1] = words[:inl - 1]
                w[seg0 + inl - 1] = len(pool)
                pool.append(n)
                if rw == 8 and r.sat:
                    sz = list(r.sizes) + [0] * (8 - len(r.sizes))
                    pool += [sz[2 * i] | (sz[2 * i + 1] << 16) for i in range(POOL_SIZES)]
                pool += words[inl - 1:]
        out[r.p] = w
    return out, np.array(pool, dtype=np.uint32)


# ------------------------------------------------------------------------------------------------
# the records replayed: what tests/test_group_corpus_cpu.py and tests/test_score_corpus_cpu.py hold against the sequential oracle,
# and the reference of tests/test_gpu_score_corpus.py
# ------------------------------------------------------------------------------------------------
def replay(c, recs, kh, kl):
    """the reference's records as the reference program would flush them: events in (F, k) order, M[read][t] += w_k * (1 / |T_k|)
    in float32 for every taxon of T_k; per group (level, F) hits / |T_k| into countAll, hits into countUnique where |T_k| = 1"""
    n_taxa = c.ix.content.n_taxa
    reads = c.sorted[1].tolist()
    M = np.zeros((c.n_reads, n_taxa), dtype=np.float32)
    ca, cu = np.zeros((kh - kl + 1, n_taxa), dtype=np.float64), np.zeros((kh - kl + 1, n_taxa), dtype=np.uint64)
    groups = {}
    for r in recs:
        for i, f in enumerate(r.F):
            groups.setdefault((f, kl + i), []).append(r.p)
    taxa_of = {}
    for (f, k), members in sorted(groups.items()):                       # a flush: one group of one level
        sets = set()
        for p in members:
            key = (id(recs[p].segs), k)
            if key not in taxa_of:
                taxa_of[key] = tuple(sorted(t for t, kf, kl_ in recs[p].segs if kf <= k <= kl_))
            sets.add(taxa_of[key])
        assert len(sets) == 1, (c.name, k, f, "the members of a group see one taxon set")
        t = np.array(sets.pop(), dtype=np.int64)
        score = (np.float32(k * k) / np.float32(625)) * (np.float32(1) / np.float32(t.shape[0]))
        rows = [reads[p] for p in members]
        if len(set(rows)) == len(rows):                                   # every hit another read: the cells are all different
            M[np.ix_(rows, t)] += score
        else:
            for r in rows:
                M[r, t] += score
        ca[kh - k, t] += float(len(members)) / float(t.shape[0])
        if t.shape[0] == 1:
            cu[kh - k, t] += np.uint64(len(members))
    return M, ca, cu


# ------------------------------------------------------------------------------------------------
# what a batch asks of group_stage, from the reference and the constants above
# ------------------------------------------------------------------------------------------------
def leaders(recs: list) -> list:
    """True per sorted query that walks the index itself: a matched query whose (representative, depth) are not those of the
    query before it in its wavefront"""
    return [r.d != 0 and (p % WAVE == 0 or (recs[p - 1].rep, recs[p - 1].d) != (r.rep, r.d) or recs[p - 1].d == 0) for p, r in enumerate(recs)]


def tile_facts(recs: list, n_idx: int) -> list:
    """Per tile: the longest walk of a leader, the segments group2_kernel parks (beyond the fourth) and group_kernel parks (from
    the fourth on), the staged span with its margins (first .. last representative as the kernels take them: of each
    wavefront's first and last matched query), and whether a leader's walk touches an entry outside group2_kernel's staged
    window (the entries it visits and the one it looks at behind the last one on the right)."""
    lead, out = leaders(recs), []
    for t0 in range(0, len(recs), TILE):
        tile = recs[t0:t0 + TILE]
        lo, hi = None, None
        for w0 in range(0, len(tile), WAVE):
            m = [r.rep for r in tile[w0:w0 + WAVE] if r.d]
            if m:
                lo, hi = (m[0] if lo is None else min(lo, m[0])), (m[-1] if hi is None else max(hi, m[-1]))
        ls = [r for r, l in zip(tile, lead[t0:t0 + TILE]) if l]
        f = {"walk": max([sum(r.walk) for r in ls], default=0), "parked2": sum(max(0, len(r.segs) - 4) for r in ls),
             "parked": sum(len(r.segs) - 3 for r in ls if len(r.segs) >= 4), "span": 0, "outside": False, "leaders": len(ls),
             "longest": max([len(r.segs) for r in ls], default=0)}
        if lo is not None:
            s_lo, s_hi = max(lo - GMARGIN, 0), min(hi + GMARGIN + 1, n_idx)
            f["span"] = s_hi - s_lo
            end = s_lo + min(s_hi - s_lo, G2_SPAN)
            f["outside"] = any(r.rep - r.walk[0] < s_lo or min(r.rep + r.walk[1] + 1, n_idx - 1) >= end for r in ls)
        out.append(f)
    return out


def listed_tiles(facts: list, n_levels: int, wide_keys: bool):
    """(tiles group2_kernel lists, tiles its second launch lists again) on the product route for narrow records"""
    first = [f for f in facts if f["walk"] > G2_STEPS or f["outside"] or f["parked2"] > g2_ovf(n_levels, wide_keys)]
    again = first
    if first and n_levels == 6 and not wide_keys and 4 * len(first) <= len(facts):
        again = [f for f in first if f["walk"] > G2_STEPS or f["outside"] or f["parked2"] > g2_ovf(n_levels, wide_keys, True)]
    return len(first), len(again)


# ------------------------------------------------------------------------------------------------
# keys and layouts
# ------------------------------------------------------------------------------------------------
def zone(c: int) -> list:
    """the 6-letter range of cluster c: ascending in c, no two share their first three letters"""
    assert 0 <= c < 19 ** 3
    return [2 + c // 361, 2 + (c // 19) % 19, 2 + c % 19, 3, 3, 3]


def rep_of(c: int, K: int) -> list:
    return zone(c) + [10] * (K - 6)


def near(R: list, s: int, side: int, i: int) -> list:
    """the i-th key that shares exactly s >= 6 letters with R = ... 10 10 10, left (side 0) or right (1) of it"""
    K = len(R)
    assert RANGE_LETTERS <= s < K and R[s] == 10
    x, j = (9 - i % 10, i // 10) if side == 0 else (11 + i % 19, i // 19)
    tail = []
    for _ in range(K - s - 1):
        tail.append(j % 29)
        j //= 29
    assert j == 0, "no %d different keys share %d letters" % (i + 1, s)
    return R[:s] + [x] + tail[::-1]


def _counter(n: int, width: int) -> list:
    out = []
    for _ in range(width):
        out.append(n % 29)
        n //= 29
    assert n == 0
    return out[::-1]


class Layout:
    """Entries and queries of one case.  Queries are added in sorted order; pos = the sorted position of the next one."""

    def __init__(self, K: int):
        self.K, self.entries, self.q, self.count, self.taxon = K, [], [], 0, 0

    @property
    def pos(self) -> int:
        return len(self.q)

    def entry(self, letters, taxon=None):
        if taxon is None:
            self.taxon = self.taxon % (N_TAXA - 1) + 1
            taxon = self.taxon
        self.entries.append((pack(letters), taxon))

    def cluster(self, c: int, spec, fresh_taxa: bool = True) -> list:
        """the representative of cluster c and, per (s, side, count) of spec, `count` entries that share s letters with it,
        every entry under a taxon of its own"""
        R = rep_of(c, self.K)
        if fresh_taxa:
            self.taxon = 0
        self.entry(R)
        for s, side, count in spec:
            for i in range(count):
                self.entry(near(R, s, side, i))
        return R

    def add(self, letters, times: int = 1):
        k = pack(letters)
        assert not self.q or self.q[-1] <= k, "the layout is not in sorted order at %d" % self.pos
        self.q += [k] * times

    def filler(self, c: int, n: int):
        """n queries behind cluster c (c = -1: before cluster 0) that match nothing: they share its first three letters"""
        for _ in range(n):
            self.count += 1
            self.add((zone(c)[:3] if c >= 0 else [1, 1, 1]) + [25] + _counter(self.count, self.K - 4))

    def stretch(self, c: int, n: int, seventh: int = 20):
        """n queries inside the range of cluster c that share the range and nothing more"""
        for _ in range(n):
            self.count += 1
            self.add(zone(c) + [seventh] + _counter(self.count, self.K - 7))

    def pad_to(self, c: int, pos: int):
        assert pos >= self.pos, (pos, self.pos)
        self.filler(c, pos - self.pos)

    def case(self, name, family, windows, seed, score_windows=(), claim=None, never_coop=True, index=None):
        ix = lc._index(self.entries, self.K > 12, N_TAXA)
        base = lc._shuffled(name, family, index or name, ix, self.q, seed, windows, score_windows)
        return Case(**{f: getattr(base, f) for f in ("name", "family", "index", "ix", "q", "payload", "n_reads", "windows", "score_windows", "runs")},
                    claim=claim or {}, never_coop=never_coop)


@dataclass
class Case(lc.Case):
    claim: dict = field(default_factory=dict)      # what the family says of the case; tests/test_group_corpus_cpu.py holds it to that
    never_coop: bool = True                        # the route "never COOP" (debug flag 131072) applies: no list of 255 or more segments
    large: bool = False                            # records are compared, the float replay on the CPU is left out


def _w(K: int) -> int:
    return 64 if K == 12 else 128


def _walk_spec(K: int, n: int, mode: str):
    """n entries beyond the representative: the nearest share K - 1 letters with it, the others K - 2"""
    nl = {"left": n, "right": 0, "both": n // 2}[mode]
    nr = n - nl
    return [(K - 1, 0, min(nl, 10)), (K - 2, 0, max(nl - 10, 0)), (K - 1, 1, min(nr, 19)), (K - 2, 1, max(nr - 19, 0))]


# ---- walk ---------------------------------------------------------------------------------------
WALK_N = [0, 1, 3, 4, 5, 7, 8, 9, 39, 40, 41, 47, 48, 49, 63, 64, 65, 127, 128, 129, 200]
WALK_MODES = ("left", "right", "both")


def walk_case(K: int, mode: str) -> Case:
    """Tile t holds the lists of WALK_N[t] entries: two leaders in its first wavefront, one in its last.  "right": the longest
    list first, its representative entry 0; "left": the longest list last, its representative the last entry."""
    lay = Layout(K)
    ns = sorted(WALK_N, reverse=(mode == "right"))
    c = 0
    for t, n in enumerate(ns):
        for at in (0, 1, TILE - 3):
            lay.pad_to(c - 1, t * TILE + at)
            lay.add(lay.cluster(c, _walk_spec(K, n, mode)))
            c += 1
    lay.filler(c - 1, 5)
    return lay.case("walk%d %s" % (_w(K), mode), "walk", WINDOWS[K], 1000 + K, WINDOWS[K][:1] if mode == "both" else (),
                    claim={"walks": ns, "mode": mode})


def walk_whole_case(K: int, n_left: int, n_right: int) -> Case:
    """the list is the whole index: it reaches entry 0 and the last entry, where coop_walk's chunk loads clamp"""
    lay = Layout(K)
    R = lay.cluster(0, [(K - 1, 0, min(n_left, 10)), (K - 2, 0, max(n_left - 10, 0)), (K - 1, 1, min(n_right, 19)), (K - 2, 1, max(n_right - 19, 0))])
    lay.add(R)
    lay.add(near(R, K - 1, 1, 0))
    lay.filler(0, 3)
    return lay.case("walk%d whole %d+%d" % (_w(K), n_left, n_right), "walk", WINDOWS[K][:1] + WINDOWS[K][-2:], 1100 + K,
                    claim={"whole": (n_left, n_right)})


WALK_WHOLE = [(63, 66), (64, 64), (65, 63), (0, 129), (129, 0), (2, 0)]


# ---- count --------------------------------------------------------------------------------------
COUNT_LISTS = [254, 255, 256, 300]                 # segments of a list
COUNT_LEVEL = [6, 7, 8, 255, 256]                  # taxa of the shallowest level of a list whose other levels hold one


def count_case(K: int, which: str) -> Case:
    """a tile per list.  lists: COUNT_LISTS segments under distinct taxa.  level: the representative alone matches deeper than
    7 letters, COUNT_LEVEL - 1 entries share exactly 7.  inl: INL and INL + 1 segments of both record widths."""
    lay = Layout(K)
    if which == "lists":
        specs = [_walk_spec(K, n - 1, "both") for n in COUNT_LISTS]
    elif which == "level":
        specs = [[(7, 0, (m - 1) // 2), (7, 1, m - 1 - (m - 1) // 2)] for m in COUNT_LEVEL]
    else:
        specs = [_walk_spec(K, n - 1, "both") for n in (INL[8], INL[8] + 1, INL[16], INL[16] + 1)]
    for t, spec in enumerate(specs):
        if t:
            lay.pad_to(t - 1, t * TILE + 5)
        R = lay.cluster(t, spec)
        lay.add(R, 2)
        if which == "level":
            lay.add(near(R, 7, 1, 0))
    lay.filler(len(specs) - 1, 3)
    long_lists = which != "inl"
    return lay.case("count%d %s" % (_w(K), which), "count", WINDOWS[K], 1200 + K, WINDOWS[K][:1] if which == "level" else (),
                    claim={"which": which}, never_coop=not long_lists)


# ---- split --------------------------------------------------------------------------------------
def _prefix_queries(lay: Layout, entries: list, step: int = 1):
    """per entry e and length c: e's first c letters and then letters no entry has (21s: behind e's subtree; 0s: before it, so
    that a query matched to c letters follows one matched deeper that shares fewer than c with it; a '^') -- sorted before
    they are added"""
    K, qs = lay.K, set()
    for e in entries:
        qs.add(tuple(e))
        for c in range(RANGE_LETTERS, K, step):
            qs.add(tuple(e[:c] + [21] * (K - c)))
            qs.add(tuple(e[:c] + [0] * (K - c)))
            qs.add(tuple(e[:c] + [HAT] + [21] * (K - c - 1)))
            if c + 2 <= K:
                qs.add(tuple(e[:c] + [e[c]] + [HAT] + [21] * (K - c - 2)))
    for q in sorted(qs):
        lay.add(list(q), 2 if q[-1] == 21 else 1)


def split_case(K: int) -> Case:
    """Per u = 5 .. K - 1 two entries A_u < B_u of one taxon that share u letters with each other and with R: B_u has dup = u.  A
    query at B_u takes A_u as (t, kLow .. u) and B_u as (t, u + 1 .. d): the taxon owns two segments.  A query at R meets B_u
    with kLast = u = dup: no segment.  Where d = dup of the representative itself, the representative yields none.  R's key is
    in the index under three taxa."""
    lay = Layout(K)
    R = rep_of(1, K)
    for t in (200, 201, 202):
        lay.entry(R, t)
    ents = [R]
    for u in range(5, K):
        A, B = R[:u] + [8] + [5] * (K - u - 1), R[:u] + [9] + [5] * (K - u - 1)
        lay.entry(A, 1 + u)
        lay.entry(B, 1 + u)
        ents += [A, B]
    lay.entry(rep_of(0, K), 203)
    lay.entry(rep_of(3, K), 203)
    _prefix_queries(lay, ents, 1 if K == 12 else 3)
    return lay.case("split%d" % _w(K), "split", WINDOWS[K], 1300 + K, WINDOWS[K], claim={})


# ---- order --------------------------------------------------------------------------------------
def order_case(K: int) -> Case:
    """two entries per shared length 6 .. K - 1 and side, and every prefix of every entry as a query"""
    lay = Layout(K)
    R = rep_of(0, K)
    lay.entry(R)
    ents = [R]
    for s in range(RANGE_LETTERS, K):
        for side in (0, 1):
            for i in (0, 1):
                e = near(R, s, side, i)
                lay.entry(e)
                ents.append(e)
    _prefix_queries(lay, ents, 1 if K == 12 else 2)
    return lay.case("order%d" % _w(K), "order", WINDOWS[K], 1400 + K, WINDOWS[K], claim={})


# ---- flush --------------------------------------------------------------------------------------
FLUSH_PLACES = {"lane pair": (10, 11), "later lane": (20, 31), "next wavefront": (127, 128), "wavefront behind": (140, 700),
                "next tile": (1023, 1024), "tile behind": (1100, 3 * TILE + 7), "nowhere": (3 * TILE + 20, None)}


def flush_case(K: int) -> Case:
    """Per place a cluster {R, E = R's range with 27 as its seventh letter}: the query R at the first position, stretch queries,
    the query E -- which opens new groups of every level above 6 -- at the second.  The last leader's groups stay open to the
    end of the batch."""
    lay = Layout(K)
    for c, (name, (p, closer)) in enumerate(FLUSH_PLACES.items()):
        lay.pad_to(c - 1, p)
        R = lay.cluster(c, [(K - 1, 0, 1)])
        E = zone(c) + [27] + [10] * (K - 7)
        lay.entry(E)
        lay.add(R)
        if closer is None:
            lay.stretch(c, 40)
        else:
            lay.stretch(c, closer - lay.pos)
            lay.add(E)
    return lay.case("flush%d" % _w(K), "flush", WINDOWS[K], 1500 + K, WINDOWS[K][:1], claim={"places": dict(FLUSH_PLACES)})


# ---- followers, hits ----------------------------------------------------------------------------
FOLLOWER_RUNS = [1, 2, 3, 64, 127, 128, 129, 1025]
HIT_GROUPS = [1, 128, 129, 1024, 1025]
HITS_LARGE = 70000


def runs_case(K: int, family: str, runs: list, phase: int, list_len: int, name=None, windows=None) -> Case:
    """Per run a cluster with a list of `list_len` entries left of R (longer than INL: the run's leader owns a pool block), the
    query R `run` times, and R's first c letters before a '^' for some c: the same representative at another depth."""
    lay = Layout(K)
    lay.add([1] * K, phase)
    for c, run in enumerate(runs):
        R = lay.cluster(c, [(K - 1, 0, min(list_len, 10)), (K - 2, 0, max(list_len - 10, 0))])
        lay.add(R, run)
        if family == "followers":
            for cut in (K - 1, 9, 8, 7):
                lay.add(R[:cut] + [HAT] + [21] * (K - cut - 1), 2)
    windows = windows or WINDOWS[K]
    return lay.case(name or "%s%d phase %d" % (family, _w(K), phase), family, windows, 1600 + K + phase, windows[:1] if phase == 0 else (),
                    claim={"runs": runs, "phase": phase})


# ---- span ---------------------------------------------------------------------------------------
def span_case(K: int, limit: int, delta: int, walk: int = 8) -> Case:
    """One tile whose first and last representative lie limit + delta - 2 * GMARGIN - 1 entries apart: a cluster with a list of
    `walk` entries on its left at the front, entries of other ranges that no query meets, a cluster with a list of `walk`
    entries on its right at the end; GMARGIN + 4 entries more on either side, so that no margin is cut."""
    lay = Layout(K)
    apart = limit + delta - 2 * GMARGIN - 1
    for i in range(GMARGIN + 4):
        lay.entry([1, 1, 1] + _counter(i, K - 3), 250)
    A = lay.cluster(0, [(K - 1, 0, min(walk, 10)), (K - 2, 0, max(walk - 10, 0))])
    inner = apart - 1
    for i in range(inner):
        lay.entry(zone(1)[:3] + [1 + i // 600] + _counter(i % 600, 2) + [7] * (K - 6), 251)
    B = lay.cluster(2, [(K - 1, 1, min(walk, 19)), (K - 2, 1, max(walk - 19, 0))], fresh_taxa=False)
    for i in range(GMARGIN + 4):
        lay.entry([25, 1, 1] + _counter(i, K - 3), 252)
    lay.add(A, 2)
    lay.filler(0, 500)
    lay.add(B, 3)
    lay.filler(2, 4)
    windows = WINDOWS[K][:1] + WINDOWS[K][-2:]
    return lay.case("span%d %d%+d walk %d" % (_w(K), limit, delta, walk), "span", windows, 1700 + K, windows[:1] if (delta, walk) in ((1, 8), (2, 96)) else (),
                    claim={"span": limit + delta, "walk": walk})


SPANS = [(G2_SPAN, -1, 8), (G2_SPAN, 0, 8), (G2_SPAN, 1, 8), (G2_SPAN, 50, 40), (G2_SPAN, 60, 40), (GSPAN, -1, 8), (GSPAN, 0, 8), (GSPAN, 1, 8),
         (GSPAN, 2, 95), (GSPAN, 2, 96), (GSPAN, 2, 97)]


# ---- park ---------------------------------------------------------------------------------------
PARK_EDGES = [1023, 1024, 1025, 511, 512, 513, 4095, 4096, 4097]
PARK_ORDINARY_TILES = 4                           # tiles without lists behind the one that parks: the second launch runs


def _park_plan(total: int, rule: str):
    """leaders of G2_STEPS-entry lists (41 segments) and one shorter list that together park `total` segments"""
    per = G2_STEPS + 1 - (4 if rule == "g2" else 3)
    n_full, rest = divmod(total, per)
    if rest == 0:
        n_full, rest = n_full - 1, per
    return n_full, rest + (4 if rule == "g2" else 3)       # (lists of 41 segments, segments of the last list)


def park_case(K: int, total: int, rule: str) -> Case:
    """One tile.  A cluster of G2_STEPS entries left of R gives up to six leaders of 41 segments: the query R and, per depth
    c = 11 .. 7, R's first c letters before a '^' -- the same representative at another depth, the same 41 entries.  rule "g2": the total as group2_kernel counts it; "g": as group_kernel does."""
    lay = Layout(K)
    n_full, last = _park_plan(total, rule)
    per_cluster = 6
    c = 0
    while n_full > 0:
        R = lay.cluster(c, _walk_spec(K, G2_STEPS, "left"))
        take = min(per_cluster, n_full)
        lay.add(R)
        for cut in range(11, 11 - (take - 1), -1):
            lay.add(R[:cut] + [HAT] + [21] * (K - cut - 1))
        n_full -= take
        c += 1
    R = lay.cluster(c, _walk_spec(K, last - 1, "left"))
    lay.add(R)
    assert lay.pos <= TILE
    lay.filler(c, (1 + PARK_ORDINARY_TILES) * TILE - lay.pos + 3)
    return lay.case("park%d %s %d" % (_w(K), rule, total), "park", [(12, 7)] + ([(12, 5)] if K == 12 else []), 1800 + K + total, [(12, 7)] if total in (1025, 4097) else (),
                    claim={"total": total, "rule": rule})


# ---- pool ---------------------------------------------------------------------------------------
POOL_LEADERS, POOL_LIST = 300, 250


def pool_case(K: int) -> Case:
    """POOL_LEADERS wavefronts of one repeated query whose list has POOL_LIST segments: every wavefront's first query leads, and
    their blocks together outgrow the pool a batch of fewer than 65 536 queries begins with"""
    lay = Layout(K)
    R = lay.cluster(0, _walk_spec(K, POOL_LIST - 1, "both"))
    lay.add(R, POOL_LEADERS * WAVE)
    return lay.case("pool%d" % _w(K), "pool", WINDOWS[K][:1], 1900 + K, WINDOWS[K][:1], claim={}, never_coop=True)


# ---- ends ---------------------------------------------------------------------------------------
ENDS = [(1, 1), (1, 2), (2, 127), (3, 128), (3, 129), (301, 2), (301, 1023), (301, 1024), (301, 1025), (301, 2049)]     # (index entries, batch)


def ends_case(K: int, n: int, batch: int) -> Case:
    base = lc.ends_case(K, n, batch)
    c = Case(**{f: getattr(base, f) for f in ("name", "family", "index", "ix", "q", "payload", "n_reads", "windows", "score_windows", "runs")},
             claim={"n": n, "batch": batch})
    if batch in (129, 2049):
        c.score_windows = list(c.windows)
    return c


def nothing_case(K: int) -> Case:
    lay = Layout(K)
    lay.cluster(0, [(K - 1, 0, 3)])
    lay.filler(1, 1500)
    return lay.case("ends%d nothing matches" % _w(K), "ends", WINDOWS[K][:2], 2000 + K, claim={})


def lookup_family_case(name: str) -> Case:
    base = lc.case(name)
    return Case(**{f: getattr(base, f) for f in ("name", "family", "index", "ix", "q", "payload", "n_reads", "windows", "score_windows", "runs")},
                claim={}, never_coop=True)


LOOKUP_CASES = ["main64", "main64+filler", "main128", "open6", "open6 edges"]


# ---- the list -----------------------------------------------------------------------------------
def _builders():
    b = {}
    for K in (12, 25):
        w = _w(K)
        for mode in WALK_MODES:
            b["walk%d %s" % (w, mode)] = functools.partial(walk_case, K, mode)
        for nl, nr in WALK_WHOLE:
            b["walk%d whole %d+%d" % (w, nl, nr)] = functools.partial(walk_whole_case, K, nl, nr)
        for which in ("lists", "level", "inl"):
            b["count%d %s" % (w, which)] = functools.partial(count_case, K, which)
        b["split%d" % w] = functools.partial(split_case, K)
        b["order%d" % w] = functools.partial(order_case, K)
        b["flush%d" % w] = functools.partial(flush_case, K)
        for phase in (0, 1):
            b["followers%d phase %d" % (w, phase)] = functools.partial(runs_case, K, "followers", FOLLOWER_RUNS, phase, 6 if K == 12 else 10)
        b["hits%d phase 0" % w] = functools.partial(runs_case, K, "hits", HIT_GROUPS, 0, 2)
        for limit, delta, walk in SPANS:
            b["span%d %d%+d walk %d" % (w, limit, delta, walk)] = functools.partial(span_case, K, limit, delta, walk)
        for total in PARK_EDGES:
            b["park%d g2 %d" % (w, total)] = functools.partial(park_case, K, total, "g2")
        for total in PARK_EDGES[:3]:
            b["park%d g %d" % (w, total)] = functools.partial(park_case, K, total, "g")
        b["pool%d" % w] = functools.partial(pool_case, K)
        for n, batch in ENDS:
            b["ends%d n%d b%d" % (w, n, batch)] = functools.partial(ends_case, K, n, batch)
        b["ends%d nothing matches" % w] = functools.partial(nothing_case, K)
    b[LARGE] = functools.partial(runs_case, 12, "hits", [HITS_LARGE], 1, 2, LARGE, WINDOWS[12][:1])
    for name in LOOKUP_CASES:
        b[name] = functools.partial(lookup_family_case, name)
    return b


LARGE = "hits64 70000"
_BUILDERS = _builders()


def case_names(large: bool = True, family=None) -> list:
    return [n for n in _BUILDERS if (large or n != LARGE) and (family is None or n.startswith(family))]


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    c = _BUILDERS[name]()
    if name == LARGE:
        c.large = True
    return c


@functools.lru_cache(maxsize=None)
def ref(name: str, k_high: int, k_low: int) -> list:
    """the reference of a case under a window, computed once and left unchanged"""
    return reference(case(name), k_high, k_low)
