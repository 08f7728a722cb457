"""Hand-made reads for the score stage (kasa_batch_score: score_main_kernel, the score_other* family, the row merges,
score_dense_kernel, score_kernel and its later passes, the sorted-event replay, the staging retry), with the plain replay of
tests/group_corpus.py as the reference and a plain restatement of what score_main_kernel decides per read -- the two register
taxa, the staging row's length, the reason a read is handed on -- so that a case can say "this read's row has 1025 records".
The inputs of tests/test_score_corpus_cpu.py (every family's claim from the reference alone, the replay against the sequential
oracle, order sensitivity) and tests/test_gpu_score_corpus.py (the device under every route of score_stage, fed the
reference's own records through kasa_batch_records_import).  Pure numpy and tests/group_corpus.py: no device, no reference tree.

A case is a group_corpus.Layout world -- clusters, stretch queries and fillers in sorted order -- plus a READ PLAN: the read of
every sorted position.  Reads are numbered along the sorted order unless a family says otherwise, so a read's first slot (the
device files a read's records by read, each read's in sorted order) is the sorted position of its first query; n_reads may
exceed the reads that own a query.  group_corpus.reference gives the event records, group_corpus.encode their device layout,
group_corpus.replay the scores.

Families (the names of DESIGN 8m):
  take       batches of 1, 63, 64, 65, 127, 128, 129 reads with reads without a query at the start, around a matched read in the
             middle and at the end; a batch whose last 64 reads are empty
  phase      reads of 1 .. 9 queries that begin 0 .. 3 records into a 128-byte line, the matched query as the read's first and
             last record and as the last record of its first line and the first of its last
  slots      a read that ends at slot 63, begins at 64, straddles 127 | 128, spans four 64-slot windows (200 queries); 200 reads
             of one query around one of 1000; 64-slot windows whose items total 63, 64, 65, 128, 129, 131
  registers  reads with 0, 1, 2, 3+ taxa at kPromote or deeper; the deepest match kPromote - 1 and kPromote; REC_SPLIT in the
             first deep query; the second register taxon in a later query, in the pool part of a list (plain, REC_SAT, 255 or
             more segments); a register taxon that comes back shallow; shallow matches only
  order      group_corpus's order and split worlds cut into reads of 2 .. 8 matched queries, consecutive and alternating between
             two reads, EVERY one of which changes its bits when replayed query by query: F rising, falling and tied, closers in
             the same read, another one, nowhere; the same worlds with every query its own read, and a kept read whose other
             taxa's sums depend on the order inside one query
  sizes      |T_k| of 1 .. 8, 63 .. 65, 254 .. 256 (and 8190 .. 8192 on an index of 8200 taxa); reads of 255 and of 256 distinct
             matched queries (the batch's counter fields go from 8 to 16 bits); 64-byte records: reads of 60 000 and 60 001 queries
  rule       Fmax == p of the read's next matched query (kept) and p + 1 (handed on), the breaking query second and last; the
             same inside reads whose rows exceed RMAX
  rows       rows of 255 .. 257, 511 .. 513, 1023 .. 1025 records; reads of 255 and 256 queries with rows of 2047 .. 2049;
             batches of 1000 reads that need 65 535, 65 536, 65 537 staging records, and (64-byte records) as many profile keys
  taxa       one small batch under content tables of 2048, 2049, 4096, 4097, 8140, 8141, 16 384, 16 385 rows, the highest taxon
             among those with k-mers
  dense      reads handed on for a long row with lists of 1, 3, 4, 5, 63, 64, 65, 128, 129, 192, 193, 256, 300 segments; a REC_SPLIT
             query with one taxon in two chunks and REC_SAT sizes on an odd and an even level; reads of 1, 2, 3 queries; 1, 3, 4,
             5 handed reads
  general    reads that touch 255, 256, 257 taxa; queries of 1023, 1024, 1025 segments
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from tests import group_corpus as gc, lookup_corpus as lc

# ------------------------------------------------------------------------------------------------
# the kernels' constants, by the names they have in kasa_hip.hip and kasa_replay.h (tests/test_score_corpus_cpu.py reads them
# out of the files)
# ------------------------------------------------------------------------------------------------
FTA = 2                           # taxa score_main_kernel keeps in registers
RMAX = 1024                       # longest staging row of a read of fewer than 256 queries
ROW_PER_QUERY = 8                 # A.rowPerQuery: a read of cnt queries may have a row of max(RMAX, 8 cnt) records where 8 cnt >= 2 RMAX ...
ROW_PER_QUERY_TAXA = 4096         # ... up to this many content rows, and with the bitmap merge
CLS_LO = (256, 512, 1024)         # R.clsLo: a row longer than these belongs to the second, third, long class (512 -> 256 beyond 2048 taxa)
NARROW_BITMAP_TAXA = 2048
EV_INV = 64
TLIST = 256
AGG = 256
PCAP_SMALL = 96
DENSE_TAXA = 16384
DQ_SEGS = 1024
SD_WAVES = 4
BM_WORDS = 512
DENSE_LDS = 160 * 1024 - 1024     # score_stage: nTaxa * 5 * SD_WAVES bytes must fit
ESR_MIN_KMERS = 16384             # kasa_replay.h
NSEG_BITS = 13                    # a list of 1 << 13 segments or more: why[3]
CNT_MAX = {8: 255, 16: 60000}     # counter fields of FB bits: a read of more queries is handed on (why[0])
CNT_FIELDS = {8: 4, 16: 2}        # by record words: |T| up to which a register taxon's events are counted in LDS
LN = {8: 4, 16: 2}                # records of a 128-byte line, by record words
TAKE = 64                         # reads a wavefront of score_main_kernel takes per turn; slots of a window of the score_other* family
FIRST_STAGING = 1 << 16           # c->stCap of a fresh context: max(this, 8 per read)
WHY = ("k-mer count", "taxa", "row length", "segments", "order rule")

HAT = lc.HAT
W12 = [(12, 7), (12, 5), (12, 11), (12, 12), (12, 3)]      # the last one: 64-byte records on 64-bit keys
W25 = [(25, 7), (25, 5)]


def windows(K: int, *which) -> list:
    """the windows of a key width; which: indices into them (a window named twice is taken once)"""
    w = W12 if K == 12 else W25
    return list(w) if not which else list(dict.fromkeys(w[i] for i in which))


def k_promote(kh: int, kl: int) -> int:
    return kl + 2 if kh - kl + 1 >= 3 else kl


# ------------------------------------------------------------------------------------------------
# a layout with a read plan
# ------------------------------------------------------------------------------------------------
@dataclass
class Case(gc.Case):
    built_for: str = ""                            # the route the case is built for, in words


class Plan(gc.Layout):
    """group_corpus.Layout + the read of every query: queries go to read `self.read`; clusters are numbered as they are made"""

    def __init__(self, K: int, n_taxa: int = gc.N_TAXA, taxmap=None):
        super().__init__(K)
        self.reads, self.read, self.c, self.n_taxa, self.taxmap = [], 0, 0, n_taxa, taxmap

    def entry(self, letters, taxon=None):
        if taxon is None:
            self.taxon = self.taxon % (self.n_taxa - 1) + 1
            taxon = self.taxon
        self.entries.append((gc.pack(letters), self.taxmap(taxon) if self.taxmap else taxon))

    def add(self, letters, times: int = 1):
        super().add(letters, times)
        self.reads += [self.read] * times

    def next_read(self) -> int:
        self.read += 1
        return self.read

    def hit(self, spec=(), before: int = 0, after: int = 0, fresh: bool = True, times: int = 1, cut: int = None, custom=None):
        """A new cluster and one query of the current read matched in it, with `before` and `after` queries of the same read that
        share the cluster's range and nothing more around it.  spec: (s, side, count) entries that share s letters with the
        representative R, every one under a taxon of its own (R: 1, then 2, 3, ... -- fresh: counted from 1 for this cluster).
        cut: the query is R's first `cut` letters before a '^' (matched to depth cut); times: the query that often.
        custom(R): further entries, added by hand.  -> the sorted position of the (first) matched query"""
        c = self.c
        self.c += 1
        if before:
            self.stretch(c, before, seventh=1)
        R = self.cluster(c, spec, fresh)
        if custom:
            custom(R)
        at = self.pos
        self.add(R if cut is None else R[:cut] + [HAT] + [21] * (self.K - cut - 1), times)
        if after:
            self.stretch(c, after)
        return at

    def unmatched(self, n: int):
        """n queries of the current read in a range of their own, whose one entry they share six letters with"""
        if n:
            c = self.c
            self.c += 1
            self.cluster(c, ())
            self.stretch(c, n)

    def finish(self, name, family, wins, seed, n_reads=None, claim=None, built_for="", index=None, never_coop=True) -> Case:
        ix = lc._index(self.entries, self.K > 12, self.n_taxa)
        n_reads = max(self.reads) + 1 if n_reads is None else n_reads
        base = lc._shuffled(name, family, index or name, ix, self.q, seed, wins, wins, payload=self.reads, n_reads=n_reads)
        c = Case(**{f: getattr(base, f) for f in ("name", "family", "index", "ix", "q", "payload", "n_reads", "windows", "score_windows", "runs")},
                 claim=claim or {}, never_coop=never_coop, built_for=built_for)
        # (equal keys of different reads would make the read of a sorted position depend on the shuffle)
        assert c.sorted[1].tolist() == self.reads, name
        return c


def replan(base: gc.Case, name: str, family: str, reads: list, wins, seed: int, claim=None, built_for="") -> Case:
    """a world of group_corpus under a read plan: reads[p] = the read of sorted position p"""
    qs = base.sorted[0]
    n_reads = max(reads) + 1
    b = lc._shuffled(name, family, base.index, base.ix, qs, seed, wins, wins, payload=reads, n_reads=n_reads)
    c = Case(**{f: getattr(b, f) for f in ("name", "family", "index", "ix", "q", "payload", "n_reads", "windows", "score_windows", "runs")},
             claim=claim or {}, never_coop=base.never_coop, built_for=built_for)
    return c


def others(K: int, m: int, s: int = None) -> list:
    """m entries right of the representative, each under a taxon of its own: the nearest 19 share K - 1 letters (s: that many) with
    it, the others one fewer"""
    s = K - 1 if s is None else s
    return [(s, 1, min(m, 19)), (s - 1, 1, max(m - 19, 0))] if m else []


# ------------------------------------------------------------------------------------------------
# what score_main_kernel decides per read, restated from the reference's records
# ------------------------------------------------------------------------------------------------
@dataclass
class ReadFacts:
    read: int
    first_slot: int              # kmerOff[read]
    n: int                       # queries
    positions: list              # sorted positions of its queries, ascending: the order of its slots
    regs: tuple = ()             # the register taxa, in the order they were found
    row: int = 0                 # records of the staging row score_main_kernel asks for (0: no match, or handed on)
    why: int = None              # index into WHY of the reason it is handed on, None: kept
    keeps_rule: bool = True      # every matched query lies at or behind the Fmax of the one before: score_dense_kernel keeps it
    items: list = None           # kept reads: work items of score_other_flat_kernel (64-byte records: of score_other_flat16_kernel's second sweep) per query
    taxa: int = 0                # distinct taxa of its segments (the cells of its score row)
    need: int = None             # records its row would have without a cap (None: the order rule or a list of 8192 segments ends the count)
    keys: int = 0                # kept reads, 64-byte records: profile keys of its row (one per counter field in use and per event of the others)
    n_other: int = 0             # kept reads: records of the other taxa (score_other*'s share of the row)

    def phase(self, rw: int) -> int:
        return self.first_slot % LN[rw]


def seg_records(rw: int, levels: int, split: bool) -> int:
    return (1 if levels else 0) if (rw == 8 and levels <= 2 and not split) else levels


def register_taxa(recs: list, kh: int, kl: int, rw: int) -> tuple:
    """part A of score_main_kernel: the first two taxa with a segment that reaches kPromote, query by query; a query's segments
    in list order, those in the pool only while they reach kPromote and only when the last inline one does"""
    kp, inl, regs = k_promote(kh, kl), gc.INL[rw], []
    for r in recs:
        if len(regs) >= FTA:
            break
        if r.d < kp:
            continue
        n = len(r.segs)
        n_inl = n if n <= inl else inl - 1
        for t, _, k_last in r.segs[:n_inl]:
            if k_last >= kp and len(regs) < FTA and (not regs or t != regs[0]):
                regs.append(t)
        if n > inl and len(regs) < FTA and r.segs[inl - 2][2] >= kp:
            for t, _, k_last in r.segs[inl - 1:]:
                if len(regs) >= FTA or k_last < kp:
                    break
                if not regs or t != regs[0]:
                    regs.append(t)
    return tuple(regs)


def row_cap(n_queries: int, n_taxa: int, sorting_merge: bool = False) -> int:
    rpq = ROW_PER_QUERY if (n_taxa <= ROW_PER_QUERY_TAXA and not sorting_merge) else 0
    return rpq * n_queries if rpq * n_queries >= 2 * RMAX else RMAX


def read_facts(case, recs: list, kh: int, kl: int, sorting_merge: bool = False) -> list:
    """One ReadFacts per read, by the steps of score_main_kernel<.., PERREAD = true>: too many queries for the counter fields;
    then query by query the order rule, the segment count, the row so far against the cap; at the end the whole row."""
    rw = gc.rec_words(kh, kl)
    rd = np.asarray(case.sorted[1], dtype=np.int64)
    counts = np.bincount(rd, minlength=case.n_reads)
    first = np.concatenate(([0], np.cumsum(counts)[:-1]))
    by_read = np.argsort(rd, kind="stable")
    fb16 = int(counts.max(initial=0)) > 255
    n_taxa = case.ix.content.n_taxa
    out = []
    for r in range(case.n_reads):
        pos = by_read[first[r]:first[r] + counts[r]].tolist()
        f = ReadFacts(r, int(first[r]), int(counts[r]), pos)
        mine = [recs[p] for p in pos]
        f.taxa = len({t for q in mine for t, _, _ in q.segs})
        prev = 0
        for q in mine:
            if q.d:
                if prev > q.p:
                    f.keeps_rule = False
                prev = q.fmax
        if f.n > (CNT_MAX[16] if fb16 else CNT_MAX[8]):
            f.why = 0
            out.append(f)
            continue
        f.regs = register_taxa(mine, kh, kl, rw)
        cap, n_other, n_keys, prev, fields, f.items, over, stop = row_cap(f.n, n_taxa, sorting_merge), 0, 0, 0, set(), [], False, None
        for q in mine:
            if not q.d:
                f.items.append(0)
                continue
            if prev > q.p:
                stop = 4
                break
            prev = q.fmax
            if len(q.segs) >= (1 << NSEG_BITS):
                stop = 3
                break
            inl = gc.INL[rw]
            n_inl = len(q.segs) if len(q.segs) <= inl else inl - 1
            levels = {t: set() for t in f.regs}
            items, recs_q, reg_big = len(q.segs) - n_inl, 0, 0
            for i, (t, kf, k_last) in enumerate(q.segs):
                if t in levels:
                    levels[t] |= set(range(kh - k_last, kh - kf + 1))
                    if rw == 16:                            # (64-byte records: a register taxon's segment is an item where a level of it has |T| > CNT_FIELDS)
                        big = sum(1 for lv in range(kh - k_last, kh - kf + 1) if q.sizes[lv] > CNT_FIELDS[16])
                        reg_big += big
                        items += i < n_inl and big > 0
                else:
                    recs_q += seg_records(rw, k_last - kf + 1, q.split)
                    n_keys += k_last - kf + 1
                    items += i < n_inl
            n_other += recs_q
            f.items.append((1 if recs_q + reg_big else 0) if q.split else items)
            over = over or n_other > cap                    # (the kernel stops here: why[2]; counted on for `need`)
            if rw == 16:                                    # a register taxon's events: counted per (level, |T|) up to CNT_FIELDS, a record each beyond
                for e, t in enumerate(f.regs):
                    for lv in levels[t]:
                        if q.sizes[lv] <= CNT_FIELDS[16]:
                            fields.add((e, lv, q.sizes[lv]))
                        else:
                            n_other += 1
                            n_keys += 1
        m = len(f.regs) + len(fields) + n_other
        if over or (stop is None and m > cap):
            f.why = 2
        elif stop is not None:
            f.why = stop
        if stop is None:
            f.need = m
        if f.why is None:
            f.row, f.n_other = m, n_other
            f.keys = len(fields) + n_keys if rw == 16 else 0
        else:
            f.items = None
        out.append(f)
    return out


def why_counts(facts: list) -> tuple:
    return tuple(sum(1 for f in facts if f.why == k) for k in range(5))


def dense_runs(case, kh: int, kl: int, flags: int) -> bool:
    """score_stage hands the fast kernels' leftovers to score_dense_kernel: narrow records, the rows of SD_WAVES reads in LDS"""
    return gc.rec_words(kh, kl) == 8 and case.ix.content.n_taxa * 5 * SD_WAVES <= DENSE_LDS and not (flags & 33554432) and not (flags & 1)


def row_classes(facts: list, n_taxa: int) -> tuple:
    """kasa_ctx_row_classes after the fast kernels under the bitmap merge: (first, second, third, long)"""
    second_hi = CLS_LO[1] if n_taxa <= NARROW_BITMAP_TAXA else CLS_LO[0]
    kept = [f.row for f in facts if f.why is None]
    second = sum(1 for m in kept if CLS_LO[0] < m <= second_hi)
    third = sum(1 for m in kept if second_hi < m <= CLS_LO[2])
    long_ = sum(1 for m in kept if m > CLS_LO[2])
    return (len(kept) - second - third - long_, second, third, long_)


def window_items(facts: list, n_queries: int, per_read: bool = False):
    """the items of every 64-slot window of score_other_flat_kernel / score_other_flat16_kernel's second sweep (a read without
    records of its own in the other taxa's part of the row has none); per_read: per window the (read, items) of the reads with
    items, in slot order"""
    per_slot, owner = [0] * n_queries, [None] * n_queries
    for f in facts:
        if f.why is None and f.n_other:
            per_slot[f.first_slot:f.first_slot + f.n] = f.items
            owner[f.first_slot:f.first_slot + f.n] = [f.read] * f.n
    if not per_read:
        return [sum(per_slot[s:s + TAKE]) for s in range(0, n_queries, TAKE)]
    out = []
    for s in range(0, n_queries, TAKE):
        w = []
        for x in range(s, min(s + TAKE, n_queries)):
            if per_slot[x]:
                if w and w[-1][0] == owner[x]:
                    w[-1] = (owner[x], w[-1][1] + per_slot[x])
                else:
                    w.append((owner[x], per_slot[x]))
        out.append(w)
    return out


def read_events(case, recs: list, read: int) -> list:
    """(F, k, p, taxa of T_k) of every event of a read"""
    rd = case.sorted[1]
    ev = []
    for r in recs:
        if r.d and rd[r.p] == read:
            for i, F in enumerate(r.F):
                k = r.d - len(r.F) + 1 + i
                ev.append((F, k, r.p, tuple(t for t, kf, kl_ in r.segs if kf <= k <= kl_)))
    return ev


def chain(events: list, by_position: bool) -> dict:
    """the float32 sums of a read's events per taxon, in flush order (F, k, p) or query by query (p, then the query's own
    flush order)"""
    M = {}
    for F, k, p, taxa in sorted(events, key=(lambda e: (e[2], e[0], e[1])) if by_position else (lambda e: (e[0], e[1], e[2]))):
        s = (np.float32(k * k) / np.float32(625)) * (np.float32(1) / np.float32(len(taxa)))
        for t in taxa:
            M[t] = np.float32(M.get(t, np.float32(0)) + s)
    return M


def chain_by_query(recs: list, positions: list, kh: int, level_order: bool) -> dict:
    """a kept read's sums as the fast kernels make them: query by query, a query's events in its record's order -- or
    (level_order) by level, k ascending, as a record with a wrong order field would have them"""
    M = {}
    for p in positions:
        r = recs[p]
        for lv in (sorted(r.order, reverse=True) if level_order else r.order):
            k = kh - lv
            taxa = [t for t, kf, kl_ in r.segs if kf <= k <= kl_]
            s = (np.float32(k * k) / np.float32(625)) * (np.float32(1) / np.float32(len(taxa)))
            for t in taxa:
                M[t] = np.float32(M.get(t, np.float32(0)) + s)
    return M


def within_query_sensitive(recs: list, f: ReadFacts, kh: int) -> bool:
    a, b = chain_by_query(recs, f.positions, kh, False), chain_by_query(recs, f.positions, kh, True)
    return any(a[t].view(np.uint32) != b[t].view(np.uint32) for t in a)


def order_sensitive(case, recs: list, read: int) -> bool:
    ev = read_events(case, recs, read)
    a, b = chain(ev, False), chain(ev, True)
    return any(a[t].view(np.uint32) != b[t].view(np.uint32) for t in a)


# ------------------------------------------------------------------------------------------------
# take
# ------------------------------------------------------------------------------------------------
TAKE_BATCHES = [1, 63, 64, 65, 127, 128, 129]


def take_case(K: int, n: int, tail: bool = False) -> Case:
    """n reads, each one matched query (two register taxa and one other) and one unmatched; without a query: read 0, the reads
    around the matched read n // 2, the last read -- or (tail) the last 64 reads"""
    lay = Plan(K)
    empty = set(range(n - TAKE, n)) if tail else ({0, n // 2 - 1, n // 2 + 1, n - 1} if n >= 63 else set())
    for r in range(n):
        if r not in empty:
            lay.read = r
            lay.hit(others(K, 2), after=1)
    return lay.finish("take%d %d%s" % (gc._w(K), n, " tail" if tail else ""), "take", windows(K), 3000 + K + n, n_reads=n,
                      claim={"reads": n, "empty": sorted(empty)}, built_for="score_main_kernel's turns of 64 reads")


# ------------------------------------------------------------------------------------------------
# phase
# ------------------------------------------------------------------------------------------------
PHASE_QUERIES = range(1, 10)


def phase_case(K: int) -> Case:
    """per phase 0 .. 3 and length n = 1 .. 9 reads whose one matched query is their first record, their last, the last of
    their first line and the first of their last line (lines of four records; of two: every second of these); a read of
    unmatched queries in front of each moves its first slot to the phase"""
    lay = Plan(K)
    plan = []
    for ph in range(4):
        for n in PHASE_QUERIES:
            for m in sorted({0, n - 1, 3 - ph, ((ph + n - 1) // 4) * 4 - ph} & set(range(n))):
                pad = (ph - lay.pos) % 4
                if pad:
                    lay.unmatched(pad)
                    lay.next_read()
                assert lay.pos % 4 == ph
                plan.append((lay.read, ph, n, m))
                lay.hit(others(K, 2), before=m, after=n - 1 - m)
                lay.next_read()
    return lay.finish("phase%d" % gc._w(K), "phase", windows(K), 3100 + K, n_reads=lay.read, claim={"plan": plan},
                      built_for="a lane's lines of LN records")


# ------------------------------------------------------------------------------------------------
# slots
# ------------------------------------------------------------------------------------------------
SLOT_UNEQUAL = (100, 1000, 100)               # reads of one query, queries of the long read, reads of one query
SLOT_ITEMS = [63, 64, 65, 128, 129, 131]      # items of the windows of slots_items_case
SLOT_LISTS = [1, 63, 64, 65, 130]             # items of one query


def slots_case(K: int) -> Case:
    lay = Plan(K)
    claim = {}
    sp = others(K, 3)
    claim["ends at 63"] = lay.read
    lay.hit(sp, after=31)
    lay.hit(sp, before=31)
    assert lay.pos == 64
    claim["begins at 64"] = lay.next_read()
    lay.hit(sp, after=9)
    lay.next_read()
    lay.unmatched(120 - lay.pos)
    claim["straddles 127 | 128"] = lay.next_read()
    assert lay.hit(sp, before=7) == 127
    assert lay.hit(sp, after=7) == 128
    claim["four windows"] = lay.next_read()
    for _ in range(5):
        lay.hit(sp, before=19, after=20)
    for i, n in enumerate(SLOT_UNEQUAL):
        if i == 1:
            claim["long"] = lay.next_read()
            for _ in range(n // 100):
                lay.hit(sp, before=49, after=50)
        else:
            for _ in range(n):
                lay.next_read()
                lay.hit(sp)
    return lay.finish("slots%d reads" % gc._w(K), "slots", windows(K), 3200 + K, claim=claim, built_for="read_of_slot, otherOff64")


def slots_items_case(K: int) -> Case:
    """Six windows of 64 slots.  A query with a list of m + 1 segments under distinct taxa, the first two the read's register
    taxa, is m - 1 items.  Window by window (items of its queries; | = a read boundary):  63  |  64  |  65  |  63 | 65  |
    64 | 64 | 1  |  130 | 1 -- a boundary at the first item of every window, in the middle of one, at the last item of one."""
    lay = Plan(K)
    for w, qs in enumerate([[63], [64], [65], [63, 65], [64, 64, 1], [130, 1]]):
        for x in qs:
            lay.hit(others(K, x + 1))
            lay.next_read()
        lay.read -= 1
        lay.unmatched((w + 1) * TAKE - lay.pos)
        lay.next_read()
    return lay.finish("slots%d items" % gc._w(K), "slots", windows(K), 3250 + K, n_reads=lay.read, claim={"items": SLOT_ITEMS, "lists": SLOT_LISTS},
                      built_for="ItemPlacer: 64 items per round", never_coop=True)


def slots_items_wide_case(K: int) -> Case:
    """The same six windows for 64-byte records, whose kernel deals out every segment of a query in which the register taxon meets
    a level of more than CNT_FIELDS taxa: a list of the representative and n - 1 entries that share seven letters with it is n
    items (n >= 3; one further entry: 1 item, the register taxon's segment stays behind), and a short row under every window."""
    lay = Plan(K)
    for w, qs in enumerate([[63], [64], [65], [63, 65], [64, 64, 1], [130, 1]]):
        for x in qs:
            lay.hit([(7, 1, x - 1 if x > 1 else 1)])
            lay.next_read()
        lay.unmatched((w + 1) * TAKE - lay.pos)        # (a read of their own: below seven letters they match, one group over many positions)
        lay.next_read()
    return lay.finish("slots%d items wide" % gc._w(K), "slots", windows(K) if K == 25 else windows(K, -1), 3260 + K, n_reads=lay.read,
                      claim={"items": SLOT_ITEMS, "lists": SLOT_LISTS}, built_for="ItemPlacer under score_other_flat16_kernel")


# ------------------------------------------------------------------------------------------------
# register taxa
# ------------------------------------------------------------------------------------------------
def _one_taxon_thrice(lay: Plan, more: int):
    """entries so that a query at R finds taxon 1 in its first three segments -- R at kHigh, an entry that shares K - 1 letters at
    K - 1, one that shares K - 2 from kLow to K - 2 (REC_SPLIT) --, taxon 2 at 9, taxon 3 at 8 and `more` further taxa at 7"""
    def custom(R):
        K = lay.K
        lay.entry(gc.near(R, K - 2, 0, 0), 1)
        lay.entry(gc.near(R, K - 1, 0, 0), 1)
        lay.entry(gc.near(R, 9, 1, 0), 2)
        lay.entry(gc.near(R, 8, 1, 0), 3)
        for i in range(more):
            lay.entry(gc.near(R, 7, 1, i), 4 + i)
    return custom


REGISTER_READS = ["none: depth kPromote - 1", "depth kPromote", "one taxon", "two taxa", "four taxa", "split first", "second in a later query",
                  "second in the pool", "second in the pool, REC_SAT", "second in the pool, 255 or more", "comes back shallow", "shallow only"]


def registers_case(K: int) -> Case:
    """one read per entry of REGISTER_READS, in that order; kPromote = 9 under the first window (K, 7)"""
    lay = Plan(K)
    kp = k_promote(K, 7)
    for label in REGISTER_READS:
        if label == "none: depth kPromote - 1":
            lay.hit(others(K, 2), cut=kp - 1, after=1)
        elif label == "depth kPromote":
            lay.hit(others(K, 2), cut=kp, before=1)
        elif label == "one taxon":
            lay.hit((), after=2)
        elif label == "two taxa":
            lay.hit(others(K, 1))
        elif label == "four taxa":
            lay.hit([(K - 1, 1, 1), (K - 2, 1, 1), (K - 3, 1, 1)], before=1, after=1)
        elif label == "split first":
            lay.hit([(K - 1, 1, 1), (K - 2, 1, 1)], custom=lambda R: (lay.entry(gc.near(R, K - 2, 0, 0), 1), lay.entry(gc.near(R, K - 1, 0, 0), 1)))
        elif label == "second in a later query":
            lay.hit((), after=3)
            lay.hit((), fresh=False)
        elif label == "second in the pool":
            lay.hit((), custom=_one_taxon_thrice(lay, 0), after=1)
        elif label == "second in the pool, REC_SAT":
            lay.hit((), custom=_one_taxon_thrice(lay, 7))
        elif label == "second in the pool, 255 or more":
            lay.hit((), custom=_one_taxon_thrice(lay, 260))
        elif label == "comes back shallow":
            lay.hit(others(K, 1), after=1)
            lay.hit(others(K, 2), cut=kp - 1)
        elif label == "shallow only":
            lay.hit(others(K, 3), cut=kp - 1)
            lay.hit(others(K, 2), cut=kp - 2, after=1)
        lay.next_read()
    return lay.finish("registers%d" % gc._w(K), "registers", windows(K), 3300 + K, n_reads=lay.read, claim={"reads": REGISTER_READS},
                      built_for="part A of score_main_kernel", never_coop=False)


# ------------------------------------------------------------------------------------------------
# order: worlds of group_corpus cut into reads
# ------------------------------------------------------------------------------------------------
ORDER_SIZES = range(2, 9)
ORDER_WORLDS = ("order", "split")


def events_at(recs: list, positions: list) -> list:
    """(F, k, p, taxa of T_k) of every event of the queries at these sorted positions"""
    ev = []
    for p in positions:
        r = recs[p]
        for i, F in enumerate(r.F):
            k = r.d - len(r.F) + 1 + i
            ev.append((F, k, p, tuple(t for t, kf, kl_ in r.segs if kf <= k <= kl_)))
    return ev


def _sensitive(recs: list, positions: list) -> bool:
    ev = events_at(recs, positions)
    a, b = chain(ev, False), chain(ev, True)
    return any(a[t].view(np.uint32) != b[t].view(np.uint32) for t in a)


def order_case(K: int, world: str, mode: str) -> Case:
    """The world's sorted queries cut into reads.  single: every query its own read -- the fast kernels keep them all, and the
    events of ONE query, in the record's order field, are what the sums depend on (within_query_sensitive).  chunks, pairs: the
    family's reads, of 2 .. 8 matched queries each (the unmatched ones between them go along) -- chunks: a read is a run of
    positions; pairs: two reads take the positions of a run in turn, so that a query's groups are closed by a query of the
    other read.  Sizes are tried in turn, 2, 3, .. 8, 2, ..: a run is taken where every read made of it changes a score's bits
    when its events are replayed query by query instead of in flush order (under the case's first window); where no size from the
    wanted one to 8 gives that, the matched query at hand becomes a read of its own and the cut goes on behind it.  So EVERY read
    of two or more matched queries depends on the flush order; the reads of one cannot."""
    base = gc.case("%s%d" % (world, gc._w(K)))
    wins = [w for w in windows(K) if w[0] > w[1]]
    d = gc.ref(base.name, *wins[0])
    if mode == "single":
        return replan(base, "order%d %s %s" % (gc._w(K), world, mode), "order", list(range(base.n)), wins, 3400 + K, claim={"mode": mode},
                      built_for="the order field of one query in a kept read")
    per = 2 if mode == "pairs" else 1
    matched = [p for p in range(base.n) if d[p].d]
    reads, r, at, want, sizes = [0] * base.n, 0, 0, ORDER_SIZES[0], {}

    def cut(first: int, last: int):
        """the reads of the run of positions [first, last]: their positions"""
        run = list(range(first, last + 1))
        return [run[i::per] for i in range(per)]

    pos, i = 0, 0                                   # the next position without a read; the next matched query without one
    while i < len(matched):
        taken = None
        for n in list(range(want, ORDER_SIZES[-1] + 1)):
            if i + n * per > len(matched):
                break
            parts = cut(pos, matched[i + n * per - 1])
            if all(sum(1 for p in part if d[p].d) == n and _sensitive(d, part) for part in parts):
                taken = (n, parts)
                break
        if taken is None:                           # a read of this one matched query (and the unmatched ones before it)
            for p in range(pos, matched[i] + 1):
                reads[p] = r
            r, pos, i = r + 1, matched[i] + 1, i + 1
            continue
        n, parts = taken
        for x, part in enumerate(parts):
            sizes[r + x] = n
            for p in part:
                reads[p] = r + x
        r, pos, i = r + per, parts[0][-1] + 1 if per == 1 else max(part[-1] for part in parts) + 1, i + n * per
        want = ORDER_SIZES[(n - 1) % len(ORDER_SIZES)]
    for p in range(pos, base.n):                    # unmatched queries behind the last matched one
        reads[p] = r
    return replan(base, "order%d %s %s" % (gc._w(K), world, mode), "order", reads, wins, 3400 + K, claim={"sizes": sizes, "mode": mode},
                  built_for="the float chains of the reads the order rule hands on")


def order_other_case(K: int) -> Case:
    """A kept read whose OTHER taxa's sums depend on the order inside a query.  Its first query gives the register slots to taxa
    290 and 291; its second is the representative R of a cluster with one entry per shared length K - 1 .. 7 right of it, each
    then a query of a read of its own: the entry that shares s letters closes R's level s + 1, so R's events come deepest
    level first, |T_k| = K + 1 - k, and taxon 1 -- in every level -- leaves one event record per level."""
    lay = Plan(K)
    claim = {"reads": []}
    for _ in range(2):
        claim["reads"].append(lay.read)
        lay.taxon = 289
        lay.hit([(K - 1, 1, 1)], fresh=False)
        c = lay.c
        lay.hit([(s, 1, 1) for s in range(K - 1, 6, -1)])
        for s in range(K - 1, 6, -1):
            lay.next_read()
            lay.add(gc.near(gc.rep_of(c, K), s, 1, 0))
        lay.next_read()
    return lay.finish("order%d other" % gc._w(K), "order", windows(K), 3450 + K, n_reads=lay.read, claim=claim,
                      built_for="the order of a query's event records in the staging row")


# ------------------------------------------------------------------------------------------------
# sizes
# ------------------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 254, 255, 256]
SIZES_BIG = [8190, 8191, 8192]
BIG_TAXA = 8200


def sizes_case(K: int, big: bool = False) -> Case:
    """per m a read whose one matched query has |T_7| = |T_8| = m and |T_k| = 1 above: the representative and m - 1 entries that
    share eight letters with it.  big: lists of 8190, 8191 and 8192 segments on an index of 8200 taxa, first window only."""
    lay = Plan(K, BIG_TAXA if big else gc.N_TAXA)
    for m in (SIZES_BIG if big else SIZES):
        lay.hit([(8, 1, m - 1)] if m > 1 else (), after=1)
        lay.next_read()
    return lay.finish("sizes%d%s" % (gc._w(K), " big" if big else ""), "sizes", windows(K)[:1] if big else windows(K), 3500 + K, n_reads=lay.read,
                      claim={"sizes": SIZES_BIG if big else SIZES}, built_for="sTab, EV_INV, the 13-bit sizes, why[3]" if big else "sTab, EV_INV, CNT_FIELDS",
                      never_coop=False)


def sizes_fb_case(K: int, n: int) -> Case:
    """a read of n matched queries in n clusters, every one the same taxon alone (its counter field reaches n), and a short
    read: no read above 255 queries -> 8-bit counter fields for the batch, else 16-bit ones"""
    lay = Plan(K)
    for _ in range(n):
        lay.hit(())
    lay.next_read()
    lay.hit(others(K, 2), after=1)
    return lay.finish("sizes%d fb %d" % (gc._w(K), n), "sizes", windows(K, 0, 1, -1), 3550 + K + n, claim={"queries": n},
                      built_for="FB == 8 up to 255 queries of a read, FB == 16 beyond")


COUNT_READS = [60000, 60001]


def sizes_count_case() -> Case:
    """wide records: reads of 60 000 and 60 001 queries -- one matched query and stretch queries -- and a short read.  The
    second is beyond the 16-bit counter fields' bound (why[0]) and, at ESR_MIN_KMERS queries or more, the sorted-event replay's"""
    lay = Plan(25)
    for n in COUNT_READS:
        lay.hit(others(25, 2), after=n - 1)
        lay.next_read()
    lay.hit(others(25, 2), after=1)
    return lay.finish("sizes128 count", "sizes", windows(25, 0), 3580, claim={"queries": COUNT_READS}, built_for="why[0]: more queries than the counter fields hold")


# ------------------------------------------------------------------------------------------------
# rule
# ------------------------------------------------------------------------------------------------
RULE_READS = ["kept: second", "handed: second", "kept: last", "handed: last"]


def rule_case(K: int, long_rows: bool) -> Case:
    """kept: the read's next matched query stands exactly where the groups of the one before close (a new range: Fmax == p).
    handed: it is the same k-mer again, one position on, and the groups close behind it (Fmax == p + 1).  second / last: the
    breaking query's place among the read's five matched queries.  long_rows: every read also has twelve queries of 91 taxa,
    a row beyond RMAX: score_main_kernel hands all four on, score_dense_kernel keeps two."""
    lay = Plan(K)
    sp = others(K, 2)
    for label in RULE_READS:
        handed, last = label.startswith("handed"), label.endswith("last")
        for i in range(5):
            breaking = i == (4 if last else 1)
            if breaking and handed:
                lay.add(lay_last_key(lay))
            else:
                lay.hit(sp, after=0 if (i == (3 if last else 0)) else 2)
        if long_rows:
            for _ in range(12):
                lay.hit(others(K, 90), after=1)
        lay.next_read()
    return lay.finish("rule%d%s" % (gc._w(K), " long rows" if long_rows else ""), "rule", windows(K), 3600 + K + long_rows, n_reads=lay.read,
                      claim={"reads": RULE_READS, "long_rows": long_rows}, built_for="prevF > Q.p in score_main_kernel%s" % (" and score_dense_kernel" if long_rows else ""))


def lay_last_key(lay: Plan):
    """the letters of the layout's last query"""
    k, out = lay.q[-1], []
    for _ in range(lay.K):
        out.append(k & 31)
        k >>= 5
    return out[::-1]


# ------------------------------------------------------------------------------------------------
# rows
# ------------------------------------------------------------------------------------------------
ROW_LENGTHS = [255, 256, 257, 511, 512, 513, 1023, 1024, 1025]
ROW_LONG = [(255, 2047), (255, 2048), (255, 2049), (256, 2047), (256, 2048), (256, 2049)]     # (queries of the read, records of its row)
ROW_BATCH = [65535, 65536, 65537]
ROW_BATCH_READS = 1000


def _row_read(lay: Plan, length: int, queries: int = 0):
    """Queries of the current read whose staging row has `length` records under (K, 7), narrow records: the two register taxa's
    final scores; per further taxon that shares K - 1 letters five event records (levels 7 .. K - 1 -- K = 12), per taxon
    that shares eight one segment record (levels 7, 8).  Padded with unmatched queries to `queries`."""
    assert lay.K == 12 and length >= 2
    a, b = divmod(length - 2, 5)
    n = 0
    while a > 0 or n == 0:
        take = min(a, 18)
        lay.hit(others(12, take + 1))
        a -= take
        n += 1
    if b:
        lay.hit([(11, 1, 1), (8, 1, b)])
        n += 1
    assert queries == 0 or n <= queries
    if queries:
        lay.unmatched(queries - n)


def rows_case(which: str) -> Case:
    lay = Plan(12)
    if which == "classes":
        for m in ROW_LENGTHS:
            _row_read(lay, m)
            lay.next_read()
        wins, claim = windows(12), {"rows": ROW_LENGTHS}
    elif which == "long":
        for q, m in ROW_LONG:
            _row_read(lay, m, q)
            lay.next_read()
        wins, claim = windows(12)[:2], {"rows": [m for _, m in ROW_LONG], "queries": [q for q, _ in ROW_LONG]}
    elif which.startswith("keys"):             # (12, 3), 64-byte records: 1000 reads of one query whose rows need `total` profile keys together
        total = int(which.split()[-1])
        # R alone: 10 counter fields; R and j further taxa that share 11 letters: 10 + 9 j keys; R and one that shares 10: 18
        y = next(n for n in range(9) if (total - 10 * ROW_BATCH_READS - 8 * n) % 9 == 0)      # reads of the last kind
        x = (total - 10 * ROW_BATCH_READS - 8 * y) // 9                                       # further taxa of the others, spread evenly
        js = [x // (ROW_BATCH_READS - y) + (i < x % (ROW_BATCH_READS - y)) for i in range(ROW_BATCH_READS - y)]
        for j in js:
            lay.hit(others(12, j))
            lay.next_read()
        for _ in range(y):
            lay.hit([(10, 1, 1)])
            lay.next_read()
        wins, claim = windows(12, -1), {"keys": total}
    else:
        total = int(which.split()[-1])
        per = 65
        for _ in range(ROW_BATCH_READS - 1):
            _row_read(lay, per)
            lay.next_read()
        _row_read(lay, total - per * (ROW_BATCH_READS - 1))
        lay.next_read()
        wins, claim = windows(12, 0, -1), {"total": total}
    return lay.finish("rows64 %s" % which, "rows", wins, 3700 + len(which), n_reads=lay.read, claim=claim,
                      built_for={"classes": "the row-merge classes", "long": "rowCap = RMAX below 256 queries, 8 per query from there"}.get(which, "the key retry" if "keys" in which else "the staging retry"))


# ------------------------------------------------------------------------------------------------
# taxa
# ------------------------------------------------------------------------------------------------
TAXA_ROWS = [2048, 2049, 4096, 4097, 8140, 8141, 16384, 16385]
TAXA_BATCH = [(0, 10), (0, 300), (0, 600), (0, 1025), (256, 1500), (0, 2)]       # (queries, records) of the reads


def taxa_case(n_taxa: int) -> Case:
    """the reads of TAXA_BATCH under a content table of n_taxa rows: the clusters' taxa 1 .. 20 are spread over the table, 20 -> the
    highest-numbered one"""
    lay = Plan(12, n_taxa, taxmap=lambda t: 1 + (t - 1) * (n_taxa - 2) // 19)
    for q, m in TAXA_BATCH:
        _row_read(lay, m, q)
        lay.next_read()
    return lay.finish("taxa64 %d" % n_taxa, "taxa", windows(12, 0, 1, -1), 3800 + n_taxa % 97, n_reads=lay.read, claim={"n_taxa": n_taxa},
                      built_for="the bounds of the bitmap merges, rowPerQuery, the dense pass's LDS, DENSE_TAXA")


# ------------------------------------------------------------------------------------------------
# dense, general
# ------------------------------------------------------------------------------------------------
DENSE_LISTS = [1, 3, 4, 5, 63, 64, 65, 128, 129, 192, 193, 256, 300]
DENSE_READS = [1, 3, 4, 5]


def dense_case(K: int, which: str) -> Case:
    lay = Plan(K)
    if which == "lists":                       # one read: a query per list length, and twelve of 91 taxa
        for n in DENSE_LISTS:
            lay.hit(others(K, n - 1), after=1)
        for _ in range(12):
            lay.hit(others(K, 90))
        lay.next_read()
        lay.hit(others(K, 2))
        claim = {"handed": 1, "lists": DENSE_LISTS}
    elif which == "queries":                   # handed reads of 1, 2 and 3 queries: 300 taxa are 298 x 4 records and more
        for n in (1, 2, 3):
            for _ in range(n):
                lay.hit(others(K, 299))
            lay.next_read()
        lay.hit(others(K, 2))
        claim = {"handed": 3, "queries": [1, 2, 3]}
    elif which == "split":                     # a read handed on whose first query has one taxon in two chunks of 64 segments (REC_SPLIT) and
        def custom(R):                         # levels of 71 and more taxa (REC_SAT: exact sizes on an odd and an even level)
            lay.entry(gc.near(R, K - 1, 0, 0), 300)
            lay.entry(gc.near(R, 8, 0, 0), 300)
        lay.hit([(K - 2, 1, 70), (7, 1, 8)], custom=custom)
        for _ in range(12):
            lay.hit(others(K, 90))
        lay.next_read()
        lay.hit(others(K, 2))
        claim = {"handed": 1}
    else:
        n = int(which.split()[-1])
        for i in range(n + 2):
            if 0 < i <= n:
                for _ in range(12):
                    lay.hit(others(K, 90))
            else:
                lay.hit(others(K, 2))
            lay.next_read()
        lay.read -= 1
        claim = {"handed": n}
    return lay.finish("dense%d %s" % (gc._w(K), which), "dense", windows(K)[:2], 3900 + K + len(which), claim=claim,
                      built_for="score_dense_kernel", never_coop=False)


GENERAL_TAXA = [255, 256, 257]
GENERAL_SEGS = [1023, 1024, 1025]


def general_case(K: int, which: str) -> Case:
    if which == "taxa":                        # per n a read of two queries that together touch n taxa
        lay = Plan(K)
        for n in GENERAL_TAXA:
            lay.hit(others(K, 199))
            lay.hit([(K - 2, 0, n - 201)], fresh=False)
            lay.next_read()
        claim = {"taxa": GENERAL_TAXA}
    else:
        lay = Plan(K, 1100)
        for n in GENERAL_SEGS:
            lay.hit([(K - 1, 1, 19), (K - 2, 1, 500), (K - 3, 0, n - 520)], after=1)
            lay.next_read()
        claim = {"segments": GENERAL_SEGS}
    return lay.finish("general%d %s" % (gc._w(K), which), "general", windows(K)[:2], 3950 + K + len(which), n_reads=lay.read, claim=claim,
                      built_for="score_kernel: TLIST and AGG" if which == "taxa" else "score_kernel: DQ_SEGS", never_coop=False)


# ------------------------------------------------------------------------------------------------
# the list
# ------------------------------------------------------------------------------------------------
def _builders():
    b = {}
    for K in (12, 25):
        w = gc._w(K)
        for n in TAKE_BATCHES:
            b["take%d %d" % (w, n)] = functools.partial(take_case, K, n)
        b["take%d 129 tail" % w] = functools.partial(take_case, K, 129, True)
        b["phase%d" % w] = functools.partial(phase_case, K)
        b["slots%d reads" % w] = functools.partial(slots_case, K)
        b["slots%d items" % w] = functools.partial(slots_items_case, K)
        b["slots%d items wide" % w] = functools.partial(slots_items_wide_case, K)
        b["registers%d" % w] = functools.partial(registers_case, K)
        for world in ORDER_WORLDS:
            for mode in ("chunks", "pairs", "single"):
                b["order%d %s %s" % (w, world, mode)] = functools.partial(order_case, K, world, mode)
        b["order%d other" % w] = functools.partial(order_other_case, K)
        b["sizes%d" % w] = functools.partial(sizes_case, K)
        for n in (255, 256):
            b["sizes%d fb %d" % (w, n)] = functools.partial(sizes_fb_case, K, n)
        for long_rows in (False, True):
            b["rule%d%s" % (w, " long rows" if long_rows else "")] = functools.partial(rule_case, K, long_rows)
        for which in ["lists", "queries"] + ["reads %d" % n for n in DENSE_READS]:
            b["dense%d %s" % (w, which)] = functools.partial(dense_case, K, which)
        for which in ("taxa", "segments"):
            b["general%d %s" % (w, which)] = functools.partial(general_case, K, which)
    b["sizes64 big"] = functools.partial(sizes_case, 12, True)
    b["sizes128 count"] = sizes_count_case
    b["dense64 split"] = functools.partial(dense_case, 12, "split")
    for which in ["classes", "long"] + ["batch %d" % t for t in ROW_BATCH] + ["keys %d" % t for t in ROW_BATCH]:
        b["rows64 %s" % which] = functools.partial(rows_case, which)
    for n in TAXA_ROWS:
        b["taxa64 %d" % n] = functools.partial(taxa_case, n)
    return b


_BUILDERS = _builders()
# left out of the comparison with the sequential oracle on the CPU (the replay remains their reference): lists of 8190 .. 8192 segments
NO_ORACLE = ("sizes64 big",)


def case_names(family=None) -> list:
    return [n for n in _BUILDERS if family is None or n.startswith(family)]


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def ref(name: str, k_high: int, k_low: int) -> list:
    """the reference of a case under a window, computed once and left unchanged"""
    return gc.reference(case(name), k_high, k_low)


@functools.lru_cache(maxsize=None)
def facts(name: str, k_high: int, k_low: int, sorting_merge: bool = False) -> list:
    return read_facts(case(name), ref(name, k_high, k_low), k_high, k_low, sorting_merge)
