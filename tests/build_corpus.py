"""Hand-made inputs for the index builder and editor (kasa_build.h and kasa_edit.h behind kasa_build_*), for 12-letter (64-bit)
and 25-letter (128-bit) k-mers, with a plain reference.  No device code here: tests/test_build_corpus_cpu.py shows that every
case holds what its family claims and holds the reference to the project's numpy helpers and the oracle's encoder,
tests/test_gpu_build_corpus.py runs the same cases through capi.Builder.

A case is a content (tax IDs per content row), an ordered list of steps for one builder --
    ("add", sequences, tax IDs, protein)      ("index", sorted unique records, chunk)      ("drop", tax IDs)
    ("shrink", strategy, percentage)
-- with K, frames, max_pairs_per_brick and KASA_EDIT_CHUNK_RECORDS where wanted, the bin counts to ask taxa_histogram() for,
and the family's claim as data.

Amino-acid input gives letter-exact control: with kLow = 1 a sequence of L letters yields its L windows, '^'-padded, every
letter is `ch & 31` ('*' reads as '['), so the bytes 0x40 .. 0x5F write any of the 32 letters, '^' (30) and '_' (31) among
them; an index run (add_index) is any sorted unique list of records.

reference() is plain loops over Python ints (a 128-bit k-mer is one int): the windows of every sequence (DNA: the codon table
and the reference project's rules, Read.hpp:1991-2290), without the k-mers that hold a '_' for DNA, the sorted unique
(k-mer, tax ID) pairs, their union with the index runs, delete, every n-th (Shrink.hpp:270-308: a counter and a double per
taxon), entropy (Shrink.hpp:152-236), the halved rule (Shrink.hpp:108), the trie's runs, the frequency rows per content row
(zero rows for a repeated ID) and the taxa histogram.  It calls none of formats.make_index, trie_from_kmers, freq_from_index or
index_edit.shrink_thresholds: the CPU test holds those to it.

The large family's inputs and results are written down analytically with numpy (large_merge, large_shrink), never by sorting;
the same two functions make the scaled-down copies that the CPU test checks against reference()."""
import functools
import itertools
import math
from dataclasses import dataclass, field

import numpy as np

from kasa_amd import formats

# ---- the constants of the code under test, restated once (tests/test_build_corpus_cpu.py reads them out of the sources) ----------
KS = (12, 25)
MERGE_ITEMS = 8                                     # kasa_build.h: merged outputs per thread of bld_merge_kernel
BLOCK = 256                                         # threads per workgroup of every kernel launched through grid_for
GRID_CAP = 8192                                     # grid_for's cap: more items than GRID_CAP * BLOCK and a thread loops
MERGE_BLOCK = BLOCK * MERGE_ITEMS                   # merged outputs of one workgroup: 2048
FREQ_LDS_CELLS = 16384                              # bld_freq_kernel<LDS> when nRank * (K + 1) <= this; edit_rank_hist_kernel<LDS> when nRank <= this
TAXA_LDS_BINS = 1024                                # edit_taxa_hist_kernel: run lengths below this are counted in LDS
EDIT_CHUNK = 1 << 30                                # records per radix sort of the n-th filter
ENC_LONG_MIN = 65536                                # windows from which a sequence is encoded by all wavefronts
TILE32 = 4096                                       # kasa_radix::Tile<uint32_t>::SIZE: the pairs of one workgroup of the n-th filter's sort
RANK_BITS = 24                                      # the n-th filter sorts over this many rank bits: three passes
MAX_TAXA = 1 << 22                                  # kasa_build_create refuses this many content rows
TRIE_LETTERS = 6
PAD, ILLEGAL = 30, 31                               # '^' and '_'
HALF_SIX_PADS = 1039104990                          # Shrink.hpp:108: six '^' in the low 30 bits

CONTENT3 = (0, 11, 22, 33)
FILLER = 1                                          # the letter 'A'


# ---- keys ------------------------------------------------------------------------------------------------------------------------
def kmer(letters, K):
    """the K letters, leftmost first, as an int"""
    assert len(letters) == K and all(0 <= x < 32 for x in letters)
    v = 0
    for x in letters:
        v = (v << 5) | x
    return v


def padded(letters, K):
    return kmer(list(letters) + [PAD] * (K - len(letters)), K)


def letter(key, j):
    """letter j counted from the right"""
    return (key >> (5 * j)) & 31


def letters_of(key, K):
    return [letter(key, K - 1 - i) for i in range(K)]


def prot(letters):
    """the amino-acid bytes that encode to these letters"""
    return bytes(0x40 | x for x in letters)


def keys_array(keys, K):
    if K == 12:
        return np.asarray(keys, dtype=np.uint64)
    out = np.zeros(len(keys), dtype=formats.KEY128_DTYPE)
    out["lo"] = [k & (2 ** 64 - 1) for k in keys]
    out["hi"] = [k >> 64 for k in keys]
    return out


def records_array(records, K):
    """[(k-mer, tax ID)] as the file records add_index takes"""
    if isinstance(records, np.ndarray):
        return records
    rec = np.zeros(len(records), dtype=formats.REC_DTYPE if K == 12 else formats.REC128_DTYPE)
    if K == 12:
        rec["kmer"] = [k for k, _ in records]
    else:
        rec["lo"] = [k & (2 ** 64 - 1) for k, _ in records]
        rec["hi"] = [k >> 64 for k, _ in records]
    rec["tax"] = [t for _, t in records]
    return rec


def records_list(records, K):
    if not isinstance(records, np.ndarray):
        return list(records)
    if K == 12:
        return [(int(k), int(t)) for k, t in zip(records["kmer"], records["tax"])]
    return [((int(h) << 64) | int(l), int(t)) for l, h, t in zip(records["lo"], records["hi"], records["tax"])]


def key_ints(km):
    if km.dtype == formats.KEY128_DTYPE:
        return [(int(h) << 64) | int(l) for l, h in zip(km["lo"], km["hi"])]
    return [int(x) for x in km]


# ---- content ------------------------------------------------------------------------------------------------------------------------
class Content:
    """tax IDs per content row: a list, or a range for the contents of many taxa.  The first row of an ID owns its frequencies;
    the rank of an ID is its place among the sorted distinct IDs."""

    def __init__(self, rows):
        self.rows = rows
        if isinstance(rows, range):
            assert rows.step == 1
            self.ids = rows
        else:
            self.rows = list(rows)
            self.ids = sorted(set(self.rows))
            self._first = {}
            for r, t in enumerate(self.rows):
                self._first.setdefault(t, r)
            self._rank = {t: i for i, t in enumerate(self.ids)}

    def knows(self, t):
        return t in self.rows if isinstance(self.rows, range) else t in self._first

    def row(self, t):
        return self.rows.index(t) if isinstance(self.rows, range) else self._first[t]

    def rank(self, t):
        return self.rows.index(t) if isinstance(self.rows, range) else self._rank[t]

    @property
    def n_rows(self):
        return len(self.rows)

    @property
    def n_ranks(self):
        return len(self.ids)

    def array(self):
        if isinstance(self.rows, range):
            return np.arange(self.rows.start, self.rows.stop, dtype=np.uint32)
        return np.asarray(self.rows, dtype=np.uint32)


@dataclass
class Case:
    name: str
    family: str
    K: int
    content: Content
    steps: list
    frames: int = 3
    brick: int = 0                                  # max_pairs_per_brick, 0: sized by the device
    edit_chunk: int = 0                             # KASA_EDIT_CHUNK_RECORDS, 0: unset
    n_bins: tuple = ()                              # taxa_histogram(n) after the finish, 0: the default taxa + 1
    claim: dict = field(default_factory=dict)
    expected: object = None                         # the large family: written down with the input
    large: bool = False


@dataclass
class Expect:
    error: tuple = None                             # (index of the step that refuses, or "finish"; text the message holds)
    kmers: object = None
    taxids: object = None
    trie: object = None                             # ([prefix], [count])
    freq: object = None                             # content row -> [K counts], zero rows left out; or a dense array
    half: object = None                             # ([low 30 bits], [content row]) of a halved result
    stats: dict = None
    hist: dict = None                               # n_bins -> (bins, distinct k-mers) or the text of the refusal


# ---- windows -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def codon_lut():
    from kasa_amd import capi
    return tuple(int(x) for x in capi.builtin_codon_table())


def protein_windows(seq, K):
    """a sequence of L letters yields L windows: window w = letters w .. w + K - 1, '^' past the end (Read.hpp:2256-2290)"""
    L = len(seq)
    if L == 0:
        return []
    let = [((0x5B if c == 0x2A else c) & 31) for c in seq]
    mask = (1 << (5 * K)) - 1
    key = 0
    for i in range(K):
        key = (key << 5) | (let[i] if i < L else PAD)
    out = [key]
    for w in range(1, L):
        key = ((key << 5) & mask) | (let[w + K - 1] if w + K - 1 < L else PAD)
        out.append(key)
    return out


def dna_windows(seq, K, frames, lut=None):
    """three frames: a window at every base but the last two; --one: at every third base while a whole codon is left.  Window at
    base p = the codons at p, p + 3, ..; base codes A C T G = 0 1 2 3, past the end 4 (the marker), anything else 5; a codon
    with a 5 reads '_', else one with a 4 reads '^' (Read.hpp:1991-2075)."""
    lut = lut or codon_lut()
    n = len(seq)
    if n < 3:
        return []

    def code(p):
        if p >= n:
            return 4
        c = seq[p]
        return (c & 14) >> 1 if (c & 0xDF) in b"ACGT" else 5

    codes = [code(p) for p in range(n + 2)]
    out = []
    for w in range(n - 2 if frames == 3 else n // 3):
        p0 = w if frames == 3 else 3 * w
        key = 0
        for i in range(K):
            p = p0 + 3 * i
            key = (key << 5) | (lut[codes[p] * 64 + codes[p + 1] * 8 + codes[p + 2]] if p < n else PAD)
        out.append(key)
    return out


def has_illegal(key, K):
    return any(letter(key, j) == ILLEGAL for j in range(K))


# ---- the filters -------------------------------------------------------------------------------------------------------------------
def nth_keeps(taxids, P):
    """Shrink.hpp:270-308 with fabsf(P) (Shrink.hpp:405), P a float: per taxon a counter from 1 and a double d from the step
    100 / |P|; a record goes iff counter == (uint64_t)d, then d += step.  A step below 1 (or P = 0) starts at (uint64_t)d = 0,
    which the counter never equals."""
    a = abs(float(np.float32(P)))
    if a == 0.0 or not 100.0 / a >= 1.0:
        return [True] * len(taxids)
    step = 100.0 / a
    counter, nxt, keep = {}, {}, []
    for t in taxids:
        c, d = counter.get(t, 1), nxt.get(t, step)
        if c != int(d):
            keep.append(True)
        else:
            keep.append(False)
            nxt[t] = d + step
        counter[t] = c + 1
    return keep


def nth_table(P, max_ordinal):
    """the ordinals the rule above drops from a taxon, up to max_ordinal: the same for every taxon"""
    keep = nth_keeps([0] * max_ordinal, P)
    return [j + 1 for j, k in enumerate(keep) if not k]


@functools.lru_cache(maxsize=None)
def _entropy_of_counts(counts, K):
    h = 0.0
    for c in counts:
        p = np.float32(c) / np.float32(K)                               # float(letterCount) / size()
        h += float(p * np.log2(p))                                      # a float product, summed in double
    h = h * (-1)
    return (h * math.log(2)) / math.log(22) > 0.5


def entropy_keeps(key, K):
    """Shrink.hpp:174-202: the letters sorted, the share of every distinct one as a float, '^' included"""
    let = sorted(letters_of(key, K))
    counts = tuple(len(list(g)) for _, g in itertools.groupby(let))
    return _entropy_of_counts(counts, K)


def half_keeps(key):
    return (key & 0x3FFFFFFF) != HALF_SIX_PADS                          # Shrink.hpp:108


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def check_run(records, content):
    """(index, message) of the first record that add_index refuses, or None"""
    for i, (k, t) in enumerate(records):
        if not content.knows(t):
            return i, "record %d has tax ID %d, which the content file does not list" % (i, t)
        if i and not records[i - 1] < (k, t):
            return i, "record %d (tax ID %d) does not follow its predecessor in strict (k-mer, tax ID) order" % (i, t)
    return None


def trie_of(keys, K):
    shift = 5 * (K - TRIE_LETTERS)
    prefix, count = [], []
    for k in keys:
        p = k >> shift
        if prefix and prefix[-1] == p:
            count[-1] += 1
        else:
            prefix.append(p)
            count.append(1)
    return prefix, count


def freq_of(records, content, K):
    out = {}
    for k, t in records:
        row = out.setdefault(content.row(t), [0] * K)
        for j in range(K):
            if letter(k, j) != PAD:
                row[j] += 1
    return {r: v for r, v in out.items() if any(v)}


def histogram_of(keys, n_bins):
    """bins[c] = distinct k-mers with c records; refused when a k-mer carries n_bins records or more, naming the first such run's
    last record"""
    bins, bad = [0] * n_bins, None
    i = 0
    while i < len(keys):
        j = i
        while j + 1 < len(keys) and keys[j + 1] == keys[i]:
            j += 1
        if j - i + 1 >= n_bins:
            bad = j if bad is None else bad
        else:
            bins[j - i + 1] += 1
        i = j + 1
    if bad is not None:
        return "the k-mer that ends at record %d carries %d records or more" % (bad, n_bins)
    return bins, sum(bins)


def reference(case):
    K, content = case.K, case.content
    pairs, runs, drop, shrink = set(), [], set(), None
    pairs_in = bricks = staged = 0
    staged_protein = None
    limit = case.brick or (1 << 62)
    for si, step in enumerate(case.steps):
        if step[0] == "add":
            _, seqs, taxids, protein = step
            for seq, t in zip(seqs, taxids):
                assert content.knows(t)
                w = protein_windows(seq, K) if protein else dna_windows(seq, K, case.frames)
                if not w:
                    continue
                if staged and (staged + len(w) > limit or staged_protein != protein):   # a brick ends between sequences
                    bricks, staged = bricks + 1, 0
                staged_protein, staged, pairs_in = protein, staged + len(w), pairs_in + len(w)
                pairs.update((k, t) for k in w if protein or not has_illegal(k, K))
        elif step[0] == "index":
            rec = records_list(step[1], K)
            bad = check_run(rec, content)
            if bad:
                return Expect(error=(si, bad[1]))
            runs.append(rec)
        elif step[0] == "drop":
            drop.update(step[1])
        else:
            shrink = (step[1], step[2])
    bricks += 1 if staged else 0
    merges, union = max(bricks - 1, 0), set(pairs)
    for rec in runs:                                                    # a run is merged unless it or the result so far is empty
        if union and rec:
            merges += 1
        union.update(rec)
    records = sorted(union)
    n0 = len(records)
    records = [r for r in records if r[1] not in drop]
    n1 = len(records)
    full = records
    if shrink:
        s, P = shrink
        if s == 1:
            keep = nth_keeps([t for _, t in records], P)
        elif s == 2:
            keep = [half_keeps(k) for k, _ in records]
        else:
            keep = [entropy_keeps(k, K) for k, _ in records]
        records = [r for r, kp in zip(records, keep) if kp]
        if not records:
            return Expect(error=("finish", "strategy %d leaves no record of the %d" % (s, n1)))
    halved = bool(shrink) and shrink[0] == 2
    keys = [k for k, _ in records]
    e = Expect(kmers=keys, taxids=[t for _, t in records], trie=trie_of(keys, K),
               freq=freq_of(full if halved else records, content, K),
               stats=dict(pairs_in=pairs_in, bricks=bricks, merges=merges, records_out=len(records), index_in=sum(len(r) for r in runs),
                          dropped_delete=n0 - n1, dropped_shrink=n1 - len(records)), hist={})
    if halved:
        e.half = ([k & 0x3FFFFFFF for k in keys], [content.row(t) for _, t in records])
    for nb in case.n_bins:
        e.hist[nb] = "halved" if halved else histogram_of(keys, nb or content.n_rows + 1)
    return e


def expect(case):
    return case.expected if case.expected is not None else reference(case)


def merge_path(a, b):
    """the merged outputs of two runs, ties A first: [(source, index in the source)] -- what bld_merge_kernel walks before it drops
    the outputs that equal their predecessor"""
    out, i, j = [], 0, 0
    while i < len(a) or j < len(b):
        if j >= len(b) or (i < len(a) and not b[j] < a[i]):
            out.append(("A", i))
            i += 1
        else:
            out.append(("B", j))
            j += 1
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
_MAKERS = {}                                        # name -> (family, large, thunk)


def _add(name, family, make, large=False):
    assert name not in _MAKERS, name
    _MAKERS[name] = (family, large, make)


def case_names(family=None, large=False):
    return [n for n, (f, lg, _) in _MAKERS.items() if (family is None or f == family) and lg == large]


def families():
    return list(dict.fromkeys(f for f, _, _ in _MAKERS.values()))


@functools.lru_cache(maxsize=64)
def case(name):
    family, large, make = _MAKERS[name]
    c = make()
    c.name, c.family, c.large = name, family, large
    return c


def _case(K, content, steps, **kw):
    return Case("", "", K, content if isinstance(content, Content) else Content(content), steps, **kw)


def stride(K):
    """k-mers q * stride cross a trie prefix every few q; in a 128-bit key both words change"""
    return {12: (1 << 30) // 3 + 12345, 25: (1 << 95) // 3 + (1 << 64) // 7 + 12345}[K]


def ukey(q, K):
    return (q + 1) * stride(K)


def urec(i, K, ids=CONTENT3[1:]):
    """record i of an ascending sequence of (k-mer, tax ID): every k-mer under each of the IDs in turn"""
    return ukey(i // len(ids), K), ids[i % len(ids)]


def _seq(first, n):
    """n amino-acid letters 1 .. 20 in turn from `first`"""
    return prot([(first + i) % 20 + 1 for i in range(n)])


def _each_k(name, family, make, large=False, ks=KS):
    for K in ks:
        _add("%s/%s/K%d" % (family, name, K), family, functools.partial(make, K), large)


# 1. unique ----------------------------------------------------------------------------------------------------------------------------
RUN_LENGTHS = (1, 2, 3, 255, 256, 257)
RANK_COUNTS = (1, 2, 64, 65)


def _unique(which, K):
    content, claim = list(CONTENT3), {}
    if which == "all equal":
        seqs, tax = [b"ABC"] * 40, [11] * 40
        claim = dict(pairs_in=120, records=3)
    elif which == "none equal":
        seqs, tax = [_seq(0, 9), prot([21, 22, 23, 24])], [11, 22]
        claim = dict(pairs_in=13, records=13)
    elif which == "runs tiny":                                          # one-letter sequences: the host's k-mers, r copies of each
        seqs = [prot([2 + i]) for i, r in enumerate(RUN_LENGTHS) for _ in range(r)]
        tax = [22] * len(seqs)
        claim = dict(runs=RUN_LENGTHS, records=len(RUN_LENGTHS))
    elif which == "runs encoded":                                       # three-letter sequences through the encoder
        seqs = [prot([3 * i + 1, 3 * i + 2, 3 * i + 3]) for i, r in enumerate(RUN_LENGTHS) for _ in range(r)]
        tax = [22] * len(seqs)
        claim = dict(runs=tuple(r for r in RUN_LENGTHS for _ in range(3)), records=3 * len(RUN_LENGTHS))
    elif which == "ranks":                                              # the same k-mer under 1, 2, 64, 65 taxa, every pair twice
        content = [0] + [100 + 3 * i for i in range(70)]
        seqs, tax = [], []
        for i, r in enumerate(RANK_COUNTS):
            for t in list(range(r)) + list(range(r - 1, -1, -1)):
                seqs.append(prot([2 + i]))
                tax.append(content[1 + (t * 3) % 70])
        claim = dict(taxa_of_kmer=RANK_COUNTS, records=sum(RANK_COUNTS))
    elif which in ("descending", "interleaved"):                        # sequences that share k-mers, not in tax ID order
        seqs = [_seq(i % 4, 7) for i in range(12)]
        tax = [33] * 4 + [22] * 4 + [11] * 4 if which == "descending" else [22, 33, 11, 33, 11, 22, 11, 22, 33, 22, 11, 33]
        claim = dict(order=which)
    elif which == "content unsorted":
        content = [0, 33, 11, 44, 22]
        seqs, tax = [_seq(i % 3, 6) for i in range(8)], [44, 11, 33, 22, 11, 44, 22, 33]
        claim = dict(rows_unsorted=True)
    else:                                                               # rows 3 and 5 repeat an ID: zero frequency rows
        content = [0, 22, 11, 22, 33, 11]
        seqs, tax = [_seq(i % 3, 6) for i in range(8)], [33, 11, 33, 22, 11, 22, 22, 33]
        claim = dict(zero_rows=(3, 5))
    return _case(K, content, [("add", seqs, tax, True)], claim=claim)


for _w in ("all equal", "none equal", "runs tiny", "runs encoded", "ranks", "descending", "interleaved", "content unsorted", "content repeats"):
    _each_k(_w, "unique", functools.partial(_unique, _w))


# 2. illegal letters (DNA) ---------------------------------------------------------------------------------------------------------------
def codon_of(x):
    """a codon of ACGT that the table reads as letter x"""
    lut = codon_lut()
    for a, b, c in itertools.product(range(4), repeat=3):
        if lut[a * 64 + b * 8 + c] == x:
            return bytes(b"ACTG"[i] for i in (a, b, c))
    raise KeyError(x)


def codon_letters():
    lut = codon_lut()
    return sorted({lut[a * 64 + b * 8 + c] for a, b, c in itertools.product(range(4), repeat=3)})


def near_misses():
    """(upper letter, lower letter, s): neither is '_', yet bits s .. s + 4 of the ten are ones"""
    L = codon_letters()
    return [(a, b, s) for a in L for b in L for s in range(1, 5) if (((a << 5) | b) >> s) & 31 == 31]


def dna_of(letters):
    return b"".join(codon_of(x) for x in letters)


def _illegal(which, frames, K):
    fill = [FILLER] * K
    normal = dna_of([codon_letters()[(5 * i + 1) % len(codon_letters())] for i in range(K)])
    claim = {}
    brick = 0
    if which == "positions":                                            # an N in codon p: window 0 holds its only '_' at letter p
        seqs = [normal]
        for p in range(K):
            s = bytearray(dna_of(fill))
            s[3 * p + (p % 3)] = ord("N")
            seqs.append(bytes(s))
        claim = dict(positions=K)
    elif which == "near misses":                                        # every pair of the table at every boundary: kept
        seqs, keys = [], []
        for a, b, _ in sorted(set((a, b, 0) for a, b, _ in near_misses())):
            for j in range(K - 1):
                let = fill[:j] + [a, b] + fill[j + 2:]
                seqs.append(dna_of(let))
                keys.append(kmer(let, K))
        claim = dict(kept=keys)
    elif which == "empty then normal":                                  # a brick per sequence; the first brick's run is empty
        seqs, brick = [b"N" * (3 * K), normal], 1
        claim = dict(bricks=2, merges=1, run_sizes="0, n")
    elif which == "normal then empty":
        seqs, brick = [normal, b"N" * (3 * K)], 1
        claim = dict(bricks=2, merges=1, run_sizes="n, 0")
    else:
        seqs, brick = [b"N" * (3 * K), b"ACN" * K], 1
        claim = dict(bricks=2, merges=1, records=0)
    return _case(K, CONTENT3, [("add", seqs, [(11, 22, 33)[i % 3] for i in range(len(seqs))], False)], frames=frames, brick=brick, claim=claim)


for _w in ("positions", "near misses", "empty then normal", "normal then empty", "two empty"):
    for _f in (3, 1):
        _each_k("%s/%s" % (_w, "three frames" if _f == 3 else "one"), "illegal", functools.partial(_illegal, _w, _f))


# 3. tiny and long sequences -----------------------------------------------------------------------------------------------------------------
TINY = {"protein": (1, 2), "dna": (3, 4), "one": (3, 4, 5, 6, 7, 8)}     # the lengths whose k-mers the host makes


def _dna(first, n):
    return bytes(b"ACGT"[(first + i * i + i // 3) % 4] for i in range(n))


def _tiny(mode, where, K):
    protein, frames = mode == "protein", 1 if mode == "one" else 3
    mk = _seq if protein else _dna
    normal = [mk(1, 40), mk(2, 47), mk(5, 38)]
    tiny = [mk(3 + n, n) for n in TINY[mode]]
    brick = 0
    if where == "lengths":
        lengths = {"protein": (1, 2, 3), "dna": (3, 4, 5), "one": (3, 4, 5, 6, 7, 8, 9)}[mode]
        seqs = [mk(n, n) for n in lengths]
    elif where == "first":
        seqs = tiny[:1] + normal
    elif where == "last":
        seqs = normal + tiny[-1:]
    elif where == "alone":
        seqs, brick = normal[:1] + tiny[:1] + normal[1:] + tiny[1:], 1
    else:
        seqs = tiny * 3
    return _case(K, CONTENT3, [("add", seqs, [(22, 11, 33)[i % 3] for i in range(len(seqs))], protein)], frames=frames, brick=brick,
                 claim=dict(tiny=TINY[mode], where=where))


for _m in ("protein", "dna", "one"):
    for _w in ("lengths", "first", "last", "alone", "only"):
        _each_k("%s/%s" % (_m, _w), "tiny", functools.partial(_tiny, _m, _w))


def _long(K):
    rng = np.random.default_rng(K)
    seqs = []
    for n in (ENC_LONG_MIN - 1, 3, ENC_LONG_MIN, 1, ENC_LONG_MIN + 1, 40):
        s = rng.integers(1, 21, size=n, dtype=np.uint8) | np.uint8(0x40)
        seqs.append(s.tobytes())
    seqs[4] = seqs[2][:30000] + seqs[4][30000:]                          # windows shared between two long sequences
    return _case(K, CONTENT3, [("add", seqs, [11, 22, 33, 22, 33, 11], True)], claim=dict(windows=(ENC_LONG_MIN - 1, ENC_LONG_MIN, ENC_LONG_MIN + 1)))


_each_k("long protein", "tiny", _long)


# 4. brick cuts ----------------------------------------------------------------------------------------------------------------------------------
BRICK_COUNTS = (2, 3, 5, 7, 8, 9)


def _bricks(which, K):
    limit = 10
    tax = None
    if which == "exact":
        steps, bricks = [("add", [_seq(0, 4), _seq(2, 6)], [11, 22], True)], 1
    elif which == "over by one":
        steps, bricks = [("add", [_seq(0, 4), _seq(2, 7)], [11, 22], True)], 2
    elif which == "single larger":
        steps, bricks = [("add", [_seq(0, 25), _seq(3, 4), _seq(9, 5)], [33, 11, 22], True)], 2
    elif which == "alphabet":
        steps, bricks = [("add", [_dna(0, 7)], [11], False), ("add", [_seq(0, 4)], [22], True)], 2
        limit = 100
    else:
        n = int(which)
        steps, bricks = [("add", [_seq(3 * i, 10) for i in range(n)], [(11, 22, 33)[i % 3] for i in range(n)], True)], n
    return _case(K, CONTENT3, steps, brick=limit, claim=dict(bricks=bricks, merges=bricks - 1))


for _w in ("exact", "over by one", "single larger", "alphabet") + tuple(str(n) for n in BRICK_COUNTS):
    _each_k(_w, "bricks", functools.partial(_bricks, _w))


# 5. merge: two index runs A and B -----------------------------------------------------------------------------------------------------------------
SIZE_EDGES = (0, 1, MERGE_ITEMS - 1, MERGE_ITEMS, MERGE_ITEMS + 1)
TWIN_SIZES = tuple(range(1, 34)) + (MERGE_BLOCK - 1, MERGE_BLOCK, MERGE_BLOCK + 1)
TWIN_PLACES = tuple(2 * MERGE_ITEMS - 1 + ph for ph in range(MERGE_ITEMS)) + (MERGE_BLOCK - 1,)


def _two(K, a, b, **claim):
    return _case(K, CONTENT3, [("index", a, 0), ("index", b, 0)], claim=dict(claim, nA=len(a), nB=len(b)), n_bins=(0,))


def _merge_sizes(nA, nB, K):
    """A the even, B the odd members of the ascending sequence"""
    return _two(K, [urec(2 * i, K) for i in range(nA)], [urec(2 * i + 1, K) for i in range(nB)])


def _merge_remainder(r, K):
    n = 2 * MERGE_ITEMS + r                                             # nA + nB, one twin (item 5) among them
    u = [urec(i, K) for i in range(n - 1)]
    return _two(K, sorted(u[0::2] + [u[5]]), u[1::2], remainder=r)


def _merge_twins(n, K):
    u = [urec(i, K) for i in range(n)]
    return _two(K, u, list(u), twins=n)


def _merge_single_twin(p, K):
    """one twin pair whose A copy is merged output p and whose B copy is p + 1; the other items go to A and B in turn"""
    n = p + 2 + 5
    a, b = [], []
    for pos in range(n):
        if pos == p + 1:
            continue
        d = pos if pos <= p else pos - 1
        if pos == p:
            a.append(urec(d, K))
            b.append(urec(d, K))
        else:
            (a if d % 2 else b).append(urec(d, K))
    return _two(K, a, b, twin_at=(p, p + 1))


def _merge_disjoint(which, K):
    lo, hi = [urec(i, K) for i in range(20)], [urec(i, K) for i in range(20, 33)]
    return _two(K, lo, hi, order="A below B") if which == "A below B" else _two(K, hi, lo, order="B below A")


def _merge_taxa(which, K):
    content = [0] + list(range(10, 100, 10))
    k = ukey(5, K)
    if which == "A larger":
        a, b = [(k, 50)], [(k, 20)]
    else:                                                               # one k-mer under nine taxa, the twin (k, 40) in the middle
        a = [(ukey(1, K), 10)] + [(k, t) for t in (10, 30, 40, 50, 70, 90)]
        b = [(k, t) for t in (20, 40, 60, 80)] + [(ukey(9, K), 10)]
    c = _two(K, a, b, same_kmer=which)
    c.content = Content(content)
    return c


def _merge_words(which, K):
    """128-bit keys that one word alone, or the words in the wrong order, would misorder"""
    W = 1 << 64
    if which == "equal hi":
        keys = [5 * W + x for x in (1, 2, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, W - 1)]
    elif which == "equal lo":
        keys = [h * W + 7 for h in (0, 1, 2, (1 << 60) - 1, 1 << 60)]
    else:                                                               # lo falls while hi rises
        keys = [h * W + (W - 1 - h * 1000) for h in range(1, 12)] + [12 * W, 12 * W + (1 << 63), 13 * W + 1]
    recs = [(k, 22) for k in keys]
    return _two(K, sorted(recs[0::2] + [recs[3]]), recs[1::2], words=which)


def _merge_mixed(which, K):
    if which == "bricks and index":
        steps = [("add", [_seq(0, 10), _seq(4, 10), _seq(8, 9)], [11, 22, 33], True)]
        w = protein_windows(_seq(4, 10), K)
        run = sorted(set([(w[0], 22), (w[3], 22), (w[3], 33), (w[9], 11)] + [urec(i, K) for i in range(5)]))
        return _case(K, CONTENT3, steps + [("index", run, 3)], brick=10, claim=dict(bricks=3, merges=3), n_bins=(0,))
    n = int(which)
    runs = [[urec(i, K) for i in range(40) if i % (r + 2) == 0 or i % 7 == r] for r in range(n)]
    return _case(K, CONTENT3, [("index", r, 0) for r in runs], claim=dict(merges=n - 1), n_bins=(0,))


for _a in SIZE_EDGES:
    for _b in SIZE_EDGES:
        _each_k("sizes %d+%d" % (_a, _b), "merge", functools.partial(_merge_sizes, _a, _b))
for _r in range(MERGE_ITEMS):
    _each_k("remainder %d" % _r, "merge", functools.partial(_merge_remainder, _r))
for _n in TWIN_SIZES:
    _each_k("twins %d" % _n, "merge", functools.partial(_merge_twins, _n))
for _p in TWIN_PLACES:
    _each_k("single twin at %d" % _p, "merge", functools.partial(_merge_single_twin, _p))
for _w in ("A below B", "B below A"):
    _each_k(_w, "merge", functools.partial(_merge_disjoint, _w))
for _w in ("A larger", "twin inside"):
    _each_k("same k-mer/%s" % _w, "merge", functools.partial(_merge_taxa, _w))
for _w in ("equal hi", "equal lo", "crossed"):
    _each_k("words/%s" % _w, "merge", functools.partial(_merge_words, _w), ks=(25,))
for _w in ("3", "4", "bricks and index"):
    _each_k("mixed/%s" % _w, "merge", functools.partial(_merge_mixed, _w))


# 6. trie ----------------------------------------------------------------------------------------------------------------------------------------
PREFIX_RUNS = (1, 255, 256, 257)


def _trie(which, K):
    shift = 5 * (K - TRIE_LETTERS)
    if which == "one prefix":
        keys = [(77 << shift) | (i * 977 + 1) for i in range(300)]
    elif which == "prefix per record":
        keys = [((i * 3 + 1) << shift) | 5 for i in range(300)]
    elif which == "bit shift":                                          # neighbours that differ in bit `shift` alone: a new entry
        keys = [(6 << shift) | 9, (7 << shift) | 9, (8 << shift) | 9, (9 << shift) | 9]
    elif which == "bit below shift":                                    # ... in bit shift - 1 alone: the same entry
        keys = [(6 << shift) | 9, (6 << shift) | (1 << (shift - 1)) | 9, (7 << shift) | 9, (7 << shift) | (1 << (shift - 1)) | 9]
    else:                                                               # runs of 1, 255, 256, 257 records; the last entry holds 3
        keys = []
        for p, r in enumerate(PREFIX_RUNS + (3,)):
            keys += [((p * 5 + 2) << shift) | (i * 31 + p) for i in range(r)]
    claim = {"one prefix": (300,), "prefix per record": (1,) * 300, "bit shift": (1, 1, 1, 1), "bit below shift": (2, 2), "runs": PREFIX_RUNS + (3,)}[which]
    return _case(K, CONTENT3, [("index", [(k, 22) for k in keys], 0)], claim=dict(counts=claim))


for _w in ("one prefix", "prefix per record", "bit shift", "bit below shift", "runs"):
    _each_k(_w, "trie", functools.partial(_trie, _w))


# 7. frequencies ---------------------------------------------------------------------------------------------------------------------------------
def freq_ranks(K):
    """the last rank count whose histogram bld_freq_kernel keeps in LDS, and the first it does not"""
    n = FREQ_LDS_CELLS // (K + 1)
    return n, n + 1


def _freq(n_ranks, repeat, K):
    rows = list(range(n_ranks))                                         # tax ID = rank; rank 0 is the content's "non_unique"
    if repeat:
        rows = rows[:5] + [3, 1] + rows[5:]
    top = n_ranks - 1
    keys = []
    for t in range(K):                                                  # a trailing run of t '^', t = 0 .. K - 1 (K: the sequences below)
        keys.append(kmer([2 + (i + t) % 20 for i in range(K - t)] + [PAD] * t, K))
    for j in range(1, K):                                               # an inner '^' alone at letter j
        let = [3 + (i % 19) for i in range(K)]
        let[K - 1 - j] = PAD
        keys.append(kmer(let, K))
    for j in range(2, K):                                               # ... above a trailing run of j - 1 or of one
        for t in {1, j - 1}:
            let = [4 + (i % 17) for i in range(K)]
            let[K - 1 - j] = PAD
            let[K - t:] = [PAD] * t
            keys.append(kmer(let, K))
    keys = sorted(set(keys))
    recs = sorted([(k, (1, top, top // 2)[i % 3]) for i, k in enumerate(keys)] + [(k, top) for k in keys[::4]] + [(k, 1) for k in keys[1::5]])
    recs = sorted(set(recs))
    steps = [("index", recs, 0), ("add", [b"^^^", b"^"], [top, 1], True)]
    return _case(K, rows, steps, claim=dict(n_ranks=n_ranks, lds=n_ranks * (K + 1) <= FREQ_LDS_CELLS, trailing=tuple(range(K + 1)), inner=tuple(range(1, K))))


for _side in (0, 1):
    _each_k("ranks %s" % ("at" if _side == 0 else "past"), "freq", lambda K, s=_side: _freq(freq_ranks(K)[s], False, K))
_each_k("repeated id", "freq", lambda K: _freq(40, True, K))


# 8. load checks ---------------------------------------------------------------------------------------------------------------------------------
def _load(which, K):
    content = [10, 20, 30, 40]
    good = [urec(i, K, (10, 20, 30)) for i in range(30)]
    r, chunk, second = list(good), 0, None
    if which == "swap":
        r[13], r[14] = r[14], r[13]
        bad = 14
    elif which == "duplicate":
        r[14] = r[13]
        bad = 14
    elif which == "descending id":                                      # the same k-mer, the IDs 30 then 20
        r[12], r[13], r[14] = (r[12][0], 10), (r[12][0], 30), (r[12][0], 20)
        bad = 14
    elif which == "id below":
        r[7] = (r[7][0], 5)
        bad = 7
    elif which == "id above":
        r[7] = (r[7][0], 41)
        bad = 7
    elif which == "between chunks":                                     # record 10 opens the second chunk and equals record 9
        r[10], chunk, bad = r[9], 10, 10
    elif which == "chunk of one":
        r[21], chunk, bad = r[20], 1, 21
    elif which == "chunk of one, good":
        chunk, bad = 1, None
    elif which == "two bad":
        r[22], r[9] = r[21], (r[9][0], 99)
        bad = 9
    elif which == "two bad, two chunks":
        r[22], r[9], chunk = r[21], r[8], 16
        bad = 9
    elif which == "hi only":                                            # 128 bits: the high word falls, the low word rises
        W = 1 << 64
        r = [(5 * W + 100, 10), (6 * W + 200, 10), (5 * W + 300, 10), (7 * W, 10)]
        bad = 2
    elif which == "lo only":
        W = 1 << 64
        r = [(5 * W + 100, 10), (5 * W + 300, 10), (5 * W + 200, 10), (7 * W, 10)]
        bad = 2
    else:                                                               # a second run that begins below the first run's end: two runs, accepted
        second, bad = good[:10], None
        r = good[5:]
    steps = [("index", r, chunk)] + ([("index", second, 0)] if second else [])
    return _case(K, content, steps, claim=dict(bad=bad))


for _w in ("swap", "duplicate", "descending id", "id below", "id above", "between chunks", "chunk of one", "chunk of one, good", "two bad",
           "two bad, two chunks", "second run below"):
    _each_k(_w, "load", functools.partial(_load, _w))
for _w in ("hi only", "lo only"):
    _each_k(_w, "load", functools.partial(_load, _w), ks=(25,))


# 9. delete --------------------------------------------------------------------------------------------------------------------------------------
def _delete(which, K):
    content = [0, 11, 22, 33, 44]
    recs = [urec(i, K, (11, 22, 33, 44)) for i in range(90) if i % 5]
    drop = {"one": [22], "top rank": [44], "unknown ids": [7, 4_000_000_000, 23], "every": [44, 11, 0, 33, 22, 5]}[which]
    return _case(K, content, [("index", recs, 0), ("drop", drop)], claim=dict(drop=which, n=len(recs)), n_bins=(0,))


for _w in ("one", "top rank", "unknown ids", "every"):
    _each_k(_w, "delete", functools.partial(_delete, _w))


# 10. every n-th -----------------------------------------------------------------------------------------------------------------------------------
PERCENTAGES = (50.0, 25.0, float(np.float32(66.67)), 99.0, -37.5, 0.0, 150.0, 100.0)
TAXON_SIZES = (31, 32, 33, 63, 64, 65)
CHUNKS = (1, 2, TILE32 - 1, TILE32, TILE32 + 1)


def _by_taxa(taxa, K):
    """record i: an ascending k-mer under taxa[i]"""
    return [(ukey(i, K), t) for i, t in enumerate(taxa)]


def _nth(which, arg, K):
    content, chunk, P = [0, 11, 22, 33, 44, 55], 0, 50.0
    rng = np.random.default_rng(7)
    if which == "percentage":
        P = arg
        taxa = [int(x) for x in rng.choice([11, 22, 22, 33, 33, 33, 33, 55], size=600)]
    elif which == "taxon size":                                         # the largest taxon sizes the bitmap of ordinals: 32 bits a word
        taxa = [11] * arg + [22] * (arg - 5) + [33] * 3
        taxa = [taxa[i] for i in rng.permutation(len(taxa))]
    elif which == "chunk":
        chunk, P = arg, float(np.float32(66.67))
        taxa = [int(x) for x in rng.choice([11, 22, 33, 33, 55, 55, 55], size=150 if arg < 3 else 3 * TILE32 + 5)]
    elif which == "drop positions":                                     # P = 50: a taxon's second record goes; chunks of 8
        chunk = 8
        taxa = [22, 33, 33, 11, 33, 33, 33, 11, 22, 33, 44, 44, 55, 44, 44, 55, 55, 11]
    elif which == "one rank":
        taxa, P = [33] * (2 * TILE32 + 37), float(np.float32(66.67))
    elif which == "ranks":                                              # arg: (content rows, the ranks in use)
        content, ranks = range(arg[0]), arg[1]
        taxa = [ranks[int(x)] for x in rng.integers(0, len(ranks), size=500)]
    return _case(K, content, [("index", _by_taxa(taxa, K), 0), ("shrink", 1, P)], edit_chunk=chunk, claim=dict(which=which, arg=arg, P=P),
                 n_bins=() if which == "ranks" else (0,))


RANK_PATTERNS = {
    "multiples of 256": (256 * 5 + 1, tuple(range(0, 256 * 5 + 1, 256))),
    "multiples of 65536, 70000 taxa": (70000, (0, 65536, 69999 // 256 * 256, 65536 + 256)),
    "top ranks, 2^22 - 1 taxa": (MAX_TAXA - 1, tuple(MAX_TAXA - 2 - i for i in range(0, 300, 7))),
    "ranks at the LDS limit": (FREQ_LDS_CELLS, (0, 1, 255, 256, FREQ_LDS_CELLS - 1)),
    "ranks past the LDS limit": (FREQ_LDS_CELLS + 1, (0, 1, 255, 256, FREQ_LDS_CELLS - 1, FREQ_LDS_CELLS)),
}

for _p in PERCENTAGES:
    _each_k("percentage %r" % _p, "nth", functools.partial(_nth, "percentage", _p))
for _s in TAXON_SIZES:
    _each_k("largest taxon %d" % _s, "nth", functools.partial(_nth, "taxon size", _s))
for _c in CHUNKS:
    _each_k("chunk %d" % _c, "nth", functools.partial(_nth, "chunk", _c))
_each_k("drop positions", "nth", functools.partial(_nth, "drop positions", None))
_each_k("one rank", "nth", functools.partial(_nth, "one rank", None))
for _w, _a in RANK_PATTERNS.items():
    _each_k(_w, "nth", functools.partial(_nth, "ranks", _a))


# 11. halved (K = 12) ----------------------------------------------------------------------------------------------------------------------------------
def _halved(which, K):
    content = [0, 11, 22, 33]
    six = [PAD] * 6
    P1, P2, P3 = [1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 7], [9, 9, 9, 9, 9, 9]
    k = lambda top, low: kmer(top + low, K)
    keys = [k(P1, [3, 4, 5, 6, 7, 8]), k(P2, [PAD, 3, 4, 5, 6, 7]), k(P2, [PAD, PAD, PAD, PAD, PAD, 3]), k(P3, [1, 1, 1, 1, 1, 1])]
    if which == "letter 5":                                             # '^' at letter 5 over real letters: stays
        keys += [k(P1, [PAD, 1, PAD, PAD, PAD, PAD]), k(P3, [PAD, PAD, PAD, PAD, PAD, 29])]
    elif which == "six pads":                                           # six '^' below a real letter 6: goes
        keys += [k(P1, six), k(P3, six)]
    elif which == "all pads":
        keys += [k(six, six)]
    elif which == "dropped first":                                      # the first record goes; its prefix keeps others
        keys += [k([0, 0, 0, 0, 0, 1], six), k([0, 0, 0, 0, 0, 1], [PAD, PAD, PAD, PAD, PAD, 31])]
    elif which == "first prefix dropped":                               # every record of the first prefix goes
        keys += [k([0, 0, 0, 0, 0, 1], six)]
    elif which == "dropped last":
        keys += [k([31] * 6, six)]
    elif which == "first of its prefix":                                # six '^' first of a prefix whose other records are larger
        keys += [k([5] * 6, six), k([5] * 6, [PAD, PAD, PAD, PAD, PAD, 31]), k([5] * 6, [31, 0, 0, 0, 0, 0])]
    elif which == "content repeats":
        content = [0, 22, 11, 22, 33, 11]
        keys += [k(P1, six)]
    recs = sorted({(x, (11, 22, 33)[i % 3]) for i, x in enumerate(sorted(keys))} | {(x, 33) for x in keys[::2]})
    return _case(K, content, [("index", recs, 0), ("shrink", 2, 0.0)], claim=dict(which=which), n_bins=(0,))


for _w in ("letter 5", "six pads", "all pads", "dropped first", "first prefix dropped", "dropped last", "first of its prefix", "content repeats"):
    _each_k(_w, "halved", functools.partial(_halved, _w), ks=(12,))


# 12. taxa histogram -------------------------------------------------------------------------------------------------------------------------------------
HIST_RUNS = (1, 2, TAXA_LDS_BINS - 1, TAXA_LDS_BINS, TAXA_LDS_BINS + 1)


def _hist(which, K):
    n_taxa = TAXA_LDS_BINS + 6
    content = range(n_taxa)
    steps_after, n_bins = [], (0,)
    if which in ("runs", "longest refused", "after delete", "after nth"):
        runs = HIST_RUNS + (n_taxa, 1, 3)                               # a run of n_taxa records; the last record closes a run of 3
        recs = [(ukey(q, K), t) for q, r in enumerate(runs) for t in range(r)]
        if which == "longest refused":
            n_bins = (n_taxa, n_taxa + 1)
        elif which == "after delete":
            steps_after = [("drop", [0, 5, TAXA_LDS_BINS, n_taxa - 1])]
        elif which == "after nth":
            steps_after = [("shrink", 1, 25.0)]
    elif which == "few bins":
        content = range(9)
        recs = [(ukey(q, K), t) for q, r in enumerate((1, 4, 2, 3, 4, 1)) for t in range(r)]
        n_bins = (5, 4, 0)
    else:                                                               # 128 bits: neighbouring k-mers equal in one word
        W = 1 << 64
        content = range(9)
        keys = [3 * W + 5, 3 * W + 6, 4 * W + 6, 4 * W + 7, 5 * W + 7]
        recs = [(x, t) for x in keys for t in (1, 2)]
    return _case(K, content, [("index", recs, 0)] + steps_after, claim=dict(which=which), n_bins=n_bins)


for _w in ("runs", "longest refused", "after delete", "after nth", "few bins"):
    _each_k(_w, "hist", functools.partial(_hist, _w))
_each_k("equal words", "hist", functools.partial(_hist, "equal words"), ks=(25,))


# 13. large: inputs and results written down analytically ----------------------------------------------------------------------------------------------------
def _mul(q, c, K):
    """q * c for an array q of values below 2^31 and a Python int c below 2^125: keys of width K"""
    q = q.astype(np.uint64)
    if K == 12:
        return q * np.uint64(c)
    limbs, carry = [], np.zeros(q.shape, np.uint64)
    for i in range(4):
        t = q * np.uint64((c >> (32 * i)) & 0xFFFFFFFF) + carry
        limbs.append(t & np.uint64(0xFFFFFFFF))
        carry = t >> np.uint64(32)
    out = np.zeros(q.shape, dtype=formats.KEY128_DTYPE)
    out["lo"], out["hi"] = limbs[0] | (limbs[1] << np.uint64(32)), limbs[2] | (limbs[3] << np.uint64(32))
    return out


def _np_records(keys, taxids, K):
    rec = np.zeros(keys.shape[0], dtype=formats.REC_DTYPE if K == 12 else formats.REC128_DTYPE)
    if K == 12:
        rec["kmer"] = keys
    else:
        rec["lo"], rec["hi"] = keys["lo"], keys["hi"]
    rec["tax"] = taxids
    return rec


def _np_letter(keys, j):
    return (formats.key_shr(keys, 5 * j) & np.uint64(31)).astype(np.int64)


def _np_runs(x):
    """(first index, length) of the runs of equal neighbours in x"""
    if x.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    first = np.flatnonzero(np.concatenate(([True], x[1:] != x[:-1])))
    return first, np.diff(np.concatenate((first, [x.shape[0]])))


def _np_expect(keys, rows, taxids, K, n_rows, freq_keys=None, freq_rows=None):
    """trie and frequency rows of sorted records (keys, content rows): numpy over the whole arrays, no sort"""
    pre = formats.key_shr(keys, 5 * (K - TRIE_LETTERS)).astype(np.uint32)
    first, length = _np_runs(pre)
    fk, fr = (keys, rows) if freq_keys is None else (freq_keys, freq_rows)
    freq = np.zeros((n_rows, K), dtype=np.uint64)
    for j in range(K):
        freq[:, j] = np.bincount(fr[_np_letter(fk, j) != PAD], minlength=n_rows)
    return Expect(kmers=keys, taxids=taxids, trie=(pre[first], length.astype(np.uint64)), freq=freq, hist={})


def large_merge(K, M, T, dropped):
    """The numbers m < M as records (k-mer (m // T + 1) * stride, tax ID 100 + 3 (m % T)): A holds the multiples of 2, B those of
    3, the twins are the multiples of 6; the taxa `dropped` (as m % T) are deleted in the same builder."""
    m = np.arange(M, dtype=np.int64)
    ids = (100 + 3 * np.arange(T)).astype(np.uint32)

    def rec(sel):
        return _mul(sel // T + 1, stride(K), K), ids[sel % T]

    in_a, in_b = m % 2 == 0, m % 3 == 0
    a, b = rec(m[in_a]), rec(m[in_b])
    union = m[in_a | in_b]
    kept = union[~np.isin(union % T, dropped)]
    keys, taxids = rec(kept)
    e = _np_expect(keys, kept % T + 1, taxids, K, T + 1)
    e.stats = dict(pairs_in=0, bricks=0, merges=1, records_out=int(kept.shape[0]), index_in=int(in_a.sum() + in_b.sum()),
                   dropped_delete=int(union.shape[0] - kept.shape[0]), dropped_shrink=0)
    _, per_kmer = _np_runs(kept // T)
    bins = np.bincount(per_kmer, minlength=T + 2)
    e.hist = {0: ([int(x) for x in bins], int(bins.sum()))}
    steps = [("index", _np_records(*a, K), 0), ("index", _np_records(*b, K), 1 << 22), ("drop", [int(ids[d]) for d in dropped])]
    return _case(K, [0] + [int(x) for x in ids], steps, n_bins=(0,), expected=e,
                 claim=dict(merged_outputs=int(in_a.sum() + in_b.sum()), twins=int((in_a & in_b).sum())))


def shrink_templates(K):
    """name -> the K - 6 low letters of a template, ascending by value"""
    n = K - TRIE_LETTERS
    t = {"one letter": [1] * n, "distinct": [8 + i for i in range(n)], "inner pad": [PAD, 3] + [PAD] * (n - 2), "pads": [PAD] * n}
    return dict(sorted(t.items(), key=lambda kv: kmer(kv[1], n)))


def large_shrink(K, strategy, P, n_perm, T):
    """Record i = (q, t, r): the q-th permutation of the letters 1 .. 6 as the six top letters, template t below them, under
    taxon r.  The letters of a k-mer are the same multiset for every q, so entropy keeps or drops a whole template; the halved
    rule reads the low six letters, which are the template's (K = 12); the ordinal of a record within its taxon is q * NT + t + 1."""
    templates = shrink_templates(K)
    NT = len(templates)
    perms = list(itertools.islice(itertools.permutations(range(1, 7)), n_perm))
    combos = [kmer(list(p) + tail, K) for p in perms for tail in templates.values()]
    assert combos == sorted(combos) and len(set(combos)) == len(combos)
    ck = keys_array(combos, K)
    ids = (100 + 3 * np.arange(T)).astype(np.uint32)
    i = np.arange(n_perm * NT * T, dtype=np.int64)
    combo, r = i // T, i % T
    keys, taxids, rows = ck[combo], ids[r], r + 1
    if strategy == 1:
        table = np.asarray(nth_table(P, n_perm * NT), dtype=np.int64)
        keep = ~np.isin(combo + 1, table)
        decided = {"ordinals dropped": int(table.shape[0])}
    else:
        rule = half_keeps if strategy == 2 else functools.partial(entropy_keeps, K=K)
        decided = {name: bool(rule(kmer(list(perms[0]) + tail, K))) for name, tail in templates.items()}
        assert all(bool(rule(c)) == list(decided.values())[j % NT] for j, c in enumerate(combos[:4 * NT]))
        keep = np.asarray(list(decided.values()))[combo % NT]
    full = (keys, rows) if strategy == 2 else (None, None)
    e = _np_expect(keys[keep], rows[keep], taxids[keep], K, T + 1, *full)
    e.stats = dict(pairs_in=0, bricks=0, merges=0, records_out=int(keep.sum()), index_in=int(i.shape[0]), dropped_delete=0,
                   dropped_shrink=int(i.shape[0] - keep.sum()))
    if strategy == 2:
        e.half = ((keys[keep] & np.uint64(0x3FFFFFFF)).astype(np.uint32), rows[keep].astype(np.uint16))
    return _case(K, [0] + [int(x) for x in ids], [("index", _np_records(keys, taxids, K), 1 << 21), ("shrink", strategy, P)], expected=e,
                 claim=dict(records=int(i.shape[0]), decided=decided))


def large_brick(K, A, L):
    """Every string of L amino-acid letters over an alphabet of A (the letters 1 .. A) as a sequence of its own, string j under
    taxon j % 3: one brick of A^L * L pairs.  The windows of a sequence are its suffixes, '^'-padded, so the unique k-mers are the
    strings of 1 .. L letters.  With '^' read as a digit A above the letters they are the L-digit numbers in base A + 1 whose digits
    A, once begun, go on to the end: ascending numbers are ascending k-mers.  A string shorter than L ends sequences of every
    taxon (A^l is 1 or 2 mod 3 for A = 2 mod 3, and the letters before it take A values or more); a string of L letters is one
    sequence."""
    assert A % 3 == 2 and A >= 3 and A < PAD and L < TRIE_LETTERS
    ids = np.asarray([100, 103, 106], dtype=np.uint32)
    j = np.arange(A ** L, dtype=np.int64)
    letters = np.stack([(j // A ** (L - 1 - i)) % A + 1 for i in range(L)], axis=1).astype(np.uint8)
    seqs = [bytes(row) for row in (letters | np.uint8(0x40))]
    v = np.arange((A + 1) ** L, dtype=np.int64)
    digit = np.stack([(v // (A + 1) ** (L - 1 - i)) % (A + 1) for i in range(L)], axis=1)
    pad = digit == A
    v, digit, pad = (x[~pad[:, 0] & (pad[:, 1:] >= pad[:, :-1]).all(axis=1)] for x in (v, digit, pad))
    length = L - pad.sum(axis=1)
    top = np.zeros(v.shape[0], dtype=np.uint64)                         # the L top letters: all above bit 64 of a 128-bit key
    base = 5 * (K - L) - (64 if K == 25 else 0)
    for i in range(L):
        top |= np.where(pad[:, i], PAD, digit[:, i] + 1).astype(np.uint64) << np.uint64(base + 5 * (L - 1 - i))
    low = padded([], K - L)                                             # the K - L letters below them are '^'
    if K == 12:
        keys = top | np.uint64(low)
    else:
        keys = np.zeros(v.shape[0], dtype=formats.KEY128_DTYPE)
        keys["lo"], keys["hi"] = low & (2 ** 64 - 1), top | np.uint64(low >> 64)
    whole = length == L
    of_whole = np.zeros(v.shape[0], dtype=np.int64)
    for i in range(L):
        of_whole = of_whole * A + np.where(whole, digit[:, i], 0)
    copies = np.where(whole, 1, 3)
    at = np.repeat(np.arange(v.shape[0]), copies)
    rank = np.where(whole[at], of_whole[at] % 3, np.arange(at.shape[0]) - np.repeat(np.cumsum(copies) - copies, copies))
    e = _np_expect(keys[at], rank + 1, ids[rank], K, 4)
    e.stats = dict(pairs_in=A ** L * L, bricks=1, merges=0, records_out=int(at.shape[0]), index_in=0, dropped_delete=0, dropped_shrink=0)
    return _case(K, [0] + [int(x) for x in ids], [("add", seqs, ids[j % 3], True)], expected=e, claim=dict(pairs=A ** L * L))


LARGE_BRICK = dict(A=14, L=5)
SMALL_BRICK = dict(A=5, L=3)
LARGE_MERGE = dict(M=20_200_000, T=300, dropped=(7, 150, 299))
SMALL_MERGE = dict(M=3_000, T=7, dropped=(2, 6))
LARGE_SHRINK = dict(n_perm=720, T=730)
SMALL_SHRINK = dict(n_perm=24, T=5)
LARGE_P = float(np.float32(66.67))

for _K in KS:
    _add("large/brick/K%d" % _K, "large", functools.partial(large_brick, _K, **LARGE_BRICK), large=True)
    _add("large/merge/K%d" % _K, "large", functools.partial(large_merge, _K, **LARGE_MERGE), large=True)
    for _s in (1, 2, 3):
        if _s != 2 or _K == 12:
            _add("large/shrink %d/K%d" % (_s, _K), "large", functools.partial(large_shrink, _K, _s, LARGE_P, **LARGE_SHRINK), large=True)


# ---- the amino-acid database with '^' letters of tests/golden/dbedit/halved_pads/ -------------------------------------------------------------------------
PADS_TAX = {"P0.1": 21, "P2.1": 21, "P5.1": 22, "P1.1": 22, "P3.1": 22, "P4.1": 23}


def pads_cases(directory):
    """(the merged index, the halved index) of a.fasta and b.fasta as cases for reference(); content rows 0, 21, 22, 23"""
    seqs = []
    for name in ("a.fasta", "b.fasta"):
        with open(directory + "/" + name) as f:
            for r in f.read().split(">")[1:]:
                head, body = r.split("\n", 1)
                seqs.append((PADS_TAX[head.split()[0]], body.replace("\n", "").encode()))
    steps = [("add", [s for _, s in seqs], [t for t, _ in seqs], True)]
    content = Content([0, 21, 22, 23])
    return Case("merged", "host", 12, content, steps), Case("halved", "host", 12, content, steps + [("shrink", 2, 0.0)])


# ---- what the device returns, in the reference's form ------------------------------------------------------------------------------------------------------
def freq_sparse(freq, K):
    """(rows with a count, their values) of a dict of rows or a dense array"""
    if isinstance(freq, dict):
        rows = sorted(freq)
        return np.asarray(rows, dtype=np.int64), np.asarray([freq[r] for r in rows], dtype=np.uint64).reshape(len(rows), K)
    rows = np.flatnonzero(freq.any(axis=1))
    return rows, freq[rows]


def arrays(e, K):
    """an Expect's k-mers, tax IDs, trie prefixes and counts as the arrays Builder.fetch() returns"""
    km = e.kmers if isinstance(e.kmers, np.ndarray) else keys_array(e.kmers, K)
    return (km, np.asarray(e.taxids, dtype=np.uint32), np.asarray(e.trie[0], dtype=np.uint32), np.asarray(e.trie[1], dtype=np.uint64))
