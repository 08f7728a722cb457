"""Hand-made reads for the encoder (kasa_batch_encode: encode_group_kernel, encode_kernel in its 192- and 512-k-mer ranking
forms, with the read id as payload, and its second launch over long sequences), with a plain numpy restatement of Read.hpp's
rules as the reference: keys in emission order, the read of every k-mer and -- where the encoder ranks -- the slot of every
k-mer.  The inputs of tests/test_encode_corpus_cpu.py (every family's claim from the reference alone, the reference against
the oracle, the dispatch rule restated) and of tests/test_gpu_encode_corpus.py (the device, form by form).  Pure numpy: no
device, nothing of oracle/ or kasa_amd/ but the 128-bit key's dtype.

The rules (Read.hpp:36-57 counts, :633-654 padding, :657-675 cleaning, :1068-1078 marker, :84-293 windows):
  marker    3 (K - kLow) X behind a DNA read, K - kLow '^' behind an amino-acid one
  padding   with X up to 3 K bases (with '^' up to K letters) -- marker included
  counts    DNA in 3 or 6 frames L - 3 K + 1 windows per strand if L > 3 K + 1; --one L/3 - K + 1 if L/3 > K + 1; amino acids
            L - K + 1 if L > K + 1; else none (L: padded length with the marker).  An empty sequence has none.
  cleaning  every byte but ACGTacgt is Z;  code = (byte & 14) >> 1: A 0, C 1, T 2, G 3, X 4, Z 5
  reverse   the complement (code ^ 2 for the four bases) of the padded body, reversed, then the marker
  letter    lut[c0 * 64 + c1 * 8 + c2] of the three codes from a position on
  key       K letters of 5 bits, the first one highest; window w begins at base w (--one: 3 w) and takes every third position
  protein   '*' -> '[', letter = byte & 31, window w = letters w .. w + K - 1

What follows from the counts and cannot be otherwise: a padded read has exactly 3 K bases (K letters) and therefore no window --
padding never reaches a k-mer, the only X a window sees are the marker's, and they stand at the letters from kLow on of the
last windows.  So of the 216 triples of codes 0 .. 5 a window can hold the 125 without X and (n, n, X), (n, X, X), (X, X, X):
156 per strand; the 60 others ((X, ., .) before a base, (n, X, n)) no input produces.  The codons family reaches every one of
the 156 on both strands; its claim is stated against that list (UNREACHABLE below: the other 60).

Families (each case names the form it is built for and the edge, Case.form and Case.why):
  alphabet     all 256 byte values as a base at positions = 0, 1, 2 (mod 3), inside windows and in the last window before
               the marker; reads of acgt only; reads of non-bases only -- under every DNA form; amino-acid reads of all 256
               values ('*', '[', '^', lower case among them)
  codons       the 125 + 30 + 1 reachable triples on both strands at every letter of a key, under a codon table that tells
               any two triples apart that differ in one position, and under the built-in one
  geometry     every raw length 0 .. 3 K + 8 (K + 8) under five (K, kHigh, kLow), 3 and 6 frames, --one, amino acids; batches
               whose first, last, every read is empty or too short; a batch whose offsets start at 21
  packing      amino-acid reads that carry each of the 32 letter values at each of the K letters of a key
  bounds       191, 192, 193, 511, 512, 513 k-mers per read by 3 frames, 6 frames and --one, the crossing read first and last;
               ENC_CHUNK - 1 .. 2 ENC_CHUNK + 1 windows per strand (--one: 169 .. 341); amino-acid reads of 512 and 513
  group_parts  groups of ENC_GROUP reads whose k-mers total CAPK - 1, CAPK, CAPK + 1 at every place a part can end; reads
               without k-mers first, inside, last, throughout; a last group of 1 .. G - 1 reads; more groups than a workgroup takes
  ranking      reads whose k-mers are all equal, ascending, descending, differ only in the last letter, only in key bits 7-8
               from the top, have every first letter, repeat far apart; K = 25: differ only in letter 25, 1, 13-14
  segments     reads of 0, 1, 2, 3 segments, empty ones among them; mates that would form k-mers if joined
  long         sequences of ENC_LONG_MIN - 1, ENC_LONG_MIN, ENC_LONG_MIN + 1 k-mers and the other cases of the second launch
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from kasa_amd.formats import KEY128_DTYPE

# ------------------------------------------------------------------------------------------------
# the encoder's constants, by the names they have in kasa_hip.hip (tests/test_encode_corpus_cpu.py reads them out of the file)
# ------------------------------------------------------------------------------------------------
ENC_CHUNK = 512
ENC_WAVES = 4
ENC_RANK_MAX = 512
ENC_LONG_MIN = 65536
ENC_GROUP = 4
ENC_GROUP_RM = 192
SMALL_RM = 192                                   # encode_kernel<Key, 192>: `c->maxCnt <= 192u`
GROUP_ROUNDS = (ENC_GROUP * 136 + 63) // 64      # constexpr int ROUNDS = (G * 136 + 63) / 64;
CAPK = GROUP_ROUNDS * 64                         # constexpr int CAPK = ROUNDS * 64;
LONG_BLOCKS = 256 * 8                            # const unsigned lblocks = 256 * 8;
LONG_SWEEP = LONG_BLOCKS * ENC_WAVES * ENC_CHUNK # windows one sweep of the second launch's grid takes

MODES = ("dna3", "dna6", "one", "protein")
FRAMES = {"dna3": 3, "dna6": 6, "one": 1, "protein": 3}
FORMS = ("group", "slots192", "slots512", "readid", "long")
GEOMETRIES = [(12, 12, 7), (12, 12, 12), (12, 12, 1), (25, 25, 7), (25, 25, 25)]

A, C, T, G, N = (ord(c) for c in "ACTGN")
BASE_OF_CODE = {0: A, 1: C, 2: T, 3: G, 5: N}    # a byte for every code a byte can have (X comes from the marker alone)
NON_X = (0, 1, 2, 3, 5)
UNREACHABLE = sorted({(a, b, c) for a in range(6) for b in range(6) for c in range(6)
                      if (a == 4 and (b != 4 or c != 4)) or (b == 4 and c != 4)})
REACHABLE = sorted({(a, b, c) for a in range(6) for b in range(6) for c in range(6)} - set(UNREACHABLE))


# ------------------------------------------------------------------------------------------------
# codon tables
# ------------------------------------------------------------------------------------------------
def builtin_table() -> np.ndarray:
    """The standard code (NCBI table 1) as the encoder's 366-entry table: any Z '_', else any X '^', TAA and TAG '[', TGA ']'."""
    tcag = "FFLLSSSSYY[[CC]WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
    place = {0: 2, 1: 1, 2: 0, 3: 3}              # code -> place in the order T C A G
    lut = np.zeros(366, dtype=np.uint8)
    for a in range(6):
        for b in range(6):
            for c in range(6):
                if 5 in (a, b, c):
                    ch = "_"
                elif 4 in (a, b, c):
                    ch = "^"
                else:
                    ch = tcag[place[a] * 16 + place[b] * 4 + place[c]]
                lut[a * 64 + b * 8 + c] = ord(ch) & 31
    return lut


def telling_table() -> np.ndarray:
    """366 entries; two triples of codes 0 .. 5 that differ in exactly one position get different letters (1, 6 and 11 times
    a difference of 1 .. 5 are never 0 mod 32)."""
    lut = np.zeros(366, dtype=np.uint8)
    for a in range(6):
        for b in range(6):
            for c in range(6):
                lut[a * 64 + b * 8 + c] = (a + 6 * b + 11 * c + 5) & 31
    return lut


TABLES = {"builtin": builtin_table, "telling": telling_table}


@functools.lru_cache(maxsize=None)
def table(name: str) -> np.ndarray:
    t = TABLES[name]()
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def codon_of_letter(name: str = "telling") -> dict:
    """letter -> three bytes that give it under the table (of ACGT where such a triple exists, else with N; the first in
    code order); the letters no triple gives are missing"""
    out = {}
    lut = table(name)
    for codes in ((0, 1, 2, 3), NON_X):                   # (one of the 32 values needs an N under the telling table)
        for a in codes:
            for b in codes:
                for c in codes:
                    out.setdefault(int(lut[a * 64 + b * 8 + c]), (BASE_OF_CODE[a], BASE_OF_CODE[b], BASE_OF_CODE[c]))
    return out


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    family: str
    seqs: list                     # the sequences, uint8 arrays
    K: int                         # letters of a key: 12 (64-bit index) or 25 (128-bit index)
    k_high: int
    k_low: int
    mode: str                      # one of MODES
    lut: str                       # one of TABLES
    form: str                      # one of FORMS: the encoder body the case is built for
    why: str                       # the edge it is built for, in words
    seg_read: list = None          # segments: the read of every sequence (ascending)
    n_reads: int = None
    debug: int = 0                 # debug flags of the run (8: the read id as payload)
    shift: int = 0                 # bytes in front of the first sequence (offsets[0]); uploaded through kasa_batch_upload_device
    second_launch: int = None      # long sequences the second launch lists (None: it is not started)
    claim: dict = field(default_factory=dict)

    def __post_init__(self):
        self.seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in self.seqs]
        if self.n_reads is None:
            self.n_reads = len(self.seqs)

    @property
    def wide(self) -> bool:
        return self.K == 25

    @property
    def ranked(self) -> bool:
        return self.form in ("group", "slots192", "slots512")

    def batch(self):
        """-> bases u8 (self.shift bytes of '#' in front), offsets i64[nSeq + 1] beginning at self.shift"""
        lens = [s.shape[0] for s in self.seqs]
        off = (np.concatenate(([0], np.cumsum(lens))) + self.shift).astype(np.int64)
        parts = [np.full(self.shift, ord("#"), dtype=np.uint8)] + self.seqs
        return np.concatenate(parts).astype(np.uint8), off


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def geometry(raw: int, K: int, k_low: int, mode: str):
    """-> (body, L, windows per strand) of a sequence of `raw` bytes"""
    if raw <= 0:
        return 0, 0, 0
    unit = 1 if mode == "protein" else 3
    marker = unit * (K - k_low)
    body = max(raw, unit * K - marker)
    L = body + marker
    if mode == "protein":
        cnt = L - K + 1 if L > K + 1 else 0
    elif mode == "one":
        cnt = L // 3 - K + 1 if L // 3 > K + 1 else 0
    else:
        cnt = L - 3 * K + 1 if L > 3 * K + 1 else 0
    return body, L, cnt


def strands(mode: str) -> int:
    return 2 if mode == "dna6" else 1


def raw_for(cnt: int, K: int, k_low: int, mode: str) -> int:
    """bytes of a sequence with `cnt` windows per strand (cnt >= 3; --one: the shortest such)"""
    unit = 1 if mode == "protein" else 3
    marker = unit * (K - k_low)
    raw = (3 * (cnt + K - 1) if mode == "one" else cnt + unit * K - 1) - marker
    assert raw > 0 and geometry(raw, K, k_low, mode)[2] == cnt, (cnt, K, k_low, mode)
    return raw


def codes_of(seq: np.ndarray) -> np.ndarray:
    ok = np.isin(seq, np.frombuffer(b"ACGTacgt", dtype=np.uint8))
    return np.where(ok, (seq & 14) >> 1, 5).astype(np.int64)


def strand_codes(seq: np.ndarray, K: int, k_low: int, mode: str) -> list:
    """the codes of the prepared read, one array of L codes per strand"""
    body, L, _ = geometry(seq.shape[0], K, k_low, mode)
    fwd = np.concatenate((codes_of(seq), np.full(body - seq.shape[0], 4, dtype=np.int64)))
    mark = np.full(L - body, 4, dtype=np.int64)
    out = [np.concatenate((fwd, mark))]
    if strands(mode) == 2:
        rev = fwd[::-1].copy()
        base = rev < 4
        rev[base] ^= 2
        out.append(np.concatenate((rev, mark)))
    return out


def letters_of(codes: np.ndarray, lut: np.ndarray) -> np.ndarray:
    """the letter from every position on (the last two positions have none)"""
    return lut[codes[:-2] * 64 + codes[1:-1] * 8 + codes[2:]].astype(np.uint64)


def protein_letters(seq: np.ndarray, K: int, k_low: int) -> np.ndarray:
    _, L, _ = geometry(seq.shape[0], K, k_low, "protein")
    s = np.concatenate((seq, np.full(L - seq.shape[0], ord("^"), dtype=np.uint8)))
    s = np.where(s == ord("*"), ord("["), s)
    return (s & 31).astype(np.uint64)


def pack(letters: np.ndarray, starts: np.ndarray, stride: int, K: int) -> np.ndarray:
    """keys of the windows that begin at `starts` and take K letters `stride` apart: u64, or KEY128_DTYPE for K = 25"""
    lo = np.zeros(starts.shape[0], dtype=np.uint64)
    hi = np.zeros(starts.shape[0], dtype=np.uint64)
    for j in range(K):
        x = letters[starts + j * stride]
        if K > 12:
            hi = (hi << np.uint64(5)) | (lo >> np.uint64(59))
        lo = (lo << np.uint64(5)) | x
    if K <= 12:
        return lo
    out = np.zeros(starts.shape[0], dtype=KEY128_DTYPE)
    out["lo"], out["hi"] = lo, hi
    return out


def sequence_keys(seq: np.ndarray, K: int, k_low: int, mode: str, lut: np.ndarray) -> np.ndarray:
    """the keys of one sequence in emission order: forward strand, then reverse, window by window"""
    _, _, cnt = geometry(seq.shape[0], K, k_low, mode)
    if cnt == 0:
        return np.zeros(0, dtype=KEY128_DTYPE if K > 12 else np.uint64)
    w = np.arange(cnt, dtype=np.int64)
    if mode == "protein":
        return pack(protein_letters(seq, K, k_low), w, 1, K)
    return np.concatenate([pack(letters_of(c, lut), w * (3 if mode == "one" else 1), 3, K) for c in strand_codes(seq, K, k_low, mode)])


def order_of(keys: np.ndarray) -> np.ndarray:
    """the stable ascending order of keys of either width"""
    if keys.dtype == KEY128_DTYPE:
        return np.lexsort((keys["lo"], keys["hi"]))
    return np.argsort(keys, kind="stable")


@dataclass
class Expected:
    keys: np.ndarray               # emission order
    read: np.ndarray               # u32: the read of every k-mer
    slot: np.ndarray               # u32 for a ranked case: the read's first k-mer + the k-mers of the read that sort before; else None
    seq_count: np.ndarray          # k-mers of every sequence (both strands)
    read_count: np.ndarray         # k-mers of every read


@functools.lru_cache(maxsize=None)
def _expected(name: str, lut_name: str) -> Expected:
    c = case(name)
    lut = table(lut_name)
    per_seq = [sequence_keys(s, c.K, c.k_low, c.mode, lut) for s in c.seqs]
    dt = KEY128_DTYPE if c.wide else np.uint64
    keys = np.concatenate(per_seq) if per_seq else np.zeros(0, dtype=dt)
    seq_count = np.array([k.shape[0] for k in per_seq], dtype=np.int64)
    seq_read = np.arange(len(c.seqs), dtype=np.uint32) if c.seg_read is None else np.asarray(c.seg_read, dtype=np.uint32)
    read = np.repeat(seq_read, seq_count).astype(np.uint32)
    read_count = np.bincount(seq_read, weights=seq_count, minlength=c.n_reads).astype(np.int64) if len(c.seqs) else np.zeros(c.n_reads, dtype=np.int64)
    slot = None
    if c.ranked:
        slot = np.zeros(keys.shape[0], dtype=np.uint32)
        first = 0
        for n in read_count:
            n = int(n)
            if n:
                slot[first + order_of(keys[first:first + n])] = first + np.arange(n, dtype=np.uint32)
            first += n
    for a in (keys, read, seq_count, read_count) + ((slot,) if slot is not None else ()):
        a.setflags(write=False)
    return Expected(keys, read, slot, seq_count, read_count)


def expected(c, lut: str = None) -> Expected:
    """The reference of a case (or of its name) under its own codon table or the named one; computed once, shared and read-only."""
    c = case(c) if isinstance(c, str) else c
    return _expected(c.name, lut or c.lut)


def dispatch(wide: bool, mode: str, segments: bool, debug: int, seq_count, read_count):
    """kasa_batch_encode's choice restated -> (form, encoder_ranked, long sequences listed for the second launch or None)."""
    longest = int(max(read_count)) if len(read_count) else 0
    ranked = (not segments) and longest <= ENC_RANK_MAX and not (debug & 8)
    if ranked:
        if not wide and longest <= ENC_GROUP_RM and mode == "dna3":
            return "group", 1, None
        return ("slots192" if longest <= SMALL_RM else "slots512"), 1, None
    if longest >= ENC_LONG_MIN:
        listed = int(sum(1 for n in seq_count if n >= ENC_LONG_MIN))
        return ("long" if listed else "readid"), 0, listed
    return "readid", 0, None


def group_parts(counts) -> list:
    """encode_group_kernel's parts of one group: as many consecutive reads as have at most CAPK k-mers together
    -> [(first read, end read, k-mers)]; a part without k-mers is skipped by the kernel but listed here"""
    parts, a = [], 0
    while a < len(counts):
        e = a + 1
        while e < len(counts) and sum(counts[a:e + 1]) <= CAPK:
            e += 1
        parts.append((a, e, sum(counts[a:e])))
        a = e
    return parts


def key_int(k) -> int:
    return (int(k["hi"]) << 64) | int(k["lo"]) if getattr(k, "dtype", None) == KEY128_DTYPE else int(k)


def describe_difference(c: Case, got: np.ndarray, want: np.ndarray) -> str:
    """where two key arrays first differ, for a failure message: read, strand, window, letter, both keys in hex"""
    if got.shape != want.shape:
        return "%d keys, %d expected" % (got.shape[0], want.shape[0])
    bad = np.flatnonzero(got != want)
    if not bad.shape[0]:
        return "equal"
    i = int(bad[0])
    e = expected(c)
    ends = np.cumsum(e.seq_count)
    s = int(np.searchsorted(ends, i, side="right"))
    within = i - int(ends[s] - e.seq_count[s])
    per = int(e.seq_count[s]) // strands(c.mode)
    g, w = key_int(got[i]), key_int(want[i])
    letter = next(j for j in range(c.K) if (g >> 5 * (c.K - 1 - j)) & 31 != (w >> 5 * (c.K - 1 - j)) & 31) if (g ^ w) >> 5 * c.K == 0 else -1
    return ("%d of %d keys differ, first at k-mer %d: sequence %d (read %d), strand %d, window %d of %d, letter %d (0 = first; -1: bits above the key): got %x, expected %x"
            % (bad.shape[0], want.shape[0], i, s, int(e.read[i]), within // per, within % per, per, letter, g, w))


# ------------------------------------------------------------------------------------------------
# the registry
# ------------------------------------------------------------------------------------------------
_BUILDERS = {}                                   # name -> (family, function that builds the case)
LARGE = set()                                    # cases of millions of bases: built only when asked for by name


def _add(name, family, build, large=False):
    assert name not in _BUILDERS, name
    _BUILDERS[name] = (family, build)
    if large:
        LARGE.add(name)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    family, build = _BUILDERS[name]
    c = build()
    c.name, c.family = name, family
    return c


def case_names(family=None, K=None, form=None, large=False):
    out = []
    for n, (f, _) in _BUILDERS.items():
        if (family is None or f == family) and (large or n not in LARGE):
            if (K is None and form is None) or ((K is None or case(n).K == K) and (form is None or case(n).form == form)):
                out.append(n)
    return out


def _rng(name: str):
    return np.random.default_rng(int.from_bytes(name.encode(), "little") % (1 << 63))


def filler(rng, n: int) -> np.ndarray:
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)]


def protein_filler(rng, n: int) -> np.ndarray:
    return np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)[rng.integers(0, 20, size=n)]


def any_filler(rng, n: int, mode: str) -> np.ndarray:
    return protein_filler(rng, n) if mode == "protein" else filler(rng, n)


def short_form(K: int, mode: str) -> str:
    """the form of a ranked batch whose reads have at most 192 k-mers"""
    return "group" if K == 12 and mode == "dna3" else "slots192"


def form_of_count(n: int, K: int, mode: str) -> str:
    """the form a batch takes whose longest read has n k-mers (one sequence per read, no debug flag)"""
    if n <= SMALL_RM:
        return short_form(K, mode)
    return "slots512" if n <= ENC_RANK_MAX else ("readid" if n < ENC_LONG_MIN else "long")


def driver(rng, form: str, K: int, k_low: int, mode: str, inner: np.ndarray = None, readid: int = 600) -> list:
    """A read that pushes a batch of short reads into `form`: 200 k-mers for the 512-k-mer ranking, 600 for the read id, ENC_LONG_MIN
    for the second launch; `inner` (if it fits) lies in its middle.  Nothing for the forms short reads take by themselves."""
    want = {"slots512": 200, "readid": readid, "long": ENC_LONG_MIN}.get(form)
    if want is None:
        return []
    raw = raw_for((want + strands(mode) - 1) // strands(mode), K, k_low, mode)
    if inner is not None and inner.shape[0] + 2 <= raw:
        a = (raw - inner.shape[0]) // 2
        return [np.concatenate((any_filler(rng, a, mode), inner, any_filler(rng, raw - a - inner.shape[0], mode)))]
    return [any_filler(rng, raw, mode)]


def _listed(form):
    return 1 if form == "long" else None


# ------------------------------------------------------------------------------------------------
# alphabet
# ------------------------------------------------------------------------------------------------
def all_values_stretch(f: np.ndarray) -> np.ndarray:
    """3072 bytes: element e = 0 .. 767 is the value e % 256 followed by three filler bases, so that every value stands at
    positions = 0, 1 and 2 (mod 3) (4 e = e mod 3, and 256 = 1 mod 3)"""
    out = np.tile(f[:4], 768).copy()
    out[::4] = np.arange(768) % 256
    return out


def _alphabet_dna(K, k_low, mode, form):
    def build():
        rng = _rng("alphabet %d %s %s" % (K, mode, form))
        seqs = []
        for v in range(256):                              # the value 3 K + r bases in, six bases before the read's end: in the last window
            for r in range(3):
                seqs.append(np.concatenate((filler(rng, 3 * K + r), [v], filler(rng, 5))))
        seqs.append(np.frombuffer(b"acgt", dtype=np.uint8)[rng.integers(0, 4, size=3 * K + 20)])
        seqs.append(np.frombuffer(b"NnXxZz-*.RYKM\x00\xff uU", dtype=np.uint8)[rng.integers(0, 18, size=3 * K + 20)])
        seqs += driver(rng, form, K, k_low, mode, all_values_stretch(filler(rng, 4)), readid=6400)
        return Case("", "", seqs, K, K, k_low, mode, "builtin", form, "every byte value as a base at each position mod 3, lower case, non-bases",
                    second_launch=_listed(form), claim={"value_reads": 768})
    return build


for _K in (12, 25):
    for _mode, _forms in (("dna3", ("group", "slots512", "readid", "long")), ("dna6", ("slots192", "slots512", "readid", "long")), ("one", ("slots192", "readid"))):
        for _form in _forms:
            _f = "slots192" if (_K == 25 and _form == "group") else _form
            _add("alphabet K%d %s %s" % (_K, _mode, _f), "alphabet", _alphabet_dna(_K, 7, _mode, _f))


def _alphabet_protein(K, form):
    def build():
        rng = _rng("alphabet protein %d %s" % (K, form))
        vals = np.arange(256, dtype=np.uint8)
        seqs = [np.concatenate((protein_filler(rng, K), vals[a:a + 64], protein_filler(rng, K))) for a in range(0, 256, 64)]
        seqs.append(np.concatenate((vals[::-1], vals)))
        seqs.append(np.frombuffer(b"*[^" * 20, dtype=np.uint8).copy())
        seqs.append(np.frombuffer(b"acdefghiklmnpqrstvwy" * 3, dtype=np.uint8).copy())
        return Case("", "", seqs, K, K, 7, "protein", "builtin", form, "every byte value as an amino-acid letter; '*', '[', '^', lower case",
                    debug=8 if form == "readid" else 0)
    return build


for _K in (12, 25):
    for _form in ("slots512", "readid"):
        _add("alphabet K%d protein %s" % (_K, _form), "alphabet", _alphabet_protein(_K, _form))


# ------------------------------------------------------------------------------------------------
# codons
# ------------------------------------------------------------------------------------------------
def _codons(K, k_low, mode, lut, form):
    def build():
        rng = _rng("codons %d %d %s" % (K, k_low, mode))
        triples = [(a, b, c) for a in NON_X for b in NON_X for c in NON_X]
        flank = 3 * K
        per = 9                                           # triples per read: 2 * 3 K + 27 bases, at most 192 k-mers in three frames even at K = 25, kLow = 1
        seqs = []
        for i in range(0, len(triples), per):
            mid = np.array([BASE_OF_CODE[x] for t in triples[i:i + per] for x in t], dtype=np.uint8)
            seqs.append(np.concatenate((filler(rng, flank), mid, filler(rng, flank))))
        for i, (a, b) in enumerate((a, b) for a in NON_X for b in NON_X):          # every pair before the marker, on both strands
            c, d = NON_X[(i // 5 + 2) % 5], NON_X[(i + 3) % 5]
            head = [BASE_OF_CODE[x ^ 2 if x < 4 else x] for x in (b, a)]           # the reverse strand ends with the complement of the start
            seqs.append(np.concatenate((head, filler(rng, flank + i % 3), [BASE_OF_CODE[c], BASE_OF_CODE[d]], [BASE_OF_CODE[a], BASE_OF_CODE[b]])).astype(np.uint8))
        seqs += driver(rng, form, K, k_low, mode)
        return Case("", "", seqs, K, K, k_low, mode, lut, form, "every reachable code triple on both strands at every letter of a key")
    return build


for _K in (12, 25):
    for _lut in ("telling", "builtin"):
        for _kl in ((7, 1, _K) if _lut == "telling" else (7,)):
            for _mode, _form in (("dna3", short_form(_K, "dna3")), ("dna6", "slots192"), ("dna6", "slots512"), ("dna6", "readid")):
                if (_form == "slots192" and _mode == "dna6" and (_K, _kl) != (12, 7)) or (_form == "readid" and _kl != 7):
                    continue                              # (six frames: only K = 12, kLow = 7 keeps these reads at 192 k-mers or fewer)
                _add("codons K%d kLow%d %s %s %s" % (_K, _kl, _mode, _form, _lut), "codons", _codons(_K, _kl, _mode, _lut, _form))


# ------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------
def _geometry(K, kh, kl, mode, which="all", shift=0):
    def build():
        rng = _rng("geometry %d %d %s" % (K, kl, mode))
        top = (K if mode == "protein" else 3 * K) + 8
        seqs = [any_filler(rng, n, mode) for n in range(top + 1)]
        short = [n for n in range(top + 1) if geometry(n, K, kl, mode)[2] == 0]
        if which == "first":
            seqs = [seqs[0], seqs[short[-1]]] + seqs[::-1]
        elif which == "last":
            seqs = seqs + [seqs[short[-1]], seqs[0]]
        elif which == "none":
            seqs = [seqs[n] for n in short]
        elif which == "one empty":
            seqs = [seqs[0]]
        return Case("", "", seqs, K, kh, kl, mode, "telling", short_form(K, mode), "every raw length from 0 to %d; %s" % (top, which), shift=shift)
    return build


for _K, _kh, _kl in GEOMETRIES:
    for _mode in MODES:
        _add("geometry K%d %d..%d %s" % (_K, _kh, _kl, _mode), "geometry", _geometry(_K, _kh, _kl, _mode))
for _K in (12, 25):
    for _mode in ("dna3", "dna6"):
        for _which in ("first", "last", "none", "one empty"):
            _add("geometry K%d %s %s without k-mers" % (_K, _mode, _which), "geometry", _geometry(_K, _K, 7, _mode, _which))
    _add("geometry K%d dna3 offsets from 21" % _K, "geometry", _geometry(_K, _K, 7, "dna3", shift=21))


# ------------------------------------------------------------------------------------------------
# packing
# ------------------------------------------------------------------------------------------------
def _packing(K, fill):
    def build():
        seqs = [np.array([64 + fill] * (K - 1) + [64 + v] + [64 + fill] * (K - 1), dtype=np.uint8) for v in range(32)]
        return Case("", "", seqs, K, K, K, "protein", "builtin", "slots192", "each of the 32 letter values at each of the %d letters, %d elsewhere" % (K, fill),
                    claim={"fill": fill})
    return build


for _K in (12, 25):
    for _fill in (21, 10):
        _add("packing K%d fill %d" % (_K, _fill), "packing", _packing(_K, _fill))


# ------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------
def _bounds(K, mode, per_strand, where="first"):
    n = per_strand * strands(mode)

    def build():
        rng = _rng("bounds %d %s %d" % (K, mode, per_strand))
        main = any_filler(rng, raw_for(per_strand, K, 7, mode), mode)
        small = [any_filler(rng, raw_for(c, K, 7, mode), mode) for c in (3, 40, 17)]
        seqs = [main] + small if where == "first" else small + [main]
        return Case("", "", seqs, K, K, 7, mode, "telling", form_of_count(n, K, mode), "one read of %d k-mers (%d windows a strand), %s in the batch" % (n, per_strand, where),
                    claim={"k-mers": n, "at": 0 if where == "first" else 3})
    return build


RANK_BOUNDS = (SMALL_RM - 1, SMALL_RM, SMALL_RM + 1, ENC_RANK_MAX - 1, ENC_RANK_MAX, ENC_RANK_MAX + 1)
CHUNK_COUNTS = (ENC_CHUNK - 1, ENC_CHUNK, ENC_CHUNK + 1, 2 * ENC_CHUNK, 2 * ENC_CHUNK + 1)
ONE_CHUNK = ENC_CHUNK // 3                        # const int chunk = (mode == ENC_ONE) ? ENC_CHUNK / 3 : ENC_CHUNK;
ONE_CHUNK_COUNTS = (ONE_CHUNK - 1, ONE_CHUNK, ONE_CHUNK + 1, 2 * ONE_CHUNK, 2 * ONE_CHUNK + 1)
for _K in (12, 25):
    for _n in sorted(set(RANK_BOUNDS + CHUNK_COUNTS)):
        _add("bounds K%d dna3 %d" % (_K, _n), "bounds", _bounds(_K, "dna3", _n))
    for _n in (SMALL_RM + 1, ENC_RANK_MAX + 1):
        _add("bounds K%d dna3 %d last" % (_K, _n), "bounds", _bounds(_K, "dna3", _n, "last"))
    for _n in sorted({SMALL_RM // 2 - 1, SMALL_RM // 2, SMALL_RM // 2 + 1, ENC_RANK_MAX // 2 - 1, ENC_RANK_MAX // 2, ENC_RANK_MAX // 2 + 1} | set(CHUNK_COUNTS)):
        _add("bounds K%d dna6 2x%d" % (_K, _n), "bounds", _bounds(_K, "dna6", _n))
    for _n in sorted(set(RANK_BOUNDS + ONE_CHUNK_COUNTS)):
        _add("bounds K%d one %d" % (_K, _n), "bounds", _bounds(_K, "one", _n))
    for _n in (SMALL_RM, SMALL_RM + 1, ENC_RANK_MAX, ENC_RANK_MAX + 1):
        _add("bounds K%d protein %d" % (_K, _n), "bounds", _bounds(_K, "protein", _n))


# ------------------------------------------------------------------------------------------------
# group_parts
# ------------------------------------------------------------------------------------------------
def split_lists() -> list:
    """Groups of ENC_GROUP counts: for every s at which a part can end before the group does ((s + 1) reads can exceed CAPK) the
    first s + 1 reads total CAPK - 1, CAPK (one part) and CAPK + 1 (the part ends behind read s), the long reads first and last."""
    out = []
    for s in range(1, ENC_GROUP):
        if (s + 1) * ENC_GROUP_RM <= CAPK:
            continue
        for total in (CAPK - 1, CAPK, CAPK + 1):
            last = total - s * ENC_GROUP_RM
            head = [ENC_GROUP_RM] * s
            if last < 3:                                  # (a read has no k-mer or at least three)
                head[-1] -= 3 - last
                last = 3
            g = head + [last]
            g += [5] * (ENC_GROUP - len(g))
            out += [g, g[:s + 1][::-1] + g[s + 1:]]
    return out


def _group_case(groups, why):
    def build():
        rng = _rng("group " + why)
        seqs = [filler(rng, raw_for(n, 12, 7, "dna3") if n else int(rng.choice([0, 1, 22]))) for g in groups for n in g]
        return Case("", "", seqs, 12, 12, 7, "dna3", "telling", "group", why, claim={"groups": [list(g) for g in groups]})
    return build


_add("group_parts totals", "group_parts", _group_case(split_lists() + [[ENC_GROUP_RM] * (ENC_GROUP - 1) + [3], [3] + [ENC_GROUP_RM] * (ENC_GROUP - 1), [ENC_GROUP_RM] * ENC_GROUP], "k-mers of a group around CAPK: where a part ends"))
_Z = [[0] + [130] * (ENC_GROUP - 1), [130] + [0] * (ENC_GROUP - 2) + [130], [130] * (ENC_GROUP - 1) + [0], [0] * ENC_GROUP, [0] * (ENC_GROUP - 1) + [ENC_GROUP_RM],
      [ENC_GROUP_RM] + [0] * (ENC_GROUP - 1), [ENC_GROUP_RM, 0] * (ENC_GROUP // 2) + [ENC_GROUP_RM] * (ENC_GROUP % 2)]
_add("group_parts zeros", "group_parts", _group_case(_Z, "reads without k-mers first, inside, last and throughout a group"))
for _r in range(1, ENC_GROUP):
    _add("group_parts tail %d" % _r, "group_parts", _group_case([[131] * ENC_GROUP, [130, 0, 64, 3, 192, 5, 77, 9, 11, 13, 15, 17, 19, 21, 23][:_r]], "a last group of %d reads" % _r))
    _add("group_parts only %d" % _r, "group_parts", _group_case([[ENC_GROUP_RM, 3, 0, 64, 65, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16][:_r]], "a batch of %d reads" % _r))
_add("group_parts many", "group_parts", _group_case([[3 + (7 * g + 5 * i) % 190 for i in range(ENC_GROUP)] for g in range(2 * ENC_WAVES + 3)],
                                                     "more groups than the wavefronts of one workgroup"))


# ------------------------------------------------------------------------------------------------
# ranking
# ------------------------------------------------------------------------------------------------
def block_letters(K: int, base: int, places: tuple, variants: list) -> list:
    """blocks of K letters, one per variant: `base` everywhere but the variant's letters at `places` (0 = first); a block more
    of `base` at the end.  The windows at the blocks' starts differ in those letters alone."""
    out = []
    for v in variants:
        b = [base] * K
        for p, x in zip(places, v):
            b[p] = x
        out += b
    return out + [base] * K


def ranking_patterns(K: int, letters: list) -> dict:
    """name -> (letter sequence, claim); `letters`: the letter values that may be used, ascending"""
    a = letters[len(letters) // 2]
    others = [x for x in letters if x != a]
    best = {}
    for r in range(4):                                                        # second letters with the same top bit and the same two low bits ...
        by = {}
        for x in letters:
            if x < 16 and x != a and x & 3 == r:
                by.setdefault((x >> 2) & 3, x)                                # ... one for every value of the two bits between: key bits 7-8 from the top
        best = by if len(by) > len(best) else best
    low2 = [best[q] for q in sorted(best)]
    pat = {
        "ascending": (sorted(letters * 2), "ascending"),
        "descending": (sorted(letters * 2, reverse=True), "descending"),
        "last letter": (block_letters(K, a, (K - 1,), [(x,) for x in others[:4]]), ("only", [K - 1])),
        "bits 7-8": (block_letters(K, a, (1,), [(x,) for x in low2]), ("bits78", [1])),
        "first letters": (list(letters) + [a] * K, "first"),
        "far pairs": (([a, others[0], others[1]] * K)[:K + 2] + others[2:8] * 3 + ([a, others[0], others[1]] * K)[:K + 2], "pairs"),
    }
    if K == 25:
        pat["letter 1"] = (block_letters(K, a, (0,), [(x,) for x in others[:5]]), ("only", [0]))
        mixed = [others[0], others[-1], others[1], others[-2], others[2], others[-3]]                # (letter 13 has key bit 64 as its top bit: both values)
        pat["letters 13-14"] = (block_letters(K, a, (12, 13), [(x, y) for x, y in zip(mixed[:5], mixed[1:])]), ("only", [12, 13]))
    return pat


def dna_of_letters(seq: list) -> np.ndarray:
    cod = codon_of_letter("telling")
    return np.array([b for x in seq for b in cod[x]], dtype=np.uint8)


def _ranking_dna(pattern, mode):
    def build():
        seq, claim = ranking_patterns(12, sorted(codon_of_letter("telling")))[pattern]
        return Case("", "", [dna_of_letters(seq), dna_of_letters(seq[::-1])], 12, 12, 12, mode, "telling", short_form(12, mode),
                    "k-mers of one read: %s (in the windows of frame 0)" % pattern, claim={"pattern": claim, "stride": 3 if mode == "dna3" else 1})
    return build


def _ranking_protein(K, pattern):
    def build():
        seq, claim = ranking_patterns(K, list(range(32)))[pattern]
        s = np.array([64 + x for x in seq], dtype=np.uint8)
        n = geometry(s.shape[0], K, K, "protein")[2]
        return Case("", "", [s, s[::-1].copy()], K, K, K, "protein", "builtin", form_of_count(n, K, "protein"), "k-mers of one read: %s" % pattern,
                    claim={"pattern": claim, "stride": 1})
    return build


def _ranking_equal(K, mode, n):
    def build():
        one = {"dna3": T, "dna6": A, "one": G, "protein": ord("K")}[mode]
        seqs = [np.full(raw_for(n // strands(mode), K, K, mode), one, dtype=np.uint8), np.full(raw_for(5, K, K, mode), one, dtype=np.uint8)]
        return Case("", "", seqs, K, K, K, mode, "telling", form_of_count(n, K, mode), "%d equal k-mers in one read: ranks in window order" % n, claim={"pattern": "equal", "stride": 1})
    return build


for _p in ("ascending", "descending", "last letter", "bits 7-8", "first letters", "far pairs"):
    _add("ranking K12 dna3 %s" % _p, "ranking", _ranking_dna(_p, "dna3"))
    _add("ranking K12 one %s" % _p, "ranking", _ranking_dna(_p, "one"))
    _add("ranking K12 protein %s" % _p, "ranking", _ranking_protein(12, _p))
for _p in ("ascending", "descending", "last letter", "bits 7-8", "first letters", "far pairs", "letter 1", "letters 13-14"):
    _add("ranking K25 protein %s" % _p, "ranking", _ranking_protein(25, _p))
_add("ranking K12 dna3 equal %d" % ENC_GROUP_RM, "ranking", _ranking_equal(12, "dna3", ENC_GROUP_RM))
_add("ranking K12 dna3 equal %d" % ENC_RANK_MAX, "ranking", _ranking_equal(12, "dna3", ENC_RANK_MAX))
_add("ranking K12 dna6 equal %d" % SMALL_RM, "ranking", _ranking_equal(12, "dna6", SMALL_RM))
_add("ranking K12 protein equal %d" % ENC_RANK_MAX, "ranking", _ranking_equal(12, "protein", ENC_RANK_MAX))
_add("ranking K25 dna3 equal %d" % SMALL_RM, "ranking", _ranking_equal(25, "dna3", SMALL_RM))
_add("ranking K25 protein equal %d" % ENC_RANK_MAX, "ranking", _ranking_equal(25, "protein", ENC_RANK_MAX))


# ------------------------------------------------------------------------------------------------
# segments
# ------------------------------------------------------------------------------------------------
def segment_sequences(K: int, mode: str):
    """-> sequences, the read of each, reads: read 0 two mates; 1 none; 2 one; 3 three, the middle one empty; 4 two mates too short
    alone that would have k-mers joined; 5 two mates whose junction would add k-mers; 6 an empty and a full mate; 7 none; 8 one"""
    rng = _rng("segments %d %s" % (K, mode))
    half = (3 * K + 2 - 3 * (K - 7)) // 2                 # two of these have k-mers together, one alone has none
    lens = [(0, 3 * K + 40), (0, 3 * K + 25), (2, 3 * K + 60), (3, 3 * K + 10), (3, 0), (3, 3 * K + 11), (4, half + 2), (4, half + 2),
            (5, 3 * K), (5, 3 * K + 1), (6, 0), (6, 3 * K + 30), (8, 100 + 3 * K)]
    seqs = [filler(rng, n) for _, n in lens]
    seqs[9][:3] = N                                       # (under the telling table Z and the marker's X give different letters: no window of
    return seqs, [r for r, _ in lens], 9                  #  the joined mates can equal the first mate's window of the same number by chance)


def _segments(K, mode, plain=False):
    def build():
        seqs, seg, n = segment_sequences(K, mode)
        if plain:
            return Case("", "", seqs, K, K, 7, mode, "telling", "readid", "the segments' sequences as reads of their own, the read id as payload (debug flag 8)", debug=8)
        return Case("", "", seqs, K, K, 7, mode, "telling", "readid", "reads of 0, 1, 2, 3 segments; no k-mer across a junction", seg_read=seg, n_reads=n,
                    claim={"too short alone": 4, "junction": 5})
    return build


for _K in (12, 25):
    for _mode in ("dna3", "dna6"):
        _add("segments K%d %s" % (_K, _mode), "segments", _segments(_K, _mode))
        _add("segments K%d %s as reads" % (_K, _mode), "segments", _segments(_K, _mode, True))


# ------------------------------------------------------------------------------------------------
# long
# ------------------------------------------------------------------------------------------------
def periodic(n: int, period: bytes, step: int) -> np.ndarray:
    """n bases of a short period with a substitution every `step` bases (the bases ACGT in turn) and one N"""
    s = np.resize(np.frombuffer(period, dtype=np.uint8), n).copy()
    at = np.arange(step // 2, n, step)
    s[at] = np.frombuffer(b"ACGT", dtype=np.uint8)[(at // step) % 4]
    s[n // 3] = N
    return s


def _long(K, mode, per_strand_list, why, kl=7, seg=False, large=False):
    def build():
        rng = _rng("long %d %s %s" % (K, mode, why))
        seqs = []
        for n in per_strand_list:
            raw = raw_for(n, K, kl, mode) if n else 0
            seqs.append(periodic(raw, b"ACGGTCATTGCA" + b"GATTACAGC", 997) if large else any_filler(rng, raw, mode))
        counts = [n * strands(mode) for n in per_strand_list]
        listed = sum(1 for n in counts if n >= ENC_LONG_MIN)
        longest = sum(counts) if seg else max(counts)
        return Case("", "", seqs, K, K, kl, mode, "telling", "long" if listed else "readid", why, second_launch=listed if longest >= ENC_LONG_MIN else None,
                    seg_read=[0] * len(seqs) if seg else None, n_reads=1 if seg else None, claim={"counts": counts})
    return build


for _d in (-1, 0, 1):
    _add("long K12 dna3 %d" % (ENC_LONG_MIN + _d), "long", _long(12, "dna3", [40, ENC_LONG_MIN + _d, 7], "a sequence of ENC_LONG_MIN %+d k-mers" % _d))
    _add("long K12 dna6 2x%d" % (ENC_LONG_MIN // 2 + _d), "long", _long(12, "dna6", [ENC_LONG_MIN // 2 + _d, 9], "two strands of ENC_LONG_MIN / 2 %+d k-mers" % _d))
_add("long K12 dna3 two", "long", _long(12, "dna3", [130, 0, ENC_LONG_MIN + 700, 131, 3, ENC_LONG_MIN + ENC_CHUNK, 192, 0],
                                        "two long sequences, short reads before, between and behind them"))
_add("long K25 dna3", "long", _long(25, "dna3", [11, ENC_LONG_MIN + 1300, 130], "a long sequence under 128-bit keys"))
_add("long K25 dna6", "long", _long(25, "dna6", [11, ENC_LONG_MIN // 2 + 77, 130], "a long sequence under 128-bit keys, both strands"))
_add("long K12 one", "long", _long(12, "one", [50, ENC_LONG_MIN + ONE_CHUNK + 1, 4], "a long sequence in one frame: chunks of ENC_CHUNK / 3 windows"))
_add("long K12 protein", "long", _long(12, "protein", [50, ENC_LONG_MIN + 5, 4], "a long amino-acid sequence"))
_add("long K25 protein", "long", _long(25, "protein", [50, ENC_LONG_MIN + 5, 4], "a long amino-acid sequence under 128-bit keys"))
_add("long K12 dna3 pair of 40000", "long", _long(12, "dna3", [40000, 40000], "a pair whose mates have 40 000 k-mers each: the read reaches ENC_LONG_MIN, no sequence does", seg=True))
_add("long K12 dna3 long mate", "long", _long(12, "dna3", [300, ENC_LONG_MIN + 3], "a pair whose second mate is a long sequence", seg=True))
_add("long K12 dna3 second sweep", "long", _long(12, "dna3", [LONG_SWEEP + ENC_CHUNK + 7, 150], "one sweep of the second launch's grid, a chunk and 7 windows: a wavefront comes round again", large=True),
     large=True)
