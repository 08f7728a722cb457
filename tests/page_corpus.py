"""Hand-made index partitions for the index pager (kasa_index_pager_load: page_prepare_kernel, then the taxon sort, the table's
running maximum and the trie check), with a plain restatement of what a slot must hold.  The inputs of
tests/test_page_cpu.py (which checks that the corpus is what it claims) and tests/test_gpu_page.py (which loads every case
into a slot and compares it with kasa_index_create's index).  Pure numpy on tests/lookup_corpus.py's helpers: no device.

A case is the records of one partition as they lie in its file (12, 20 or -- halved, K = 12 -- 6 bytes each), its `_trie`
arrays and its content.  The records are laid out by a string of kinds, one per record:

    P   the record opens a new 6-letter prefix (a new `_trie` entry)
    K   a new k-mer inside the entry
    T   the k-mer of the record before under the next taxon

T stands for the prepare kernel's tile (records per workgroup), LDS_TAXA for the most taxa whose table it searches on chip;
both restate kasa_pager.h's constants (test_page_cpu.py compares them with the library's).

Families:
  size     n = 1, 2, T - 1, T, T + 1, 2 T + 1 of the default layout
  edge     a key change, a taxon change and a prefix change on the last record of a tile (T - 1) and on the first of the next (T)
  forty    one k-mer under 40 taxa, 20 of them on either side of a tile edge
  taxa     LDS_TAXA and LDS_TAXA + 1 content entries, the records' taxa spread over all of them
  entries  (what the halved form walks; run in every form) an entry of one record at a tile's last and at its first record, one
           entry over three tiles, 1000 entries of one record inside one tile
  refusals unsorted, duplicate, a key bit beyond the width, an unknown tax ID, a taxon index == nTaxa (halved), a trie count
           off by one -- each at record 0, at a tile edge and at the last record
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from kasa_amd import formats
from tests import lookup_corpus as lc

T = 1024
LDS_TAXA = 7424
BITS = {12: 60, 25: 125}
FORMS = [("k12", 12, False), ("k25", 25, False), ("half", 12, True)]          # (name, letters, halved)


@dataclass
class Case:
    name: str
    K: int
    halved: bool
    keys: list                   # Python integers, as the records give them
    taxid: np.ndarray            # u32: tax IDs as the file holds them (halved: content.taxids[tix])
    tix: np.ndarray              # halved: the u16 taxon indices of the file
    low: np.ndarray              # halved: the u32 low words of the file
    trie_prefix: np.ndarray
    trie_count: np.ndarray
    content: formats.Content
    kinds: str = ""
    refusal: str = ""            # a phrase of the message kasa_index_create refuses the case with; "": a good case

    @property
    def n(self) -> int:
        return len(self.keys)

    @property
    def record_bytes(self) -> int:
        return 6 if self.halved else (12 if self.K == 12 else 20)

    def records(self) -> np.ndarray:
        """the partition as it lies in its file"""
        if self.halved:
            rec = np.zeros(self.n, dtype=formats.HALF_DTYPE)
            rec["low"], rec["tax"] = self.low, self.tix
        elif self.K == 12:
            rec = np.zeros(self.n, dtype=formats.REC_DTYPE)
            rec["kmer"], rec["tax"] = np.array(self.keys, dtype=np.uint64), self.taxid
        else:
            rec = np.zeros(self.n, dtype=formats.REC128_DTYPE)
            km = lc.keys_from_ints(self.keys, True)
            rec["lo"], rec["hi"], rec["tax"] = km["lo"], km["hi"], self.taxid
        return rec


# ------------------------------------------------------------------------------------------------
# layout
# ------------------------------------------------------------------------------------------------
def default_kinds(n: int) -> str:
    return "".join("P" if i % 301 == 0 else ("T" if i % 7 == 3 else "K") for i in range(n))


def put(kinds: str, at: int, what: str) -> str:
    return kinds[:at] + what + kinds[at + len(what):]


def lay_out(name: str, K: int, halved: bool, kinds: str, n_taxa: int = lc.N_TAXA, spread: bool = False) -> Case:
    """kinds -> records: prefix number p (from 1), k-mer number c inside the prefix; key = p in the upper 30 bits, c * 37 in
    the low ones -- neighbours share every number of letters from 6 up; the taxon of a P or K record is one of the first five
    (spread: any but the last 41), a T record takes the next."""
    assert kinds and kinds[0] == "P"
    c = lc.content(n_taxa)
    keys, tix, pre, cnt = [], [], [], []
    p = cc = t = 0
    for i, kind in enumerate(kinds):
        if kind == "P":
            p, cc = p + 1, 0
            pre.append(p * 3); cnt.append(0)
        elif kind == "K":
            cc += 1
        if kind == "T":
            t += 1
        else:
            t = 1 + ((i * 2654435761) % (n_taxa - 42) if spread else i % 5)
        assert t < n_taxa
        keys.append(((p * 3) << (5 * (K - 6))) | (cc * 37))
        tix.append(t)
        cnt[-1] += 1
    tix = np.array(tix, dtype=np.int64)
    return Case(name, K, halved, keys, c.taxids[tix].astype(np.uint32), tix.astype(np.uint16), np.array([k & 0x3FFFFFFF for k in keys], dtype=np.uint32),
                np.array(pre, dtype=np.uint32), np.array(cnt, dtype=np.uint64), c, kinds)


SIZES = [1, 2, T - 1, T, T + 1, 2 * T + 1]
EDGES = [(kind, at) for kind in "KTP" for at in (T - 1, T)]


def _good(form: str, K: int, halved: bool) -> dict:
    b = {}
    for n in SIZES:
        b["%s size %d" % (form, n)] = functools.partial(lay_out, "%s size %d" % (form, n), K, halved, default_kinds(n))
    for kind, at in EDGES:
        # the records around the edge are plain k-mer changes, the one named is of the kind named
        kinds = put(put(default_kinds(T + 40), T - 3, "KKKKKK"), at, kind)
        b["%s edge %s at %d" % (form, kind, at)] = functools.partial(lay_out, "%s edge %s at %d" % (form, kind, at), K, halved, kinds)
    b["%s forty" % form] = functools.partial(lay_out, "%s forty" % form, K, halved, put(default_kinds(T + 60), T - 20, "K" + "T" * 39 + "K"))
    for n_taxa in (LDS_TAXA, LDS_TAXA + 1):
        b["%s taxa %d" % (form, n_taxa)] = functools.partial(lay_out, "%s taxa %d" % (form, n_taxa), K, halved, default_kinds(T + 1), n_taxa, True)
    b["%s entries of one" % form] = functools.partial(lay_out, "%s entries of one" % form, K, halved, put(default_kinds(T + 40), T - 2, "KPPPK"))
    three = "P" + "K" * (T - 6) + "P" + "K" * (T + 9) + "P" + "K" * (T + 4)
    b["%s entry over three tiles" % form] = functools.partial(lay_out, "%s entry over three tiles" % form, K, halved, three)
    b["%s 1000 entries in a tile" % form] = functools.partial(lay_out, "%s 1000 entries in a tile" % form, K, halved, put(default_kinds(2 * T + 1), T + 10, "P" * 1000))
    return b


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
NOT_SORTED = "the index is not sorted by (kmer, taxid), not unique, or uses more than"
UNKNOWN_TAX = "carry a tax ID the content file does not know"
BAD_TIX = "names taxon index"
TRIE_DIFFERS = "the trie file does not match the index"
REFUSAL_N = 2 * T + 1
PLACES = {"record 0": 0, "tile edge": T, "last record": REFUSAL_N - 1}


def _refusal_base(name, K, halved) -> Case:
    kinds = default_kinds(REFUSAL_N)
    for at in (0, T - 2, REFUSAL_N - 4):                       # plain k-mer changes around the three places, all inside one entry
        kinds = put(kinds, at, "KKKK")
    return lay_out(name, K, halved, "P" + kinds[1:])


def _set_key(c: Case, i: int, key: int):
    c.keys[i] = key
    c.low[i] = key & 0x3FFFFFFF


def refusal(name: str, K: int, halved: bool, what: str, place: str) -> Case:
    c = _refusal_base(name, K, halved)
    at = PLACES[place]
    if what == "unsorted":                                      # the record is out of order against a neighbour (inside its entry)
        _set_key(c, at, c.keys[1] + 1 if at == 0 else c.keys[at - 1] - 1)
        c.refusal = NOT_SORTED
    elif what == "duplicate":                                   # the record equals its neighbour
        src = 1 if at == 0 else at - 1
        _set_key(c, at, c.keys[src])
        c.taxid[at], c.tix[at] = c.taxid[src], c.tix[src]
        c.refusal = NOT_SORTED
    elif what == "wide":                                        # a key bit beyond the width (the full forms only)
        c.keys[at] |= 1 << BITS[K]
        c.refusal = NOT_SORTED
    elif what == "unknown":                                     # a tax ID the content does not list (the full forms only)
        c.taxid[at] = 7
        c.refusal = UNKNOWN_TAX
    elif what == "tix":                                         # the halved form's taxon index one past the content
        c.tix[at] = c.content.n_taxa
        c.refusal = BAD_TIX
    elif what == "trie":                                        # a count off by one, the sum kept: the entry of the record grows, a neighbour shrinks
        e = int(np.searchsorted(np.cumsum(c.trie_count.astype(np.int64)), at, side="right"))
        other = e + 1 if e + 1 < c.trie_count.shape[0] else e - 1
        c.trie_count[e] += 1
        c.trie_count[other] -= 1
        c.refusal = NOT_SORTED if halved else TRIE_DIFFERS      # (halved: the moved record takes the other entry's prefix)
    else:
        raise KeyError(what)
    return c


def _refusals(form: str, K: int, halved: bool) -> dict:
    b = {}
    kinds = ["unsorted", "duplicate", "trie"] + (["tix"] if halved else ["wide", "unknown"])
    for what in kinds:
        for place in PLACES:
            name = "%s refused %s at %s" % (form, what, place)
            b[name] = functools.partial(refusal, name, K, halved, what, place)
    return b


_GOOD, _REFUSED = {}, {}
for _form, _K, _halved in FORMS:
    _GOOD.update(_good(_form, _K, _halved))
    _REFUSED.update(_refusals(_form, _K, _halved))


def good_names() -> list:
    return list(_GOOD)


def refusal_names() -> list:
    return list(_REFUSED)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    return (_GOOD.get(name) or _REFUSED[name])()


# ------------------------------------------------------------------------------------------------
# the restatement: what a slot (and kasa_index_create's index) holds
# ------------------------------------------------------------------------------------------------
def full_keys(c: Case) -> list:
    """the k-mers as integers; the halved form's from the low words and the entries' prefixes"""
    if not c.halved:
        return list(c.keys)
    pre = np.repeat(c.trie_prefix.astype(np.uint64), c.trie_count.astype(np.int64))
    return ((pre << np.uint64(30)) | (c.low.astype(np.uint64) & np.uint64(0x3FFFFFFF))).tolist()


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """(keys as the library's array, dense taxa u32, meta u8 / u16, table u32[2^tb], tb) of a good case"""
    c = case(name)
    keys, n, K = full_keys(c), c.n, c.K
    dense = formats.dense_tax(c.content.taxids[c.tix.astype(np.int64)] if c.halved else c.taxid, c.content)
    shift = 4 if K == 12 else 8
    meta, last = np.zeros(n, dtype=np.uint32), {}
    for i, k in enumerate(keys):
        prev = lc.shared_letters(keys[i - 1], k, K) if i else 0
        t = int(dense[i])
        dup = lc.shared_letters(keys[last[t]], k, K) if t in last else 0
        last[t] = i
        meta[i] = prev | (dup << shift)
    tb = lc.table_bits(n)
    buckets = np.array([k >> (BITS[K] - tb) for k in keys], dtype=np.int64)
    table = np.searchsorted(buckets, np.arange(1 << tb, dtype=np.int64), side="right").astype(np.uint32)
    return lc.keys_from_ints(keys, K > 12), dense.astype(np.uint32), meta.astype(np.uint8 if K == 12 else np.uint16), table, tb


def violations(c: Case) -> dict:
    """what kasa_index_create's checks count in a case, record by record"""
    keys, K = full_keys(c) if c.refusal != BAD_TIX else None, c.K
    out = {"order": 0, "unknown": 0, "tix": int((c.tix.astype(np.int64) >= c.content.n_taxa).sum()) if c.halved else 0}
    if keys is None:
        return out
    ids = c.content.taxids[np.minimum(c.tix.astype(np.int64), c.content.n_taxa - 1)] if c.halved else c.taxid
    known = set(c.content.taxids.tolist())
    for i in range(c.n):
        if i and (keys[i - 1] > keys[i] or (keys[i - 1] == keys[i] and ids[i - 1] >= ids[i]) or keys[i] >> BITS[K]):
            out["order"] += 1
        out["unknown"] += int(ids[i]) not in known
    return out


def trie_describes(c: Case) -> bool:
    """trie_check_kernel's rule: every entry is the whole run of records with its prefix"""
    keys, K = full_keys(c), c.K
    pre = [k >> (5 * (K - 6)) for k in keys]
    at = 0
    for p, cnt in zip(c.trie_prefix.tolist(), c.trie_count.tolist()):
        run = pre[at:at + cnt]
        if cnt == 0 or any(x != p for x in run) or (at and pre[at - 1] >= p) or (at + cnt < len(pre) and pre[at + cnt] <= p):
            return False
        at += cnt
    return at == len(pre)
