"""`update | delete | shrink | getFrequency` on the device (kasa_amd/csrc/kasa_edit.h behind kasa_build_add_index / drop_taxa /
shrink): the C++ host writes the reference's own files byte for byte (tests/golden/dbedit/), an update equals a build of the
union, and capi.Builder's filters equal numpy's on random indices."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from kasa_amd import build as hipbuild, capi, formats, index_edit
from tests import helpers

pytestmark = pytest.mark.gpu

SUFFIXES = ("", "_trie", "_trie.txt", "_info.txt", "_f.txt")
DBINDEX = os.path.join(helpers.GOLDEN, "dbindex")
DBEDIT = os.path.join(helpers.GOLDEN, "dbedit")
PAIRS = os.path.join(helpers.GOLDEN, "pairs")


def _host(args, tmp_path, env=None, ok=True):
    exe = hipbuild.build_host()
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([exe] + args + ["-m", "4", "-n", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                       cwd=str(tmp_path), env=e)
    if ok:
        assert r.returncode == 0, r.stdout + r.stderr
    return r


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _copy(src, dst, pad=0):
    for s in SUFFIXES:
        shutil.copyfile(src + s, dst + s)
    if pad:                                                              # the zero padding the reference's STXXL writes
        size = os.path.getsize(dst)
        with open(dst, "ab") as f:
            f.write(b"\0" * ((size + pad - 1) // pad * pad - size + pad))


def _same(new, ref, skip=()):
    for s in SUFFIXES:
        if s not in skip:
            assert _read(new + s) == _read(ref + s), s


OLD = {"update64": os.path.join(DBINDEX, "headers", "idx"), "update128": os.path.join(DBEDIT, "update128", "old"),
       "update_one": os.path.join(DBINDEX, "one", "idx")}


@pytest.mark.parametrize("case", ["update64", "update128", "update_one"])
@pytest.mark.parametrize("pad", [0, 2 << 20])
def test_cpp_update_fixtures(case, pad, tmp_path):
    d = os.path.join(DBEDIT, case)
    _copy(OLD[case], str(tmp_path / "old"), pad)
    _host(["update", "-d", str(tmp_path / "old"), "-o", str(tmp_path / "n"), "-i", os.path.join(d, "new.fasta"), "-c", os.path.join(d, "content.txt")]
          + (["--one"] if case == "update_one" else []), tmp_path)
    _same(str(tmp_path / "n"), os.path.join(d, "idx"))


def test_cpp_update_in_place(tmp_path):
    d = os.path.join(DBEDIT, "update64")
    _copy(OLD["update64"], str(tmp_path / "x"))
    _host(["update", "-d", str(tmp_path / "x"), "-i", os.path.join(d, "new.fasta"), "-c", os.path.join(d, "content.txt")], tmp_path,
          {"KASA_BUILD_BRICK_PAIRS": "300"})
    _same(str(tmp_path / "x"), os.path.join(d, "idx"))
    assert sorted(os.listdir(tmp_path)) == sorted("x" + s for s in SUFFIXES)


def test_cpp_update_unknown_taxon_leaves_the_index(tmp_path):
    """A content file without one of the old index's taxa: refused while loading, nothing written, the old index intact."""
    d = os.path.join(DBEDIT, "update64")
    _copy(OLD["update64"], str(tmp_path / "x"))
    c = tmp_path / "c.txt"
    c.write_text("".join(l for l in open(os.path.join(d, "content.txt")) if not l.startswith("Other\t")))
    r = _host(["update", "-d", str(tmp_path / "x"), "-i", os.path.join(d, "new.fasta"), "-c", str(c)], tmp_path, ok=False)
    assert r.returncode == 1 and r.stderr.startswith("ERROR: ") and "tax ID 77" in r.stderr, r.stderr
    _same(str(tmp_path / "x"), OLD["update64"])
    assert sorted(os.listdir(tmp_path)) == sorted(["c.txt"] + ["x" + s for s in SUFFIXES])


@pytest.mark.parametrize("case,old,content", [("delete64", os.path.join(DBINDEX, "multiline", "idx"), os.path.join(DBINDEX, "multiline", "content.txt")),
                                              ("delete128", OLD["update128"], os.path.join(DBINDEX, "headers", "content.txt"))])
def test_cpp_delete_fixtures(case, old, content, tmp_path):
    d = os.path.join(DBEDIT, case)
    _copy(old, str(tmp_path / "old"), 2 << 20)
    _host(["delete", "-d", str(tmp_path / "old"), "-o", str(tmp_path / "n"), "-l", os.path.join(d, "delnodes.dmp"), "-c", content], tmp_path)
    if case == "delete128":                                              # the reference's own _info.txt lacks the "128" line
        _same(str(tmp_path / "n"), os.path.join(d, "idx"), skip=("_info.txt",))
        assert _read(str(tmp_path / "n_info.txt")) == _read(os.path.join(d, "idx_info.txt")) + b"\n128"
    else:
        _same(str(tmp_path / "n"), os.path.join(d, "idx"))


def test_cpp_delete_onto_itself(tmp_path):
    d = os.path.join(DBEDIT, "delete64")
    _copy(os.path.join(DBINDEX, "multiline", "idx"), str(tmp_path / "x"))
    _host(["delete", "-d", str(tmp_path / "x"), "-o", str(tmp_path / "x"), "-l", os.path.join(d, "delnodes.dmp"), "-c",
           os.path.join(DBINDEX, "multiline", "content.txt")], tmp_path)
    _same(str(tmp_path / "x"), os.path.join(d, "idx"))


def test_cpp_delete_every_taxon_leaves_an_empty_index(tmp_path):
    """delnodes lists every taxon of the small halved_pads database: no record is left, which `build` refuses and an edit writes --
    a records file of 0 bytes, _info.txt = 0, an empty _trie, _trie.txt = 0, exit status 0."""
    d = os.path.join(DBEDIT, "halved_pads")
    content, delnodes = tmp_path / "c.txt", tmp_path / "delnodes.dmp"
    content.write_text("ProtA\t21\t21\tP0.1;P2.1\nProtB\t22\t22\tP1.1;P3.1;P5.1\nProtC\t23\t23\tP4.1\n")
    delnodes.write_text("21\t|\n22\t|\n23\t|\n")
    assert int(_read(os.path.join(d, "idx_info.txt"))) > 0
    r = _host(["delete", "-d", os.path.join(d, "idx"), "-o", str(tmp_path / "n"), "-l", str(delnodes), "-c", str(content)], tmp_path)
    assert r.returncode == 0 and "OUT: Index: 0 entries, trie: 0 entries" in r.stdout, r.stdout
    assert _read(str(tmp_path / "n")) == b"" and _read(str(tmp_path / "n_info.txt")) == b"0"
    assert _read(str(tmp_path / "n_trie")) == b"" and _read(str(tmp_path / "n_trie.txt")) == b"0"
    assert sorted(os.listdir(tmp_path)) == sorted(["c.txt", "delnodes.dmp"] + ["n" + s for s in SUFFIXES])


SHRINK = [("s1_30", "update64", ["-s", "1", "-g", "30"]), ("s1_333", "update64", ["-s", "1", "-g", "33.3"]),
          ("s1_150", "update64", ["-s", "1", "-g", "150"]), ("s1_333w", "update128", ["-s", "1", "-g", "33.3"]),
          ("s3", "update64", ["-s", "3"]), ("s3w", "update128", ["-s", "3"])]


@pytest.mark.parametrize("name,src,args", SHRINK)
def test_cpp_shrink_fixtures(name, src, args, tmp_path):
    _copy(os.path.join(DBEDIT, src, "idx"), str(tmp_path / "in"))
    _host(["shrink", "-d", str(tmp_path / "in"), "-o", str(tmp_path / "n"), "-c", os.path.join(DBEDIT, src, "content.txt")] + args, tmp_path,
          {"KASA_EDIT_CHUNK_RECORDS": "1000"} if name == "s1_333" else None)
    _same(str(tmp_path / "n"), os.path.join(DBEDIT, "shrink", name))


def test_cpp_shrink_fivecol_and_default_content(tmp_path):
    _copy(os.path.join(DBINDEX, "fivecol", "idx"), str(tmp_path / "in"))
    _host(["shrink", "-d", str(tmp_path / "in"), "-o", str(tmp_path / "n"), "-c", os.path.join(DBINDEX, "fivecol", "content.txt"), "-s", "3"], tmp_path)
    _same(str(tmp_path / "n"), os.path.join(DBEDIT, "shrink", "s3_five"))
    _copy(os.path.join(DBEDIT, "update64", "idx"), str(tmp_path / "m"))
    shutil.copyfile(os.path.join(DBEDIT, "update64", "content.txt"), str(tmp_path / "m_content.txt"))
    _host(["shrink", "-d", str(tmp_path / "m"), "-s", "3"], tmp_path)
    _same(str(tmp_path / "m_s"), os.path.join(DBEDIT, "shrink", "s_noc"))
    assert _read(str(tmp_path / "m_s_content.txt")) == _read(os.path.join(DBEDIT, "shrink", "s_noc_content.txt"))


def test_cpp_shrink_halved_equals_pairs_idx_half(tmp_path):
    _copy(os.path.join(PAIRS, "idx"), str(tmp_path / "in"), 2 << 20)
    _host(["shrink", "-d", str(tmp_path / "in"), "-o", str(tmp_path / "h"), "-c", os.path.join(PAIRS, "content.txt"), "-s", "2"], tmp_path)
    _same(str(tmp_path / "h"), os.path.join(PAIRS, "idx_half"))


def test_cpp_shrink_everything_refused(tmp_path):
    _copy(os.path.join(DBEDIT, "update64", "idx"), str(tmp_path / "in"))
    r = _host(["shrink", "-d", str(tmp_path / "in"), "-o", str(tmp_path / "n"), "-c", os.path.join(DBEDIT, "update64", "content.txt"), "-s", "1", "-g", "100"],
              tmp_path, ok=False)
    assert r.returncode == 1 and r.stderr.startswith("ERROR: ") and "leaves no record" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == sorted("in" + s for s in SUFFIXES)


def test_cpp_get_frequency(tmp_path):
    _copy(os.path.join(DBEDIT, "update64", "idx"), str(tmp_path / "gf"))
    (tmp_path / "gf_f.txt").write_text("stale\n")
    _host(["getFrequency", "-d", str(tmp_path / "gf"), "-c", os.path.join(DBEDIT, "update64", "content.txt")], tmp_path)
    assert _read(str(tmp_path / "gf_f.txt")) == _read(os.path.join(DBEDIT, "getfreq", "idx_f.txt"))


# ---- properties: update(build(A), B) == build(A u B) ---------------------------------------------------------------------

def _genomes(seed, n_taxa, per_taxon, length):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    pool = rng.choice(acgt, 20000)
    seqs, tax = [], []
    for t in range(n_taxa):
        for _ in range(per_taxon):
            x = rng.choice(acgt, length)
            p = int(rng.integers(0, length - 3000))                      # a stretch shared with other taxa
            q = int(rng.integers(0, pool.shape[0] - 3000))
            x[p:p + 3000] = pool[q:q + 3000]
            seqs.append(x)
            tax.append(1000 + t)
    return seqs, np.asarray(tax, np.uint32)


def _pack(seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([s.shape[0] for s in seqs], out=off[1:])
    return np.concatenate(seqs), off


def _build(taxids, seqs, tax, K, brick=0):
    b = capi.Builder(taxids, K, 3, None, brick)
    try:
        bases, off = _pack(seqs)
        b.add(bases, off, tax)
        b.finish()
        return b.fetch()
    finally:
        b.close()


@pytest.mark.parametrize("K", [12, 25])
@pytest.mark.parametrize("shape", ["one_brick", "bricks", "chunks"])
def test_update_equals_build_of_the_union(K, shape):
    seqs, tax = _genomes(5 + K, 12, 2, 90_000)                           # ~2 Mbp
    taxids = np.concatenate(([0], np.unique(tax))).astype(np.uint32)
    half = len(seqs) // 2
    a_seqs, b_seqs = seqs[:half] + seqs[half + 3:half + 5], seqs[half:]  # B repeats sequences of A: duplicates to drop
    a_tax, b_tax = np.concatenate((tax[:half], tax[half + 3:half + 5])), tax[half:]
    km, tid, tp, tc, freq = _build(taxids, a_seqs, a_tax, K)
    rec = np.zeros(km.shape[0], dtype=formats.REC128_DTYPE if K == 25 else formats.REC_DTYPE)
    if K == 25:
        rec["lo"], rec["hi"] = km["lo"], km["hi"]
    else:
        rec["kmer"] = km
    rec["tax"] = tid
    b = capi.Builder(taxids, K, 3, None, 200_000 if shape == "bricks" else 0)
    try:
        bases, off = _pack(b_seqs)
        b.add(bases, off, b_tax)
        b.add_index(rec, 7777 if shape == "chunks" else 0)
        b.finish()
        got = b.fetch()
        st, es = b.stats(), b.edit_stats()
    finally:
        b.close()
    want = _build(taxids, seqs, tax, K)
    assert es["index_in"] == rec.shape[0] and es["dropped_delete"] == 0 and es["dropped_shrink"] == 0
    if shape == "bricks":
        assert st["bricks"] > 1
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ---- differential against numpy on random indices -----------------------------------------------------------------------

def _random_index(seed, n, n_taxa, K):
    rng = np.random.default_rng(seed)
    taxids = np.concatenate(([0], rng.choice(np.arange(1, 10 ** 7, dtype=np.uint32), n_taxa - 1, replace=False))).astype(np.uint32)
    letters = rng.integers(0, 26, size=(n, K), dtype=np.uint64)
    pad = rng.integers(0, K, size=n)                                     # a trailing '^' run on some records
    letters[np.arange(K)[None, :] >= (K - pad[:, None] * (rng.random(n) < 0.2)[:, None])] = 30
    lo = np.zeros(n, np.uint64)
    hi = np.zeros(n, np.uint64)
    for j in range(K):                                                   # letter j from the left: bits 5 (K - 1 - j)
        s = 5 * (K - 1 - j)
        if s < 64:
            lo |= letters[:, j] << np.uint64(s)
            if s + 5 > 64:
                hi |= letters[:, j] >> np.uint64(64 - s)
        else:
            hi |= letters[:, j] << np.uint64(s - 64)
    tid = taxids[1 + rng.integers(0, n_taxa - 1, size=n)]
    if K == 25:
        km = np.zeros(n, formats.KEY128_DTYPE)
        km["lo"], km["hi"] = lo, hi
    else:
        km = lo
    content = formats.Content(["non_unique"] + ["T%d" % i for i in range(1, n_taxa)], taxids)
    ix = formats.make_index(km, tid, content)
    return ix


def _model(ix, keep):
    km, tid = ix.kmer[keep], ix.taxid[keep]
    tax = formats.dense_tax(tid, ix.content)
    tp, tc = formats.trie_from_kmers(km)
    return km, tid, tp, tc, formats.freq_from_index(km, tax, ix.content.n_taxa)


def _ordinals(tax):
    """1-based ordinal of every record within its taxon, in index order"""
    order = np.argsort(tax, kind="stable")
    st = tax[order]
    first = np.searchsorted(st, st, side="left")
    out = np.empty(tax.shape[0], np.int64)
    out[order] = np.arange(tax.shape[0]) - first + 1
    return out


def _check(got, want):
    for name, g, w in zip(("kmer", "taxid", "trie_prefix", "trie_count", "freq"), (got.kmer, got.taxid, got.trie_prefix, got.trie_count, got.freq), want):
        assert np.array_equal(g, w), name


@pytest.mark.parametrize("K", [12, 25])
@pytest.mark.parametrize("n,n_taxa", [(120_000, 30), (400_000, 50_000), (1_000_000, 900)])
def test_edits_against_numpy(K, n, n_taxa, monkeypatch):
    ix = _random_index(n + K + n_taxa, n, n_taxa, K)
    rng = np.random.default_rng(n_taxa)
    # delete: a random drop set with IDs the index does not hold
    drop = np.concatenate((rng.choice(ix.content.taxids[1:], max(1, n_taxa // 7), replace=False), [4_000_000_000, 7]))
    got = index_edit.delete_taxa(ix, drop, chunk=n // 3 + 1)
    _check(got, _model(ix, ~np.isin(ix.taxid, drop)))
    assert got.edit_stats["dropped_delete"] == ix.n - got.n and got.edit_stats["index_in"] == ix.n
    # shrink 1: random float percentages, the carry between chunks forced
    monkeypatch.setenv("KASA_EDIT_CHUNK_RECORDS", str(n // 5 + 13))
    for P in (float(np.float32(rng.uniform(1, 99))), -float(np.float32(rng.uniform(1, 99))), 150.0):
        ords = _ordinals(ix.tax)
        table = index_edit.shrink_thresholds(P, int(ords.max()))
        got = index_edit.shrink_index(ix, 1, P)
        _check(got, _model(ix, ~np.isin(ords, table.astype(np.int64))))
    monkeypatch.delenv("KASA_EDIT_CHUNK_RECORDS")
    # shrink 3: entropy
    letters = np.stack([(formats.key_shr(ix.kmer, 5 * j) & np.uint64(31)).astype(np.int64) for j in range(K)], axis=1)
    counts = np.stack([(letters == c).sum(axis=1) for c in range(32)], axis=1)
    p = counts / K
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -np.where(counts > 0, p * np.log2(np.where(counts > 0, p, 1)), 0).sum(axis=1)
    got = index_edit.shrink_index(ix, 3)
    _check(got, _model(ix, h * np.log(2) / np.log(22) > 0.5))
    # shrink 2 (64-bit): the halved records
    if K == 12:
        got = index_edit.shrink_index(ix, 2)
        keep = (ix.kmer & np.uint64(0x3FFFFFFF)) != np.uint64(1039104990)   # six '^' (Shrink.hpp:108)
        km, tid, tp, tc, _ = _model(ix, keep)
        assert np.array_equal(got.kmer, km) and np.array_equal(got.taxid, tid) and np.array_equal(got.trie_count, tc)
        assert np.array_equal(got.freq, ix.freq)


def test_unsorted_and_duplicate_input_refused():
    ix = _random_index(3, 50_000, 40, 12)
    rec = index_edit._records(ix)
    for bad in ("swap", "dup", "unknown"):
        r = rec.copy()
        i = 31_000
        if bad == "swap":
            r[i], r[i + 1] = rec[i + 1], rec[i]
        elif bad == "dup":
            r[i + 1] = r[i]
        else:
            r[i]["tax"] = 123_456_789
        b = capi.Builder(ix.content.taxids, 12)
        try:
            with pytest.raises(RuntimeError) as e:
                b.add_index(r, 20_000)                                   # the bad record in the second chunk
            want = {"swap": "record %d " % (i + 1), "dup": "record %d " % (i + 1), "unknown": "record %d has tax ID 123456789" % i}[bad]
            assert want in str(e.value), str(e.value)
        finally:
            b.close()
    # the break between two chunks
    r = rec.copy()
    r[20_000] = rec[19_999]
    b = capi.Builder(ix.content.taxids, 12)
    try:
        with pytest.raises(RuntimeError, match="record 20000 "):
            b.add_index(r, 20_000)
    finally:
        b.close()


# ---- entropy: every multiset of letters --------------------------------------------------------------------------------

def _partitions(n, most=None):
    most = n if most is None else most
    if n == 0:
        yield []
        return
    for k in range(min(n, most), 0, -1):
        for rest in _partitions(n - k, k):
            yield [k] + rest


@pytest.mark.parametrize("K", [12, 25])
def test_entropy_every_partition(K):
    parts = list(_partitions(K))
    assert len(parts) == {12: 77, 25: 1958}[K]
    rng = np.random.default_rng(K)
    lo = np.zeros(len(parts), np.uint64)
    hi = np.zeros(len(parts), np.uint64)
    for i, part in enumerate(parts):
        codes = rng.permutation(31)[:len(part)]                         # distinct letters ('^' = 30 among them at times)
        word = np.concatenate([np.full(c, codes[j]) for j, c in enumerate(part)])
        rng.shuffle(word)
        v = 0
        for x in word:
            v = (v << 5) | int(x)
        lo[i], hi[i] = v & (2 ** 64 - 1), v >> 64
    if K == 25:
        km = np.zeros(len(parts), formats.KEY128_DTYPE)
        km["lo"], km["hi"] = lo, hi
    else:
        km = lo
    content = formats.Content(["non_unique", "T"], np.asarray([0, 5], np.uint32))
    ix = formats.make_index(km, np.full(len(parts), 5, np.uint32), content)
    got = index_edit.shrink_index(ix, 3)
    order = formats.key_order(km)
    keep = np.asarray([index_edit.entropy_keeps(parts[i], K) for i in order])
    assert 0 < keep.sum() < len(parts)
    assert np.array_equal(got.kmer, ix.kmer[keep])
