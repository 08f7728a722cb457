"""`merge | redundancy | trie` on the device (two index runs of a builder, kasa_build_taxa_histogram, the trie of a finish):
`kasa_index` writes the reference's own files byte for byte (tests/golden/dbmerge/), a merge of two builds equals the build of
the union, and the taxa histogram equals numpy's on random sorted records."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from kasa_amd import build as hipbuild, capi, formats, index_edit
from tests import helpers
from tests.test_merge_cpu import REDUNDANCY, numpy_histogram

pytestmark = pytest.mark.gpu

SUFFIXES = ("", "_trie", "_trie.txt", "_info.txt", "_f.txt")
DBINDEX = os.path.join(helpers.GOLDEN, "dbindex")
DBEDIT = os.path.join(helpers.GOLDEN, "dbedit")
DBMERGE = os.path.join(helpers.GOLDEN, "dbmerge")


def _run(exe, args, tmp_path, env=None, ok=True):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([exe] + args + ["-m", "4", "-n", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, cwd=str(tmp_path), env=e)
    if ok:
        assert r.returncode == 0, r.stdout + r.stderr
    return r


def _tool(args, tmp_path, env=None, ok=True):
    return _run(hipbuild.build_index_tool(), args, tmp_path, env, ok)


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


def _stage(case, tmp_path, pad=0):
    d = os.path.join(DBMERGE, case)
    for side in ("a", "b"):
        _copy(os.path.join(d, side, "idx"), str(tmp_path / side), pad)
        shutil.copyfile(os.path.join(d, side, "content.txt"), str(tmp_path / (side + "_content.txt")))
    return d


# ---- kasa_index merge against the reference's files ---------------------------------------------------------------------

@pytest.mark.parametrize("case", ["merge64", "merge128"])
@pytest.mark.parametrize("pad", [0, 2 << 20])
def test_cpp_merge_fixtures(case, pad, tmp_path):
    d = _stage(case, tmp_path, pad)
    before = {n: _read(str(tmp_path / n)) for n in os.listdir(tmp_path)}
    _tool(["merge", "--firstIndex", str(tmp_path / "a"), "--secondIndex", str(tmp_path / "b"), "-o", str(tmp_path / "m")], tmp_path)
    for s in ("", "_trie", "_trie.txt", "_f.txt", "_content.txt"):
        assert _read(str(tmp_path / ("m" + s))) == _read(os.path.join(d, "m" + s)), s
    # the reference writes no _info.txt; ours is that of a build of the union
    with open(str(tmp_path / "u.fasta"), "wb") as f:
        f.write(_read(os.path.join(d, "a", "db.fasta")) + _read(os.path.join(d, "b", "db.fasta")))
    _run(hipbuild.build_host(), ["build", "-c", os.path.join(d, "m_content.txt"), "-d", str(tmp_path / "u"), "-i", str(tmp_path / "u.fasta")]
         + (["--kH", "25"] if case == "merge128" else []), tmp_path)
    for s in SUFFIXES:
        assert _read(str(tmp_path / ("m" + s))) == _read(str(tmp_path / ("u" + s))), s
    assert sorted(os.listdir(tmp_path)) == sorted(list(before) + ["m" + s for s in SUFFIXES] + ["m_content.txt", "u.fasta"] + ["u" + s for s in SUFFIXES])
    for n, data in before.items():
        assert _read(str(tmp_path / n)) == data, n


def test_cpp_merge_content_flags(tmp_path):
    """-c1 / -c2 / -co name the content files; -c is the merged content itself and none is written"""
    d = _stage("merge64", tmp_path)
    os.rename(str(tmp_path / "a_content.txt"), str(tmp_path / "ca.txt"))
    os.rename(str(tmp_path / "b_content.txt"), str(tmp_path / "cb.txt"))
    _tool(["merge", "--firstIndex", "a", "--secondIndex", "b", "-o", "m", "-c1", "ca.txt", "-c2", "cb.txt", "-co", "co.txt"], tmp_path)
    assert _read(str(tmp_path / "co.txt")) == _read(os.path.join(d, "m_content.txt")) and not (tmp_path / "m_content.txt").exists()
    _tool(["merge", "--firstIndex", "b", "--secondIndex", "a", "-o", "n", "-c", "co.txt", "--device", "0"], tmp_path)
    for s in ("", "_trie", "_trie.txt", "_f.txt"):
        assert _read(str(tmp_path / ("n" + s))) == _read(os.path.join(d, "m" + s)), s
    assert not (tmp_path / "n_content.txt").exists()


def test_cpp_merge_unknown_taxon_leaves_nothing(tmp_path):
    """A merged content file (-c) without one of the second index's taxa: refused while loading, nothing written, inputs intact."""
    d = _stage("merge64", tmp_path)
    (tmp_path / "c.txt").write_text("".join(l for l in open(os.path.join(d, "m_content.txt")) if not l.startswith("TaxB2\t")))
    before = {n: _read(str(tmp_path / n)) for n in os.listdir(tmp_path)}
    r = _tool(["merge", "--firstIndex", "a", "--secondIndex", "b", "-o", "m", "-c", "c.txt"], tmp_path, ok=False)
    assert r.returncode == 1 and r.stderr.startswith("ERROR: ") and "tax ID 777" in r.stderr, r.stderr
    assert {n: _read(str(tmp_path / n)) for n in os.listdir(tmp_path)} == before


# ---- merge(build(A), build(B)) == build(A u B) ---------------------------------------------------------------------------

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


def _build_index(content, seqs, tax, K):
    b = capi.Builder(content.taxids, K)
    try:
        off = np.zeros(len(seqs) + 1, np.int64)
        np.cumsum([s.shape[0] for s in seqs], out=off[1:])
        b.add(np.concatenate(seqs), off, tax)
        b.finish()
        km, tid, tp, tc, freq = b.fetch()
    finally:
        b.close()
    return formats.Index(km, tid, formats.dense_tax(tid, content), tp, tc, content, freq)


def _same_index(got, want):
    for name in ("kmer", "taxid", "trie_prefix", "trie_count", "freq"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name


@pytest.mark.parametrize("K", [12, 25])
def test_merge_equals_build_of_the_union(K, monkeypatch):
    monkeypatch.setenv("KASA_EDIT_CHUNK_RECORDS", "5000")
    seqs, tax = _genomes(40 + K, 10, 2, 60_000)
    content = formats.Content(["non_unique"] + ["T%d" % t for t in np.unique(tax)], np.concatenate(([0], np.unique(tax))).astype(np.uint32))
    half = len(seqs) // 2
    a_seqs, b_seqs = seqs[:half] + seqs[half + 2:half + 5], seqs[half:]  # A repeats sequences of B: records in both, taxa in both
    a_tax, b_tax = np.concatenate((tax[:half], tax[half + 2:half + 5])), tax[half:]
    a, b = _build_index(content, a_seqs, a_tax, K), _build_index(content, b_seqs, b_tax, K)
    want = _build_index(content, seqs, tax, K)
    assert want.n < a.n + b.n
    for x, y in ((a, b), (b, a)):
        got = index_edit.merge_indices(x, y, content, chunk=7777)       # many add_index calls per run
        _same_index(got, want)
        assert got.edit_stats["index_in"] == a.n + b.n and got.edit_stats["dropped_delete"] == 0 and got.edit_stats["dropped_shrink"] == 0
    _same_index(index_edit.merge_indices(a, a, content, chunk=1001), a)  # an index and its copy
    empty = formats.Index(a.kmer[:0], a.taxid[:0], a.tax[:0], a.trie_prefix[:0], a.trie_count[:0], content, np.zeros_like(a.freq))
    _same_index(index_edit.merge_indices(a, empty, content), a)
    _same_index(index_edit.merge_indices(empty, a, content), a)


def test_second_run_restarts_the_order_check():
    """The second run's first record may be smaller than the first run's last; a break inside the second run is still found."""
    rec = np.zeros(6, formats.REC_DTYPE)
    rec["kmer"], rec["tax"] = [5, 5, 9, 1, 5, 9], [3, 4, 3, 3, 4, 4]
    taxids = np.asarray([0, 3, 4], np.uint32)
    b = capi.Builder(taxids, 12)
    try:
        b.add_index(rec[:3])
        b.add_index(rec[3:], chunk=2)
        assert b.finish()[0] == 5                                        # (5, 4) is in both
        km, tid = b.fetch()[:2]
        assert km.tolist() == [1, 5, 5, 9, 9] and tid.tolist() == [3, 3, 4, 3, 4]
        assert b.edit_stats()["index_in"] == 6
    finally:
        b.close()
    b = capi.Builder(taxids, 12)
    try:
        b.add_index(rec[:3])
        with pytest.raises(RuntimeError, match="record 2 "):
            b.add_index(rec[[3, 5, 4]], chunk=2)
    finally:
        b.close()


# ---- the taxa histogram against numpy ----------------------------------------------------------------------------------

def _sorted_records(seed, lens, n_taxa, K):
    """records of len(lens) distinct random k-mers, run r carrying lens[r] distinct tax IDs; content IDs with the 0 of row 0"""
    rng = np.random.default_rng(seed)
    taxids = np.concatenate(([0], np.sort(rng.choice(np.arange(1, 10 ** 7, dtype=np.uint32), n_taxa - 1, replace=False)))).astype(np.uint32)
    m = lens.shape[0]
    pool = rng.integers(0, 2 ** 63, 4096, dtype=np.uint64) >> np.uint64(4)    # few low words, few high words: both must be compared
    if K == 25:
        pairs = np.unique(rng.integers(0, 1024 * 4096, int(m * 1.3) + 16))[:m]
        while pairs.shape[0] < m:
            pairs = np.unique(np.concatenate((pairs, rng.integers(0, 1024 * 4096, m))))[:m]
        hi, lo = (pairs // 4096).astype(np.uint64), pool[pairs % 4096]
        order = np.lexsort((lo, hi))
        keys = np.zeros(m, formats.KEY128_DTYPE)
        keys["lo"], keys["hi"] = lo[order], hi[order]
    else:
        keys = np.zeros(0, np.uint64)
        while keys.shape[0] < m:
            x = (rng.integers(0, 2 ** 27, m + 16, dtype=np.uint64) << np.uint64(32)) | (pool[rng.integers(0, 4096, m + 16)] & np.uint64(0xFFFFFFFF))
            keys = np.unique(np.concatenate((keys, x)))[:m]
    n = int(lens.sum())
    start = np.zeros(m, np.int64)
    np.cumsum(lens[:-1], out=start[1:])
    run = np.repeat(np.arange(m), lens)
    first_tax = rng.integers(0, n_taxa - lens + 1)                      # a run's taxa: lens[r] neighbours among the sorted IDs
    tax = taxids[first_tax[run] + (np.arange(n) - start[run])]
    rec = np.zeros(n, formats.REC128_DTYPE if K == 25 else formats.REC_DTYPE)
    if K == 25:
        rec["lo"], rec["hi"] = keys["lo"][run], keys["hi"][run]
    else:
        rec["kmer"] = keys[run]
    rec["tax"] = tax
    return rec, taxids


def _lens(shape, n, n_taxa, rng):
    if shape == "ones":
        return np.ones(n, np.int64)
    if shape == "few":                                                   # what an index looks like: mostly one taxon, some 2..6
        lens = np.ones(n * 9 // 10, np.int64)
        some = rng.random(lens.shape[0]) < 0.08
        lens[some] = rng.integers(2, min(7, n_taxa + 1), int(some.sum()))
    elif shape == "crowded":                                             # runs of 50..500 between runs of 1..3
        lens = rng.integers(1, 4, n // 8)
        big = rng.random(lens.shape[0]) < 0.02
        lens[big] = rng.integers(min(50, n_taxa), min(500, n_taxa) + 1, int(big.sum()))
    else:                                                                # "full": one run of every tax ID the content lists
        lens = rng.integers(1, 3, n // 2)
        lens[lens.shape[0] // 3] = n_taxa
    lens = lens[np.cumsum(lens) <= n]
    return lens.astype(np.int64)


def _hist_of(rec):
    k = rec[["lo", "hi"]] if "lo" in rec.dtype.names else rec["kmer"]
    return k


@pytest.mark.parametrize("K", [12, 25])
@pytest.mark.parametrize("n,n_taxa", [(120_000, 30), (400_000, 50_000), (1_000_000, 900)])
@pytest.mark.parametrize("shape", ["ones", "few", "crowded", "full"])
def test_taxa_histogram_against_numpy(K, n, n_taxa, shape):
    rng = np.random.default_rng(n + n_taxa + K)
    lens = _lens(shape, n, n_taxa, rng)
    rec, taxids = _sorted_records(n_taxa + K, lens, n_taxa, K)
    want = np.bincount(lens, minlength=n_taxa + 1).astype(np.uint64)
    assert np.array_equal(want, numpy_histogram(_hist_of(rec), n_taxa + 1))
    if shape == "full":
        assert want[n_taxa] == 1
    if shape == "crowded" and n_taxa >= 500:
        assert want[50:501].sum() > 50
    b = capi.Builder(taxids, K)
    try:
        with pytest.raises(RuntimeError, match="kasa_build_finish first"):
            b.taxa_histogram()
        b.add_index(rec, chunk=rec.shape[0] // 7 + 3)                    # runs straddle the chunks, and the blocks of 256
        b.finish()
        hist, distinct = b.taxa_histogram()
        assert hist.shape[0] == n_taxa + 1 and hist[0] == 0
        assert np.array_equal(hist, want)
        assert distinct == lens.shape[0]
        hist2, _ = b.taxa_histogram()                                    # (no state is left behind)
        assert np.array_equal(hist2, want)
        longest = int(lens.max())
        h3, d3 = b.taxa_histogram(longest + 1)
        assert np.array_equal(h3, want[:longest + 1]) and d3 == distinct
        with pytest.raises(RuntimeError, match="kasa_build_taxa_histogram: the k-mer that ends at record"):
            b.taxa_histogram(longest)
    finally:
        b.close()


@pytest.mark.parametrize("K", [12, 25])
def test_taxa_histogram_describes_the_filtered_result(K, monkeypatch):
    rng = np.random.default_rng(K)
    n_taxa = 900
    lens = _lens("crowded", 300_000, n_taxa, rng)
    rec, taxids = _sorted_records(7 + K, lens, n_taxa, K)
    drop = rng.choice(taxids[1:], 300, replace=False)

    def run(edit):
        b = capi.Builder(taxids, K)
        try:
            edit(b)
            b.add_index(rec, chunk=50_001)
            b.finish()
            return b.taxa_histogram(), b.fetch()[0]
        finally:
            b.close()

    (hist, distinct), km = run(lambda b: b.drop_taxa(drop))
    kept = rec[~np.isin(rec["tax"], drop)]
    want = numpy_histogram(_hist_of(kept), n_taxa + 1)
    assert np.array_equal(hist, want) and distinct == int(want.sum()) and km.shape[0] == kept.shape[0]
    monkeypatch.setenv("KASA_EDIT_CHUNK_RECORDS", "40000")
    for strategy, edit in ((1, lambda b: b.shrink(1, 37.5)), (3, lambda b: b.shrink(3))):
        (hist, distinct), km = run(edit)
        assert 0 < km.shape[0] <= rec.shape[0] and (strategy == 3 or km.shape[0] < rec.shape[0])
        want = numpy_histogram(km, n_taxa + 1)
        assert np.array_equal(hist, want) and distinct == int(want.sum())


def test_taxa_histogram_refused_on_a_halved_result():
    ix = helpers.load_case("pairs")[1]
    b = capi.Builder(ix.content.taxids, 12)
    try:
        b.shrink(2)
        b.add_index(index_edit._records(ix))
        b.finish()
        with pytest.raises(RuntimeError, match="halved"):
            b.taxa_histogram()
    finally:
        b.close()


def test_redundancy_and_rebuild_trie_on_the_fixtures():
    for name, (prefix, content) in REDUNDANCY.items():
        ix = formats.load_index(prefix, content)
        hist, cutoff = index_edit.redundancy(ix)
        assert np.array_equal(hist, numpy_histogram(ix.kmer, ix.content.taxids.shape[0] + 1)), name
        assert cutoff == {"headers": 2, "multiline": 1, "wide": 2, "clones6": 6}[name]
        tp, tc = index_edit.rebuild_trie(ix)
        assert np.array_equal(tp, ix.trie_prefix) and np.array_equal(tc, ix.trie_count), name


# ---- kasa_index redundancy | trie --------------------------------------------------------------------------------------

def _report(stdout, verbose):
    ls = stdout.splitlines()
    first = next(i for i, x in enumerate(ls) if x.startswith("Number of unique")) if verbose else max(i for i, x in enumerate(ls) if x.startswith("OUT:"))
    return "\n".join(ls[first:]) + "\n"


@pytest.mark.parametrize("name", sorted(REDUNDANCY))
@pytest.mark.parametrize("verbose", [False, True])
def test_cpp_redundancy_fixtures(name, verbose, tmp_path):
    prefix, content = REDUNDANCY[name]
    _copy(prefix, str(tmp_path / "r"), 2 << 20)
    shutil.copyfile(content, str(tmp_path / "r_content.txt"))                      # the default content file
    before = {n: _read(str(tmp_path / n)) for n in os.listdir(tmp_path)}
    r = _tool(["redundancy", "-d", str(tmp_path / "r")] + (["-v"] if verbose else []), tmp_path)
    assert _report(r.stdout, verbose) == open(os.path.join(DBMERGE, "redundancy", name + ("_v" if verbose else "") + ".txt")).read()
    r2 = _tool(["redundancy", "-d", "r", "-c", content] + (["-v"] if verbose else []), tmp_path)
    assert _report(r2.stdout, verbose) == _report(r.stdout, verbose)
    assert {n: _read(str(tmp_path / n)) for n in os.listdir(tmp_path)} == before


def _golden_indices():
    out = []
    for root in (DBINDEX, DBEDIT, DBMERGE):
        for info in sorted(glob.glob(os.path.join(root, "**", "*_info.txt"), recursive=True)):
            prefix = info[:-len("_info.txt")]
            if not all(os.path.exists(prefix + s) for s in SUFFIXES):
                continue
            words = open(info).read().split()
            # (dbedit/delete128: the reference's own _info.txt lacks the "128" line, so the file does not describe its index)
            if words[1:] != ["3"] and os.path.getsize(prefix) == int(words[0]) * (20 if words[1:] == ["128"] else 12):
                out.append(os.path.relpath(prefix, helpers.GOLDEN))
    return out


def test_the_golden_indices_cover_both_widths():
    kinds = {tuple(open(os.path.join(helpers.GOLDEN, p) + "_info.txt").read().split()[1:]) for p in _golden_indices()}
    assert kinds == {(), ("128",)} and len(_golden_indices()) >= 20


@pytest.mark.parametrize("prefix", _golden_indices())
def test_cpp_trie_restores_the_files(prefix, tmp_path):
    src = os.path.join(helpers.GOLDEN, prefix)
    _copy(src, str(tmp_path / "x"), 2 << 20)
    os.remove(str(tmp_path / "x_trie"))
    (tmp_path / "x_trie.txt").write_text("stale")
    before = {n: _read(str(tmp_path / n)) for n in ("x", "x_info.txt", "x_f.txt")}
    _tool(["trie", "-d", str(tmp_path / "x")], tmp_path)
    assert _read(str(tmp_path / "x_trie")) == _read(src + "_trie") and _read(str(tmp_path / "x_trie.txt")) == _read(src + "_trie.txt")
    assert sorted(os.listdir(tmp_path)) == sorted("x" + s for s in SUFFIXES)
    for n, data in before.items():
        assert _read(str(tmp_path / n)) == data, n
