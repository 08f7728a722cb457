"""`build` on the device (kasa_amd/csrc/kasa_build.h behind kasa_build_*): the C++ host's `kasa_identify build` writes the
reference's own index files byte for byte, and capi.Builder equals numpy's sort + unique + trie + frequencies on the same
pairs however many bricks the input is cut into."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

from kasa_amd import build as hipbuild, capi, formats, reads
from tests import helpers

pytestmark = pytest.mark.gpu

SUFFIXES = ("", "_trie", "_trie.txt", "_info.txt", "_f.txt")
BUILD = os.path.join(helpers.GOLDEN, "dbindex")
CASES = ["folder", "headers", "multiline", "protein", "one", "fivecol"]
EXTRA = {"one": ["--one"]}


def _read(path):
    if not os.path.exists(path) and os.path.exists(path + ".gz"):
        with gzip.open(path + ".gz", "rb") as f:
            return f.read()
    with open(path, "rb") as f:
        return f.read()


def _build(args, tmp_path, env=None):
    exe = hipbuild.build_host()
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([exe, "build"] + args + ["-m", "4", "-n", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600, cwd=str(tmp_path), env=e)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _same_files(new, ref):
    for s in SUFFIXES:
        assert _read(new + s) == _read(ref + s), s


@pytest.mark.parametrize("stem,extra", [("idx", []), ("idx25", ["--kH", "25"]), ("idxa", ["-a", "gc.prt", "2"])])
def test_cpp_build_pairs(stem, extra, tmp_path):
    d = os.path.join(helpers.GOLDEN, "pairs")
    if extra[:1] == ["-a"]:
        extra = ["-a", os.path.join(d, "gc.prt"), "2"]
    _build(["-i", os.path.join(d, "db.fasta"), "-c", os.path.join(d, "content.txt"), "-d", str(tmp_path / "n")] + extra, tmp_path)
    _same_files(str(tmp_path / "n"), os.path.join(d, stem))


@pytest.mark.parametrize("brick", [None, "1000"])
def test_cpp_build_batches_many_taxa(brick, tmp_path):
    """The `batches` database (gzipped FASTA, a content file of many taxa), in one brick and in dozens."""
    d = os.path.join(helpers.GOLDEN, "batches")
    content = str(tmp_path / "content.txt")
    with gzip.open(os.path.join(d, "content.txt.gz"), "rb") as f, open(content, "wb") as g:
        shutil.copyfileobj(f, g)
    r = _build(["-i", os.path.join(d, "db.fasta.gz"), "-c", content, "-d", str(tmp_path / "n"), "-v"], tmp_path,
               {"KASA_BUILD_BRICK_PAIRS": brick} if brick else None)
    _same_files(str(tmp_path / "n"), os.path.join(d, "idx"))
    if brick:
        assert ", bricks 1," not in r.stdout


def test_cpp_build_clones(tmp_path):
    d = os.path.join(helpers.GOLDEN, "clones")
    _build(["-i", os.path.join(d, "db.fasta"), "-c", os.path.join(d, "content.txt"), "-d", str(tmp_path / "n")], tmp_path)
    _same_files(str(tmp_path / "n"), os.path.join(d, "idx"))


@pytest.mark.parametrize("case", CASES)
def test_cpp_build_fixture_cases(case, tmp_path):
    d = os.path.join(BUILD, case)
    src = os.path.join(d, "db") + "/" if case == "folder" else os.path.join(d, "db.fasta")
    _build(["-i", src, "-c", os.path.join(d, "content.txt"), "-d", str(tmp_path / "n")] + EXTRA.get(case, []), tmp_path)
    _same_files(str(tmp_path / "n"), os.path.join(d, "idx"))


def test_cpp_build_empty_index(tmp_path):
    d = os.path.join(BUILD, "headers")
    c = tmp_path / "c.txt"
    c.write_text("Nobody\t5\t5\tNOTHING.1\n")
    exe = hipbuild.build_host()
    r = subprocess.run([exe, "build", "-i", os.path.join(d, "db.fasta"), "-c", str(c), "-d", str(tmp_path / "n")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 1
    assert r.stderr.strip() == "ERROR: Index is empty, are all input files okay?"


def test_build_then_identify(tmp_path):
    """The index the C++ host builds, read by its `identify`: the reference's outputs for pairs/reads.fastq."""
    d = os.path.join(helpers.GOLDEN, "pairs")
    content = os.path.join(d, "content.txt")
    _build(["-i", os.path.join(d, "db.fasta"), "-c", content, "-d", str(tmp_path / "n")], tmp_path)
    exe = hipbuild.build_host()
    out, prof = str(tmp_path / "out.json"), str(tmp_path / "prof.csv")
    r = subprocess.run([exe, "identify", "-c", content, "-d", str(tmp_path / "n"), "-i", os.path.join(d, "reads.fastq"), "-q", out, "-p", prof,
                        "--json", "-m", "4", "-n", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert _read(out) == _read(os.path.join(d, "out_default.json"))
    assert _read(prof) == _read(os.path.join(d, "prof_default.csv"))


# ---- differential: capi.Builder against numpy on the same pairs --------------------------------------------------------

def _random_db(seed, n_taxa, n_seq):
    rng = np.random.default_rng(seed)
    shared = rng.choice(np.frombuffer(b"ACGT", np.uint8), 400)
    seqs, tax = [], []
    for s in range(n_seq):
        L = int(rng.choice([rng.integers(1, 40), rng.integers(40, 3000)]))           # lengths below K too
        x = rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), L)
        if L > 200 and rng.random() < 0.5:                                               # a region shared between taxa
            p = int(rng.integers(0, L - 150))
            x[p:p + 150] = shared[:150]
        if L > 100 and rng.random() < 0.3:                                               # an N run
            p = int(rng.integers(0, L - 30))
            x[p:p + int(rng.integers(1, 30))] = ord("N")
        seqs.append(x)
        tax.append(int(rng.integers(1, n_taxa)))
    content = formats.Content(["non_unique"] + ["T%d" % t for t in range(1, n_taxa)],
                              np.asarray([0] + [1000 + 7 * t for t in range(1, n_taxa)], dtype=np.uint32))
    off = np.zeros(n_seq + 1, np.int64)
    np.cumsum([len(x) for x in seqs], out=off[1:])
    return np.concatenate(seqs), off, content.taxids[np.asarray(tax)], content


def _letters_31(km, K):
    """k-mers with a letter '_' (31): DNA builds drop them (Read.hpp:2008-2066)."""
    bad = np.zeros(km.shape[0], dtype=bool)
    for j in range(K):
        bad |= (formats.key_shr(km, 5 * j) & np.uint64(31)) == np.uint64(31)
    return bad


def _tiny_kmers(seq, K, lut):
    """The windows of a 3- or 4-base sequence (Read.hpp:1991-2075: length + 3(K-1) marker bases - 3K + 1 windows)."""
    def code(p):
        if p >= len(seq):
            return 4
        c = int(seq[p])
        return (c & 14) >> 1 if (c & 0xDF) in b"ACGT" else 5
    out = []
    for w in range(len(seq) - 2):
        key = 0
        for i in range(K):
            p = w + 3 * i
            key = (key << 5) | int(lut[code(p) * 64 + code(p + 1) * 8 + code(p + 2)])
        out.append(key)
    return out


def _numpy_index(bases, off, seq_taxid, content, K):
    """The pairs of the reference's build, from the encoder's (kLow = 1, through an identify context) + the windows of 3- and
    4-base sequences, without the k-mers that hold a '_' -> formats.make_index."""
    one = np.array([1], dtype=np.uint64)
    if K > formats.K64:
        one = np.zeros(1, dtype=formats.KEY128_DTYPE)
        one["lo"] = 1
    boot = formats.make_index(one, content.taxids[1:2].copy(), content)
    dix = capi.DeviceIndex(boot, 0, check_trie=False)
    ctx = capi.Context(dix, K, 1, 3)
    ctx.upload(bases, off)
    ctx.encode()
    ctx.sort_and_range()
    km, seq = ctx.queries()
    ctx.close()
    dix.close()
    tax = seq_taxid[seq]
    lut = capi.builtin_codon_table()
    extra, extra_tax = [], []
    for s in range(off.shape[0] - 1):
        if 3 <= off[s + 1] - off[s] <= 4:
            t = _tiny_kmers(bases[off[s]:off[s + 1]], K, lut)
            extra += t
            extra_tax += [seq_taxid[s]] * len(t)
    if extra:
        if K > formats.K64:
            e = np.zeros(len(extra), dtype=formats.KEY128_DTYPE)
            e["lo"] = [x & (2**64 - 1) for x in extra]
            e["hi"] = [x >> 64 for x in extra]
        else:
            e = np.asarray(extra, dtype=np.uint64)
        km = np.concatenate([km, e])
        tax = np.concatenate([tax, np.asarray(extra_tax, dtype=np.uint32)])
    keep = ~_letters_31(km, K)
    return formats.make_index(km[keep], tax[keep], content)


@pytest.mark.parametrize("K", [12, 25])
@pytest.mark.parametrize("brick", [0, 4099, 1000])
@pytest.mark.parametrize("seed", [1, 2])
def test_builder_differential_bricks(K, brick, seed):
    bases, off, seq_taxid, content = _random_db(100 * seed + K, 9, 60)
    want = _numpy_index(bases, off, seq_taxid, content, K)
    b = capi.Builder(content.taxids, K, 3, None, brick)
    half = 25                                                                            # two add() calls, as a parser streams
    b.add(bases[:off[half]], off[:half + 1], seq_taxid[:half])
    b.add(bases[off[half]:], off[half:] - off[half], seq_taxid[half:])
    n, m = b.finish()
    km, taxid, tp, tc, freq = b.fetch()
    st = b.stats()
    b.close()
    assert n == want.n and m == want.trie_prefix.shape[0]
    assert np.array_equal(km, want.kmer)
    assert np.array_equal(taxid, want.taxid)
    assert np.array_equal(tp, want.trie_prefix) and np.array_equal(tc, want.trie_count)
    assert np.array_equal(freq, want.freq)
    assert st["records_out"] == n
    if brick:
        assert st["bricks"] > 1 and st["merges"] == st["bricks"] - 1
    else:
        assert st["bricks"] == 1


def test_builder_unknown_tax_id_is_refused():
    content_ids = np.asarray([0, 5, 9], dtype=np.uint32)
    b = capi.Builder(content_ids, 12)
    with pytest.raises(RuntimeError, match="does not list"):
        b.add(np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT", np.uint8), np.asarray([0, 40]), np.asarray([7], np.uint32))
    b.close()


def test_index_build_routes_through_builder(tmp_path):
    """index_build.build_index (same signature) with the reference's accession rule: the `headers` case's files."""
    from kasa_amd import index_build
    d = os.path.join(BUILD, "headers")
    ix = index_build.build_index(os.path.join(d, "db.fasta"), os.path.join(d, "content.txt"))
    formats.write_index(ix, str(tmp_path / "n"), str(tmp_path / "c.txt"))
    _same_files(str(tmp_path / "n"), os.path.join(d, "idx"))
