"""CPU-only checks of `merge | redundancy | trie`: the content merge against the reference's files (tests/golden/dbmerge/),
the redundancy cutoff against a literal transcription of the reference's loop (Shrink.hpp:60-71), the report text against the
reference's stdout, every refusal of `kasa_index` (all before any device work), and the exported symbol."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from kasa_amd import build as hipbuild, formats, index_edit
from tests import helpers

DBINDEX = os.path.join(helpers.GOLDEN, "dbindex")
DBEDIT = os.path.join(helpers.GOLDEN, "dbedit")
DBMERGE = os.path.join(helpers.GOLDEN, "dbmerge")
PAIRS = os.path.join(helpers.GOLDEN, "pairs")
SUFFIXES = ("", "_trie", "_trie.txt", "_info.txt", "_f.txt")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (index prefix, content file) of the four indices whose `redundancy` output the reference printed
REDUNDANCY = {"headers": (os.path.join(DBINDEX, "headers", "idx"), os.path.join(DBINDEX, "headers", "content.txt")),
              "multiline": (os.path.join(DBINDEX, "multiline", "idx"), os.path.join(DBINDEX, "multiline", "content.txt")),
              "wide": (os.path.join(DBEDIT, "update128", "old"), os.path.join(DBINDEX, "headers", "content.txt")),
              "clones6": (os.path.join(DBMERGE, "redundancy", "clones6", "idx"), os.path.join(DBMERGE, "redundancy", "clones6", "content.txt"))}


def numpy_histogram(kmer, n_bins):
    """hist[c] = distinct k-mers with exactly c records, of k-mers in index order"""
    head = np.ones(kmer.shape[0], dtype=bool)
    head[1:] = kmer[1:] != kmer[:-1]
    pos = np.flatnonzero(head)
    lens = np.diff(np.concatenate((pos, [kmer.shape[0]])))
    return np.bincount(lens, minlength=n_bins).astype(np.uint64)


def _read(path):
    with open(path, "rb") as f:
        return f.read()


# ---- merge_content ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["merge64", "merge128"])
def test_merge_content_equals_the_reference(case, tmp_path):
    d = os.path.join(DBMERGE, case)
    index_edit.merge_content(os.path.join(d, "a", "content.txt"), os.path.join(d, "b", "content.txt"), str(tmp_path / "c.txt"))
    assert _read(str(tmp_path / "c.txt")) == _read(os.path.join(d, "m_content.txt"))


def _rows(path):
    return [line.split("\t") for line in open(path).read().splitlines()]


def test_merge_content_joins_the_lists_of_a_shared_taxon(tmp_path):
    d = os.path.join(DBMERGE, "merge_lists")
    index_edit.merge_content(os.path.join(d, "a_content.txt"), os.path.join(d, "b_content.txt"), str(tmp_path / "c.txt"))
    got, want = _rows(str(tmp_path / "c.txt")), _rows(os.path.join(d, "m_content.txt"))
    assert [r[:2] for r in got] == [r[:2] for r in want]                  # names (the second file's) and tax IDs, in order
    for g, w in zip(got, want):                                           # the reference's order inside a list is a hash table's
        assert len(g) == len(w) == 4
        for col in (2, 3):
            assert len(g[col].split(";")) == len(set(g[col].split(";")))
            assert set(g[col].split(";")) == set(w[col].split(";"))
    shared = [r for r in got if r[1] == "500"][0]
    assert shared[2] == "500;501;502" and shared[3] == "SH_1.1;SH_2.1;SH_3.1;SH_4.1"   # the first file's, then the second's new ones


def test_merge_content_sorts_unsorted_inputs(tmp_path):
    (tmp_path / "a.txt").write_text("Z\t900\t900\tZ.1\nA\t5\t5\tA.1\nM\t77\t77\tM.1\n")
    (tmp_path / "b.txt").write_text("Q\t500\t500\tQ.1\nM2\t77\t78\tM.2\nB\t6\t6\tB.1\n")
    index_edit.merge_content(str(tmp_path / "a.txt"), str(tmp_path / "b.txt"), str(tmp_path / "c.txt"))
    assert (tmp_path / "c.txt").read_text() == "A\t5\t5\tA.1\nB\t6\t6\tB.1\nM2\t77\t77;78\tM.1;M.2\nQ\t500\t500\tQ.1\nZ\t900\t900\tZ.1\n"


BAD_CONTENT = [("\nA\t5\t5\tA.1\n", "leading empty line"), ("A\t5\t5\n", "less than 4 columns"), ("A\t5\t5\tA.1\t1\n", "five columns"),
               ("A\t5\t5\tA.1\nEWAN_0\t4294967295\t4294967295\tX.1\n", "dummy taxa")]


@pytest.mark.parametrize("text,what", BAD_CONTENT)
@pytest.mark.parametrize("side", [0, 1])
def test_merge_content_refusals(text, what, side, tmp_path):
    good = "B\t6\t6\tB.1\n"
    (tmp_path / "a.txt").write_text(text if side == 0 else good)
    (tmp_path / "b.txt").write_text(text if side == 1 else good)
    with pytest.raises(ValueError, match=what):
        index_edit.merge_content(str(tmp_path / "a.txt"), str(tmp_path / "b.txt"), str(tmp_path / "c.txt"))
    assert not (tmp_path / "c.txt").exists()


# ---- redundancy ------------------------------------------------------------------------------------------------------

def _reference_cutoff(tax_ids, size):
    """Shrink.hpp:60-71: taxIDs[i] = k-mers with i taxa, i < iNumOfTaxIDs + 1"""
    percentage = 0.0
    idx_of_99 = 0
    for i in range(1, len(tax_ids)):
        percentage += float(int(tax_ids[i])) * i / size
        if percentage >= 0.99 and idx_of_99 == 0:
            idx_of_99 = i
    return idx_of_99


def test_redundancy_cutoff_against_the_reference_loop():
    rng = np.random.default_rng(99)
    seen = set()
    for trial in range(300):
        bins = int(rng.integers(2, 40))
        hist = np.zeros(bins, np.uint64)
        hist[1:] = rng.integers(0, 10 ** int(rng.integers(1, 7)), bins - 1) * (rng.random(bins - 1) < rng.uniform(0.2, 1.0))
        if trial % 3 == 0:
            hist[1] = int(hist[1:].astype(np.float64) @ np.arange(1, bins)) * int(rng.integers(50, 200))   # nearly all k-mers have one taxon
        size = int(sum(int(hist[i]) * i for i in range(1, bins)))
        if size == 0:
            continue
        want = _reference_cutoff(hist, size)
        assert index_edit.redundancy_cutoff(hist, size) == want
        seen.add(min(want, 4))
    assert {1, 2, 3, 4} <= seen
    # a sum that never reaches 0.99: the records the histogram describes are fewer than n_records says
    hist = np.asarray([0, 10, 5, 1], np.uint64)
    assert _reference_cutoff(hist, 100) == 0 and index_edit.redundancy_cutoff(hist, 100) == 0
    assert index_edit.redundancy_report(hist, 100).startswith("OUT: 99% of the k-mers in your index have 0 or less taxa. Using unique")


@pytest.mark.parametrize("name", sorted(REDUNDANCY))
@pytest.mark.parametrize("verbose", [False, True])
def test_redundancy_report_equals_the_reference(name, verbose):
    prefix, content = REDUNDANCY[name]
    ix = formats.load_index(prefix, content)
    hist = numpy_histogram(ix.kmer, ix.content.taxids.shape[0] + 1)
    want = open(os.path.join(DBMERGE, "redundancy", name + ("_v" if verbose else "") + ".txt")).read()
    assert index_edit.redundancy_report(hist, ix.n, verbose) == want
    assert index_edit.redundancy_cutoff(hist, ix.n) == {"headers": 2, "multiline": 1, "wide": 2, "clones6": 6}[name]


# ---- kasa_index: refusals, all before any device work -------------------------------------------------------------------

def _tool(args, cwd):
    exe = hipbuild.build_index_tool()
    return subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=str(cwd))


def _copy(src, dst):
    for s in SUFFIXES:
        shutil.copyfile(src + s, dst + s)


def _snapshot(d):
    return {name: _read(os.path.join(str(d), name)) for name in sorted(os.listdir(str(d)))}


@pytest.fixture
def two(tmp_path):
    """a, b: the two 64-bit indices of merge64 with their content files; w: a 128-bit index; h: a halved one"""
    for side in ("a", "b"):
        _copy(os.path.join(DBMERGE, "merge64", side, "idx"), str(tmp_path / side))
        shutil.copyfile(os.path.join(DBMERGE, "merge64", side, "content.txt"), str(tmp_path / (side + "_content.txt")))
    _copy(os.path.join(DBMERGE, "merge128", "a", "idx"), str(tmp_path / "w"))
    shutil.copyfile(os.path.join(DBMERGE, "merge128", "a", "content.txt"), str(tmp_path / "w_content.txt"))
    _copy(os.path.join(PAIRS, "idx_half"), str(tmp_path / "h"))
    shutil.copyfile(os.path.join(PAIRS, "content.txt"), str(tmp_path / "h_content.txt"))
    return tmp_path


MERGE = ["merge", "--firstIndex", "a", "--secondIndex", "b", "-o", "m"]


@pytest.mark.parametrize("args,what", [
    (["merge", "--firstIndex", "a", "--secondIndex", "a", "-o", "m"], "-d and -i must point to different indices!"),
    (["merge", "--firstIndex", "a", "--secondIndex", "b", "-o", "a"], "You can't overwrite indices (yet)!"),
    (["merge", "--firstIndex", "a", "--secondIndex", "b", "-o", "b"], "You can't overwrite indices (yet)!"),
    (["merge", "--firstIndex", "a", "--secondIndex", "b"], "No output file given!"),
    (["merge", "--firstIndex", "a", "-o", "m"], "two indices"),
    (["merge", "--firstIndex", "a", "--secondIndex", "w", "-o", "m"], "Indices are not of the same format!"),
    (["merge", "--firstIndex", "w", "--secondIndex", "b", "-o", "m"], "Indices are not of the same format!"),
    (["merge", "--firstIndex", "a", "--secondIndex", "h", "-o", "m"], "Halved indices"),
    (["merge", "--firstIndex", "h", "--secondIndex", "b", "-o", "m"], "Halved indices"),
    (["merge", "--firstIndex", "a", "--secondIndex", "nothing", "-o", "m"], "Info file for the second index can not be found!"),
    (["merge", "--firstIndex", "nothing", "--secondIndex", "b", "-o", "m"], "Info file for the first index can not be found!"),
    (["merge", "--firstIndex", "a", "--secondIndex", "noindex", "-o", "m"], "The index file cannot be found!"),
    (MERGE + ["-c2", "missing.txt"], "Second content file couldn't be read!"),
    (MERGE + ["-c1", "missing.txt"], "First content file couldn't be read!"),
    (MERGE + ["-c", "missing.txt"], "Content file not found."),
    (MERGE + ["-c1", "empty_line.txt"], "leading empty line"),
    (MERGE + ["-c2", "three.txt"], "less than 4 columns"),
    (MERGE + ["-c1", "five.txt"], "five columns"),
    (MERGE + ["-c", "five.txt"], "five columns"),
    (MERGE + ["-c2", "ewan.txt"], "dummy taxa"),
    (MERGE + ["-k", "12", "7"], "-k"),
    (MERGE + ["--kL", "7"], "--kL"),
    (MERGE + ["--kH", "25"], "--kH"),
    (MERGE + ["-y", "tax/"], "not supported"),
    (MERGE + ["-f", "acc2tax/"], "not supported"),
    (MERGE + ["-u", "species"], "not supported"),
    (MERGE + ["-d", "a"], "unknown parameter"),
    (["redundancy", "-d", "h"], "redundancy cannot be called on shrunken indices!"),
    (["redundancy", "-d", "nothing"], "Info file for this index can not be found!"),
    (["redundancy", "-d", "a", "-c", "missing.txt"], "Content file not found."),
    (["redundancy", "-d", "a", "--kH", "25"], "--kH"),
    (["redundancy"], "no index given"),
    (["trie", "-d", "nothing"], "Info file for this index can not be found!"),
    (["trie", "-d", "noindex"], "The index file cannot be found!"),
    (["trie", "-d", "h"], "Halved indices"),
    (["trie", "-d", "a", "-k", "12", "7"], "-k"),
    (["trie", "-d", "a", "--kH", "25"], "--kH"),
    (["trie", "-d", "a", "-c", "a_content.txt"], "unknown parameter"),
    (["trie"], "no index given"),
])
def test_kasa_index_refusals(args, what, two):
    (two / "noindex_info.txt").write_text("10")
    (two / "empty_line.txt").write_text("\nA\t5\t5\tA.1\n")
    (two / "three.txt").write_text("A\t5\t5\n")
    (two / "five.txt").write_text("A\t5\t5\tA.1\t1\n")
    (two / "ewan.txt").write_text("A\t5\t5\tA.1\nEWAN_0\t4294967295\t4294967295\tX.1\n")
    before = _snapshot(two)
    r = _tool(args, two)
    assert r.returncode != 0, r.stdout + r.stderr
    assert r.stderr.startswith("ERROR: ") and what in r.stderr, r.stderr
    assert _snapshot(two) == before


@pytest.mark.parametrize("args", [[], ["identify"], ["build"], ["update"], ["half"], ["generateCF"]])
def test_kasa_index_lists_its_modes(args, tmp_path):
    r = _tool(args, tmp_path)
    assert r.returncode != 0 and r.stderr.startswith("ERROR: "), r.stderr
    for mode in ("`merge`", "`redundancy`", "`trie`"):
        assert mode in r.stderr, r.stderr
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("mode", ["merge", "redundancy", "trie"])
def test_kasa_identify_still_refuses_the_modes(mode, tmp_path):
    r = subprocess.run([hipbuild.build_host(), mode, "-d", "x"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 1 and r.stderr.startswith("ERROR: only the modes `build`, `update`, `delete`, `shrink`, `getFrequency`, `identify`"), r.stderr


# ---- the ABI ---------------------------------------------------------------------------------------------------------

def test_taxa_histogram_is_exported_and_declared():
    so = hipbuild.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert re.search(r" T kasa_build_taxa_histogram$", syms, re.M)
    header = open(os.path.join(ROOT, "include", "kasa_hip.h")).read()
    assert "int kasa_build_taxa_histogram(kasa_builder *b, uint64_t *hist, uint64_t nBins, uint64_t *distinctKmers);" in header
