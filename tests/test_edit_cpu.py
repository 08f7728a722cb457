"""CPU-only checks of the edit modes' host side: the refusals of `kasa_identify update | delete | shrink | getFrequency` (all
before any device work), delnodes.dmp parsing, the table of ordinals `shrink -s 1 -g P` drops against a literal transcription
of the reference's loop (Shrink.hpp:270-308), and the percentage `shrink -m` derives (main.cpp:839-857)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from kasa_amd import build as hipbuild, index_edit
from tests import helpers

DBINDEX = os.path.join(helpers.GOLDEN, "dbindex")
DBEDIT = os.path.join(helpers.GOLDEN, "dbedit")
SUFFIXES = ("", "_trie", "_trie.txt", "_info.txt", "_f.txt")


def _host(args, tmp_path):
    exe = hipbuild.build_host()
    return subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=str(tmp_path))


def _copy(src, dst):
    for s in SUFFIXES:
        shutil.copyfile(src + s, dst + s)


def _refused(r, what):
    assert r.returncode == 1, r.stdout + r.stderr
    assert r.stderr.startswith("ERROR: ") and what in r.stderr, r.stderr


@pytest.fixture
def old(tmp_path):
    _copy(os.path.join(DBINDEX, "headers", "idx"), str(tmp_path / "old"))
    return str(tmp_path / "old")


def _untouched(old):
    for s in SUFFIXES:
        with open(old + s, "rb") as f, open(os.path.join(DBINDEX, "headers", "idx") + s, "rb") as g:
            assert f.read() == g.read(), s


@pytest.mark.parametrize("args,what", [
    (["update", "-i", "new.fasta"], "content file (-c)"),
    (["update", "-i", "new.fasta", "-c", "C", "-u", "species"], "not supported"),
    (["update", "-i", "new.fasta", "-c", "C", "-y", "tax/"], "not supported"),
    (["update", "-i", "new.fasta", "-c", "C", "-f", "acc2tax/"], "not supported"),
    (["update", "-i", "new.fasta", "-c", "C", "-k", "12", "7"], "-k"),
    (["delete", "-c", "C", "-o", "out"], "delnodes.dmp"),
    (["delete", "-c", "C", "-l", "D"], "No output file given!"),
    (["delete", "-l", "D", "-o", "out"], "content file"),
    (["delete", "-l", "D", "-o", "out", "-c", "C", "--kL", "7"], "--kL"),
    (["shrink", "-c", "C", "-s", "1", "-g", "50", "-o", "OLD"], "Paths and names of input and output are the same!"),
    (["shrink", "-c", "C", "-s", "4"], "strategy 4"),
    (["shrink", "-c", "C", "-s", "3", "--kH", "25"], "--kH"),
    (["getFrequency", "-c", "C", "-k", "12", "5"], "-k"),
])
def test_edit_refusals(args, what, old, tmp_path):
    c = os.path.join(DBINDEX, "headers", "content.txt")
    d = tmp_path / "D"
    d.write_text("77\t|\n")
    args = [c if x == "C" else (str(d) if x == "D" else (old if x == "OLD" else x)) for x in args]
    r = _host(args[:1] + ["-d", old] + args[1:], tmp_path)
    _refused(r, what)
    _untouched(old)
    assert sorted(os.listdir(tmp_path)) == sorted(["D"] + ["old" + s for s in SUFFIXES])


def test_halved_and_wide_refusals(tmp_path):
    p = os.path.join(helpers.GOLDEN, "pairs")
    c = os.path.join(p, "content.txt")
    r = _host(["delete", "-d", os.path.join(p, "idx_half"), "-c", c, "-l", c, "-o", str(tmp_path / "x")], tmp_path)
    _refused(r, "Halved indices cannot be modified in this way. Sorry...")
    r = _host(["shrink", "-d", os.path.join(p, "idx25"), "-c", c, "-s", "2", "-o", str(tmp_path / "x")], tmp_path)
    _refused(r, "If k is larger than 12, the index can not be halved as of now!")
    r = _host(["shrink", "-d", os.path.join(p, "idx25"), "-c", c, "-o", str(tmp_path / "x")], tmp_path)   # -s defaults to 2
    _refused(r, "can not be halved")
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("mode", ["delete", "getFrequency"])
def test_five_column_content_refused(mode, tmp_path):
    d = os.path.join(DBINDEX, "fivecol")
    _copy(os.path.join(d, "idx"), str(tmp_path / "old"))
    (tmp_path / "del.dmp").write_text("4001\t|\n")
    args = [mode, "-d", str(tmp_path / "old"), "-c", os.path.join(d, "content.txt")]
    if mode == "delete":
        args += ["-l", str(tmp_path / "del.dmp"), "-o", str(tmp_path / "new")]
    r = _host(args, tmp_path)
    _refused(r, "five columns")
    assert not os.path.exists(str(tmp_path / "new"))


def test_unsupported_modes_list_the_available_ones(tmp_path):
    for mode in ("merge", "redundancy", "trie", "generateCF"):
        r = _host([mode, "-d", "x"], tmp_path)
        _refused(r, "only the modes")
        for m in ("build", "update", "delete", "shrink", "getFrequency", "identify"):
            assert "`" + m + "`" in r.stderr


def test_read_delnodes(tmp_path):
    p = tmp_path / "delnodes.dmp"
    p.write_text("12\t|\n\n3456\t|\n7\n99\t|\textra\n")
    assert index_edit.read_delnodes(str(p)).tolist() == [12, 3456, 7, 99]


def _reference_loop(P, n):
    """Shrink.hpp:270-308 for one taxon of n records, transcribed literally: which ordinals (1-based) go."""
    a = abs(float(np.float32(P)))
    step = 100.0 / a if a else float("inf")                # (C++: a double divided by 0.f)
    steps, nxt, gone = 1, step, []
    for _ in range(n):
        thr = int(nxt) if np.isfinite(nxt) else 0       # (uint64_t) of the double; inf never equals an ordinal
        if steps != thr:
            pass
        else:
            gone.append(steps)
            nxt += step
        steps += 1
    return gone


@pytest.mark.parametrize("P", [30, 33.3, -30, 50, 66.6, 99.9, 100, 12.5, 1.0, 0.7, 7.77, 150, 0, 1e-3, 100.5, -100])
def test_threshold_table_matches_the_reference_loop(P):
    n = 5000
    assert index_edit.shrink_thresholds(P, n).tolist() == _reference_loop(P, n)


def test_threshold_table_float_percentage():
    """33.3 as the reference reads it (stof) differs from the double 33.3 somewhere in the first hundred thousand ordinals."""
    t = index_edit.shrink_thresholds(33.3, 100000)
    step = 100.0 / 33.3
    d, other = step, []
    while int(d) <= 100000:
        other.append(int(d))
        d += step
    assert t.tolist() != other
    assert index_edit.shrink_thresholds(-33.3, 100000).tolist() == t.tolist()
    assert index_edit.shrink_thresholds(150, 10 ** 6).size == 0 and index_edit.shrink_thresholds(0, 10 ** 6).size == 0
    assert index_edit.shrink_thresholds(100, 50).tolist() == list(range(1, 51))


def test_memory_percentage():
    # 4882 records of 12 bytes; -m 0 and sizes far above the index: negative percentages, which keep everything
    for gib, n, rb in [(1, 10 ** 9, 12), (3, 4 * 10 ** 8, 12), (2, 10 ** 9, 20), (5, 4882, 12)]:
        mem = np.float32(gib * 1024 ** 3)
        want = np.float32(100.0) - np.float32(100.0) * mem / np.float32(n * rb)
        assert index_edit.memory_percentage(gib, n, rb) == float(np.float32(want))
    assert abs(index_edit.memory_percentage(1, 10 ** 9, 12) - (100 - 100 * 2 ** 30 / 12e9)) < 1e-3


def test_entropy_rule_examples():
    assert not index_edit.entropy_keeps([12], 12)                 # one letter: H = 0
    assert index_edit.entropy_keeps([1] * 12, 12)                 # twelve letters: log2(12) / log2(22) > 0.5
    assert not index_edit.entropy_keeps([11, 1], 12)
