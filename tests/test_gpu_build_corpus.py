"""The index builder and editor (kasa_amd/csrc/kasa_build.h and kasa_edit.h behind kasa_build_*) on the hand-made cases of
tests/build_corpus.py, both key widths, through capi.Builder: k-mers, tax IDs, trie prefixes and counts, frequency rows, the
counts of stats() and edit_stats(), taxa_histogram() and, where a case refuses, the text of the refusal -- all against the
corpus's plain reference, all exact.  A halved result (shrink 2) is compared as fetch() rebuilds it and as the raw 6-byte
records.  tests/test_build_corpus_cpu.py shows on the CPU that every case holds what its family claims.

No case is left out: every family's test runs all of the family's cases and counts them, and the counts add up to the corpus's.
Every case with an index, drop or shrink step runs a second time finished by finish_slabs() -- the calls the C++ edit modes and
`kasa_index merge` write their files through: exactly one slab, and the same comparisons.

The C++ hosts run one round trip -- `kasa_identify build` twice, `kasa_index merge`, `kasa_identify shrink -s 2` -- on the small
amino-acid database of tests/golden/dbedit/halved_pads/, whose sequences hold '^' and '~': against the plain reference's
files byte for byte, and against the files the reference's own binary wrote for that database (records, info and frequencies
byte for byte; the trie up to its last count, which the reference writes one short -- DESIGN.md section 8o).

Wall time on an MI355X (pytest --durations): the file's 23 tests in about 10 s.  large/merge/K25 3.0 s and large/merge/K12 1.3 s
(each with the building of its case: 16.8 M merged outputs), the C++ round trip 1.6 s, the nth family's 52 cases 1.4 s, the tiny
family 1.0 s (the plain reference of its long sequences), large/brick and large/shrink at most 0.5 s each, every other family at
most 0.25 s.  In the same run tests/test_gpu_edit.py takes 17 s and tests/test_gpu_merge.py 23 s."""
import os
import subprocess

import numpy as np
import pytest

from kasa_amd import build as hipbuild, capi, formats
from tests import build_corpus as bc, helpers
from tests.test_gpu_parity import _gpu_or_fail

pytestmark = pytest.mark.gpu

SMALL_FAMILIES = ("unique", "illegal", "tiny", "bricks", "merge", "trie", "freq", "load", "delete", "nth", "halved", "hist")
RAN = {}                                            # family -> the cases compared


def _first_difference(a, b):
    n = min(a.shape[0], b.shape[0])
    d = np.flatnonzero(a[:n] != b[:n])
    return int(d[0]) if d.shape[0] else n


def _refusal(ex):
    """the text of a refusal; an error of the HIP runtime ("hip...(...) failed: ...") is no refusal and ends the test"""
    if " failed: " in str(ex):
        raise ex
    return str(ex)


def _finish_by_slabs(b, c):
    """finish_slabs() in fetch()'s form, for a builder whose runs stayed on the device: exactly one slab"""
    parts = list(b.finish_slabs())
    assert len(parts) == 1, f"{c.name}: {len(parts)} slabs"
    rec, tp, tc = parts[0]
    assert (b.n_records, b.n_trie) == (rec.shape[0], tp.shape[0]), c.name
    b.raw_records = rec
    if rec.dtype == formats.HALF_DTYPE:                              # (as fetch() rebuilds a halved result)
        km = (np.repeat(tp.astype(np.uint64), tc.astype(np.int64)) << np.uint64(30)) | rec["low"].astype(np.uint64)
        tid = b.taxids[rec["tax"].astype(np.int64)]
    elif c.K == 25:
        km = np.zeros(rec.shape[0], dtype=formats.KEY128_DTYPE)
        km["lo"], km["hi"] = rec["lo"], rec["hi"]
        tid = np.ascontiguousarray(rec["tax"])
    else:
        km, tid = np.ascontiguousarray(rec["kmer"]), np.ascontiguousarray(rec["tax"])
    return b.n_records, b.n_trie, (km, tid, tp, tc, b.fetch_freq())


def run_case(c, monkeypatch, by_slabs=False):
    """the case through one capi.Builder, everything compared with the reference; raises AssertionError with the case's name.
    by_slabs: finished by finish_slabs() (finish_begin / slab / fetch_slab / finish_end) instead of finish() + fetch()."""
    e = bc.expect(c)
    if c.edit_chunk:
        monkeypatch.setenv("KASA_EDIT_CHUNK_RECORDS", str(c.edit_chunk))
    else:
        monkeypatch.delenv("KASA_EDIT_CHUNK_RECORDS", raising=False)
    b = capi.Builder(c.content.array(), c.K, c.frames, None, c.brick)
    try:
        error = None
        for si, step in enumerate(c.steps):
            try:
                if step[0] == "add":
                    seqs = step[1]
                    off = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.int64)
                    b.add(np.frombuffer(b"".join(seqs), dtype=np.uint8), off, np.asarray(step[2], dtype=np.uint32), protein=step[3])
                elif step[0] == "index":
                    b.add_index(bc.records_array(step[1], c.K), step[2])
                elif step[0] == "drop":
                    b.drop_taxa(step[1])
                else:
                    b.shrink(step[1], step[2])
            except RuntimeError as ex:
                error = (si, _refusal(ex))
                break
        if error is None:
            try:
                if by_slabs:
                    n, m, fetched = _finish_by_slabs(b, c)
                else:
                    n, m = b.finish()
            except RuntimeError as ex:
                error = ("finish", _refusal(ex))
        if e.error is not None:
            assert error is not None and error[0] == e.error[0] and e.error[1] in error[1], f"{c.name}: refusal {error}, expected {e.error}"
            return
        assert error is None, f"{c.name}: refused at step {error[0]}: {error[1]}"
        km, tid, tp, tc, freq = fetched if by_slabs else b.fetch()
        wkm, wtid, wtp, wtc = bc.arrays(e, c.K)
        assert n == wkm.shape[0] and m == wtp.shape[0], f"{c.name}: {n} records and {m} trie entries, expected {wkm.shape[0]} and {wtp.shape[0]}"
        assert np.array_equal(km, wkm), f"{c.name}: k-mers differ, first at {_first_difference(km, wkm)} of {n}"
        assert np.array_equal(tid, wtid), f"{c.name}: tax IDs differ, first at {_first_difference(tid, wtid)} of {n}"
        assert np.array_equal(tp, wtp), f"{c.name}: trie prefixes differ, first at {_first_difference(tp, wtp)} of {m}"
        assert np.array_equal(tc, wtc), f"{c.name}: trie counts differ, first at {_first_difference(tc, wtc)} of {m}"
        rows, vals = bc.freq_sparse(e.freq, c.K)
        assert freq.shape == (c.content.n_rows, c.K), c.name
        assert np.array_equal(freq[rows], vals), f"{c.name}: frequency rows differ, first at content row {rows[_first_difference(freq[rows].sum(axis=1), vals.sum(axis=1))] if rows.shape[0] else -1}"
        assert np.count_nonzero(freq.any(axis=1)) == rows.shape[0], f"{c.name}: frequency rows that must be zero are not"
        if e.half is not None:
            raw = b.raw_records
            assert raw.dtype == formats.HALF_DTYPE and np.array_equal(raw["low"], np.asarray(e.half[0], dtype=np.uint32)), f"{c.name}: low 30 bits of the 6-byte records"
            assert np.array_equal(raw["tax"], np.asarray(e.half[1], dtype=np.uint16)), f"{c.name}: content rows of the 6-byte records"
        st, es = b.stats(), b.edit_stats()
        got = dict(pairs_in=st["pairs_in"], bricks=st["bricks"], merges=st["merges"], records_out=st["records_out"], index_in=es["index_in"],
                   dropped_delete=es["dropped_delete"], dropped_shrink=es["dropped_shrink"])
        assert got == e.stats, f"{c.name}: stats {got}, expected {e.stats}"
        for nb, want in e.hist.items():
            try:
                hist, distinct = b.taxa_histogram(nb)
            except RuntimeError as ex:
                assert isinstance(want, str) and want in _refusal(ex), f"{c.name}: taxa_histogram({nb}) refused: {ex}"
                continue
            assert not isinstance(want, str), f"{c.name}: taxa_histogram({nb}) must refuse: {want}"
            assert np.array_equal(hist, np.asarray(want[0], dtype=np.uint64)) and distinct == want[1], f"{c.name}: taxa_histogram({nb})"
    finally:
        b.close()


@pytest.mark.parametrize("family", SMALL_FAMILIES)
def test_family(family, monkeypatch):
    """Every case of the family; a case that differs is reported by name, and the others still run."""
    _gpu_or_fail()
    names = bc.case_names(family)
    failures = []
    for name in names:
        try:
            run_case(bc.case(name), monkeypatch)
        except AssertionError as ex:
            failures.append(str(ex))
    RAN[family] = len(names)
    assert not failures, "%d of %d cases differ:\n%s" % (len(failures), len(names), "\n".join(failures[:20]))


@pytest.mark.parametrize("name", bc.case_names("large", large=True))
def test_large(name, monkeypatch):
    """More items than one pass of grid_for's capped grid takes: one brick of more than 8192 * 256 pairs, two runs of more than
    8192 * 256 * MERGE_ITEMS merged outputs with a delete in the same builder, and an index of more than 8192 * 256 records through
    each shrink strategy."""
    _gpu_or_fail()
    c = bc.case(name)
    if "merge" in name:
        assert c.claim["merged_outputs"] > bc.GRID_CAP * bc.BLOCK * bc.MERGE_ITEMS
    elif "brick" in name:
        assert c.claim["pairs"] > bc.GRID_CAP * bc.BLOCK
    else:
        assert c.claim["records"] > bc.GRID_CAP * bc.BLOCK
    run_case(c, monkeypatch)
    RAN[name] = 1
    bc.case.cache_clear()


def _edits(c):
    return any(step[0] in ("index", "drop", "shrink") for step in c.steps)


def test_edited_builders_through_the_slab_calls(monkeypatch):
    """Every case of the small families with an index, drop or shrink step, refusals included, finished by finish_begin / slab /
    fetch_slab / finish_end as the C++ edit modes and `kasa_index merge` finish: one slab, everything else as in test_family."""
    _gpu_or_fail()
    names = [n for n in bc.case_names() if _edits(bc.case(n))]
    ran, failures = 0, []
    for name in names:
        try:
            run_case(bc.case(name), monkeypatch, by_slabs=True)
        except AssertionError as ex:
            failures.append(str(ex))
        ran += 1
    assert ran == sum(1 for f in SMALL_FAMILIES for n in bc.case_names(f) if _edits(bc.case(n))) and ran > 0
    assert not failures, "%d of %d cases differ:\n%s" % (len(failures), ran, "\n".join(failures[:20]))


def test_every_case_ran():
    """no case skipped, none excluded by a filter: the cases compared are the corpus's"""
    assert set(bc.families()) == set(SMALL_FAMILIES) | {"large"}
    small, large = bc.case_names(), bc.case_names("large", large=True)
    assert sum(len(bc.case_names(f)) for f in SMALL_FAMILIES) == len(small)
    assert {f: RAN.get(f) for f in SMALL_FAMILIES} == {f: len(bc.case_names(f)) for f in SMALL_FAMILIES}
    assert sum(RAN.get(n, 0) for n in large) == len(large) == 9
    assert sum(RAN.values()) == len(small) + len(large)


# ---- the C++ hosts: build, merge, shrink -s 2 on an amino-acid database with '^' letters ----------------------------------------------
PADS = os.path.join(helpers.GOLDEN, "dbedit", "halved_pads")


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _host(exe, args, cwd):
    r = subprocess.run([exe] + args + ["-m", "4", "-n", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, cwd=str(cwd))
    assert r.returncode == 0, r.stdout + r.stderr


def test_cpp_round_trip_build_merge_halve(tmp_path):
    _gpu_or_fail()
    host, tool = hipbuild.build_host(), hipbuild.build_index_tool()
    for side in ("a", "b"):
        _host(host, ["build", "-i", os.path.join(PADS, side + ".fasta"), "-c", os.path.join(PADS, side + "_content.txt"), "-d", str(tmp_path / side)], tmp_path)
        with open(str(tmp_path / (side + "_content.txt")), "wb") as f:
            f.write(_read(os.path.join(PADS, side + "_content.txt")))
    _host(tool, ["merge", "--firstIndex", str(tmp_path / "a"), "--secondIndex", str(tmp_path / "b"), "-o", str(tmp_path / "m")], tmp_path)
    _host(host, ["shrink", "-d", str(tmp_path / "m"), "-o", str(tmp_path / "h"), "-c", str(tmp_path / "m_content.txt"), "-s", "2"], tmp_path)
    # the plain reference on the sequences of both files
    full, half = (bc.reference(c) for c in bc.pads_cases(PADS))
    assert any(bc.letter(k, 5) == bc.PAD and bc.half_keeps(k) for k in full.kmers) and len(half.kmers) < len(full.kmers)
    rec = bc.records_array(list(zip(full.kmers, full.taxids)), 12)
    assert _read(str(tmp_path / "m")) == rec.tobytes() and _read(str(tmp_path / "m_info.txt")) == str(len(full.kmers)).encode()
    want = np.zeros(len(half.kmers), dtype=formats.HALF_DTYPE)
    want["low"], want["tax"] = half.half
    assert _read(str(tmp_path / "h")) == want.tobytes() and _read(str(tmp_path / "h_info.txt")) == b"%d\n3" % len(half.kmers)
    for prefix, e in (("m", full), ("h", half)):
        t = np.zeros(len(e.trie[0]), dtype=formats.TRIE_DTYPE)
        t["prefix"], t["count"] = e.trie
        assert _read(str(tmp_path / (prefix + "_trie"))) == t.tobytes() and _read(str(tmp_path / (prefix + "_trie.txt"))) == str(t.shape[0]).encode(), prefix
        got = formats.read_freq(str(tmp_path / prefix), 4)
        rows, vals = bc.freq_sparse(e.freq, 12)
        assert np.array_equal(got[rows], vals) and np.count_nonzero(got.any(axis=1)) == rows.shape[0], prefix
    # the files the reference's binary wrote for the same database
    for s in ("", "_info.txt", "_trie", "_trie.txt", "_f.txt"):
        assert _read(str(tmp_path / ("m" + s))) == _read(os.path.join(PADS, "idx" + s)), s
    for s in ("", "_info.txt", "_trie.txt", "_f.txt"):
        assert _read(str(tmp_path / ("h" + s))) == _read(os.path.join(PADS, "idx_half" + s)), s
    ours, theirs = formats.read_trie(str(tmp_path / "h")), formats.read_trie(os.path.join(PADS, "idx_half"))
    assert np.array_equal(ours[0], theirs[0]) and np.array_equal(ours[1][:-1], theirs[1][:-1])
    assert int(ours[1][-1]) == int(theirs[1][-1]) + 1 == 2 and int(ours[1].sum()) == len(half.kmers)   # Shrink.hpp:126-131 writes iCount - 1
