"""The corpus for the index builder and editor (tests/build_corpus.py) is what it claims to be -- one assertion per family, from the
plain model and from the constants as the sources name them -- and its plain reference agrees with the project's numpy helpers
(formats.make_index, trie_from_kmers, freq_from_index, write_index_halved, index_edit.shrink_thresholds, entropy_keeps,
test_merge_cpu.numpy_histogram) and with the oracle's encoder on every case.  The large family is built here at a small scale
by the functions that build it at full scale, and checked against the plain reference.  No device here:
tests/test_gpu_build_corpus.py runs the same cases through capi.Builder."""
import os
import re

import numpy as np
import pytest

from kasa_amd import formats, index_edit
from oracle import oracle
from tests import build_corpus as bc
from tests.test_merge_cpu import numpy_histogram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("unique", "illegal", "tiny", "bricks", "merge", "trie", "freq", "load", "delete", "nth", "halved", "hist", "large")


def _cases(family, **claim):
    out = [c for c in map(bc.case, bc.case_names(family)) if all(c.claim.get(k) == v for k, v in claim.items())]
    assert out, (family, claim)
    return out


def _source(name):
    return open(os.path.join(ROOT, "kasa_amd", "csrc", name)).read()


def _constant(text, name):
    """the value the sources give the named constant: an integer, 1 << n or 1ull << n"""
    m = re.search(r"\b%s\s*=\s*([^;,]+)[;,]" % re.escape(name), text)
    assert m, name
    v = m.group(1).strip().replace("ull", "").replace("u", "")
    m2 = re.fullmatch(r"(\d+)\s*<<\s*(\d+)", v)
    return int(m2.group(1)) << int(m2.group(2)) if m2 else int(v)


# ---- the constants ----------------------------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    build, edit, hip, radix = _source("kasa_build.h"), _source("kasa_edit.h"), _source("kasa_hip.hip"), _source("kasa_radix.h")
    assert _constant(build, "MERGE_ITEMS") == bc.MERGE_ITEMS
    assert _constant(build, "FREQ_LDS_CELLS") == bc.FREQ_LDS_CELLS
    assert _constant(edit, "TAXA_LDS_BINS") == bc.TAXA_LDS_BINS
    assert _constant(edit, "EDIT_CHUNK") == bc.EDIT_CHUNK
    assert _constant(hip, "ENC_LONG_MIN") == bc.ENC_LONG_MIN
    assert _constant(hip, "RANGE_LETTERS") == bc.TRIE_LETTERS == formats.TRIE_LETTERS
    m = re.search(r"grid_for\(uint64_t n, unsigned threads = (\d+), unsigned cap = (\d+)\)", build)
    assert m and (int(m.group(1)), int(m.group(2))) == (bc.BLOCK, bc.GRID_CAP)
    assert "__launch_bounds__(256) void bld_merge_kernel" in build and "<<<g, 256, 0, b->stream>>>" in build
    assert bc.MERGE_BLOCK == bc.BLOCK * bc.MERGE_ITEMS == 2048
    m = re.search(r"THREADS = (\d+),", radix)
    m2 = re.search(r"struct Tile \{ static constexpr int ITEMS = sizeof\(Key\) == 8 \? (\d+) : (\d+), SIZE = THREADS \* ITEMS; \};", radix)
    assert m and m2 and int(m.group(1)) * int(m2.group(2)) == bc.TILE32                   # a 4-byte key takes the second branch
    assert re.search(r"sort_pairs<uint32_t>\([^;]*\(uint32_t\)m, 0, %d," % bc.RANK_BITS, edit)
    assert "nTaxa >= (1u << 22)" in build and bc.MAX_TAXA == 1 << 22
    assert "(uint64_t)nRank * (KL + 1) <= (uint64_t)FREQ_LDS_CELLS" in build and "nRank <= (uint32_t)FREQ_LDS_CELLS" in edit
    assert "HALF_SIX_PADS" in edit and bc.HALF_SIX_PADS == formats.HALF_SIX_PADS == sum(bc.PAD << (5 * j) for j in range(6))
    # every loop the large family is there for sits behind grid_for's cap
    for kernel in ("bld_flag_kernel", "bld_scatter_kernel", "bld_emit_kernel", "bld_trie_flag_kernel", "bld_trie_scatter_kernel"):
        assert re.search(r"%s<Key><<<grid_for\(n\), 256," % kernel, build), kernel
    for kernel in ("edit_drop_flag_kernel<<<grid_for(n0)", "edit_half_flag_kernel<Key><<<grid_for(n1)", "edit_entropy_flag_kernel<Key><<<grid_for(n1)",
                   "edit_scatter_kernel<Key><<<grid_for(n)", "edit_iota_kernel<<<grid_for(m)", "edit_nth_flag_kernel<<<grid_for(m)",
                   "edit_load_kernel<uint64_t><<<grid_for(count)"):
        assert kernel in edit, kernel


def test_codon_table_is_the_oracles():
    assert list(bc.codon_lut()) == [int(x) for x in oracle.codon_table()]


def test_every_family_is_there_in_both_widths():
    assert tuple(bc.families()) == FAMILIES
    for f in FAMILIES:
        names = bc.case_names(f, large=f == "large")
        assert names and all(bc._MAKERS[n][0] == f for n in names)
        ks = {bc.case(n).K for n in names} if f != "large" else {int(n.rsplit("K", 1)[1]) for n in names}
        assert ks == ({12} if f == "halved" else {12, 25}), f
    for n in bc.case_names():
        c = bc.case(n)
        top = 1 << (5 * c.K)
        for step in c.steps:
            if step[0] == "index":
                assert all(0 <= k < top for k, _ in step[1]), n


# ---- the reference against the project's numpy helpers and the oracle's encoder ------------------------------------------------------
def _oracle_windows(c, seqs, protein):
    """per sequence the k-mers the oracle's encoder emits with kLow = 1 (none for the sequences whose k-mers the host makes)"""
    bases = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    off = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.int64)
    km, rd = oracle.encode(bases, off, oracle.params(c.K, 1, c.frames, K=c.K, protein=protein))
    ints = bc.key_ints(km)
    out = [[] for _ in seqs]
    for k, r in zip(ints, rd):
        out[int(r)].append(k)
    return out


def _numpy_model(c):
    """what the project's helpers make of the case: (k-mers, tax IDs, trie prefixes, counts, dense frequencies) and the keep mask's
    sizes; None for a case that refuses"""
    e = bc.expect(c)
    if e.error:
        return None
    keys, tax, drop, shrink = [], [], set(), None
    for step in c.steps:
        if step[0] == "add":
            _, seqs, taxids, protein = step
            mode = "protein" if protein else ("one" if c.frames == 1 else "dna")
            got = _oracle_windows(c, seqs, protein)
            for s, t, w in zip(seqs, taxids, got):
                mine = bc.protein_windows(s, c.K) if protein else bc.dna_windows(s, c.K, c.frames)
                if w:
                    assert w == mine, (c.name, s[:20])
                else:                                                   # the read geometry emits nothing: 1-2 letters, 3-4 or 3-8 bases
                    assert len(s) in bc.TINY[mode] or not mine, (c.name, len(s))
                for k in mine:
                    if protein or not bc.has_illegal(k, c.K):
                        keys.append(k)
                        tax.append(t)
        elif step[0] == "index":
            for k, t in bc.records_list(step[1], c.K):
                keys.append(k)
                tax.append(t)
        elif step[0] == "drop":
            drop.update(step[1])
        else:
            shrink = step[1:]
    content = formats.Content([""] * c.content.n_rows, c.content.array())
    ix = formats.make_index(bc.keys_array(keys, c.K), np.asarray(tax, dtype=np.uint32), content)
    keep = ~np.isin(ix.taxid, np.asarray(sorted(drop), dtype=np.uint32))
    km, tid = ix.kmer[keep], ix.taxid[keep]
    full = (km, tid)
    if shrink and shrink[0] == 1:
        dense = formats.dense_tax(tid, content)
        order = np.argsort(dense, kind="stable")
        first = np.searchsorted(dense[order], dense[order], side="left")
        ords = np.empty(tid.shape[0], np.int64)
        ords[order] = np.arange(tid.shape[0]) - first + 1
        table = index_edit.shrink_thresholds(shrink[1], int(ords.max())).astype(np.int64)
        assert table.tolist() == bc.nth_table(shrink[1], int(ords.max())), c.name
        k2 = ~np.isin(ords, table)
        km, tid = km[k2], tid[k2]
    elif shrink and shrink[0] == 3:
        k2 = np.asarray([index_edit.entropy_keeps([x for x in np.bincount(bc.letters_of(k, c.K)) if x], c.K) for k in bc.key_ints(km)], dtype=bool)
        km, tid = km[k2], tid[k2]
    elif shrink:
        k2 = (km & np.uint64(0x3FFFFFFF)) != np.uint64(formats.HALF_SIX_PADS)
        km, tid = km[k2], tid[k2]
    tp, tc = formats.trie_from_kmers(km)
    fk, ft = full if shrink and shrink[0] == 2 else (km, tid)
    return km, tid, tp, tc, formats.freq_from_index(fk, formats.dense_tax(ft, content), content.n_taxa)


def _same_as_model(c):
    model = _numpy_model(c)
    if model is None:
        return False
    e = bc.expect(c)
    km, tid, tp, tc = bc.arrays(e, c.K)
    assert np.array_equal(km, model[0]) and np.array_equal(tid, model[1]), c.name
    assert np.array_equal(tp, model[2]) and np.array_equal(tc, model[3]), c.name
    rows, vals = bc.freq_sparse(e.freq, c.K)
    mrows, mvals = bc.freq_sparse(model[4], c.K)
    assert np.array_equal(rows, mrows) and np.array_equal(vals, mvals), c.name
    for nb, h in e.hist.items():
        if not isinstance(h, str):
            assert np.array_equal(np.asarray(h[0], dtype=np.uint64), numpy_histogram(km, nb or c.content.n_rows + 1)) and h[1] == sum(h[0]), c.name
    return True


@pytest.mark.parametrize("family", FAMILIES[:-1])
def test_reference_agrees_with_the_numpy_helpers_and_the_oracle(family):
    done = sum(_same_as_model(bc.case(n)) for n in bc.case_names(family))
    refused = sum(bc.expect(bc.case(n)).error is not None for n in bc.case_names(family))
    assert done + refused == len(bc.case_names(family)) and done > 0


def test_halved_files_are_the_references(tmp_path):
    """formats.write_index_halved writes what the plain reference holds: records, trie, info and the full index's frequencies"""
    for c in _cases("halved"):
        e = bc.expect(c)
        recs = bc.records_list(c.steps[0][1], c.K)
        content = formats.Content(["n%d" % r for r in range(c.content.n_rows)], c.content.array())
        ix = formats.make_index(bc.keys_array([k for k, _ in recs], 12), np.asarray([t for _, t in recs], dtype=np.uint32), content)
        formats.write_index_halved(ix, str(tmp_path / "h"))
        n, kind = formats.read_info(str(tmp_path / "h"))
        half = np.fromfile(str(tmp_path / "h"), dtype=formats.HALF_DTYPE)
        assert (n, kind) == (len(e.kmers), 3) and half["low"].tolist() == e.half[0] and half["tax"].tolist() == e.half[1], c.name
        tp, tc = formats.read_trie(str(tmp_path / "h"))
        assert (tp.tolist(), tc.tolist()) == (e.trie[0], e.trie[1]) and int(tc.sum()) == n, c.name
        rows, vals = bc.freq_sparse(e.freq, c.K)
        got = formats.read_freq(str(tmp_path / "h"), content.n_taxa)
        assert np.array_equal(got[rows], vals) and np.count_nonzero(got.any(axis=1)) == rows.shape[0], c.name


def test_reference_binary_fixture_of_a_database_with_pad_letters(tmp_path):
    """tests/golden/dbedit/halved_pads/: what the reference's own binary wrote for `build` and `shrink -s 2` of an amino-acid database
    with '^' and '~'.  The plain reference and formats.write_index_halved give its records; the rule of letter 5 alone would not.  Its
    trie's last count is one short of the records it covers (Shrink.hpp:126-131 writes iCount - 1); the project writes the count."""
    d = os.path.join(ROOT, "tests", "golden", "dbedit", "halved_pads")
    full, half = (bc.reference(c) for c in bc.pads_cases(d))
    km, tid = formats.read_records(os.path.join(d, "idx"))
    assert km.tolist() == full.kmers and tid.tolist() == full.taxids
    tp, tc = formats.read_trie(os.path.join(d, "idx"))
    assert (tp.tolist(), tc.tolist()) == full.trie
    content = formats.read_content(os.path.join(d, "u_content.txt"))
    rows, vals = bc.freq_sparse(full.freq, 12)
    for name in ("idx", "idx_half"):                                    # the halved index keeps the full one's frequencies
        got = formats.read_freq(os.path.join(d, name), content.n_taxa)
        assert np.array_equal(got[rows], vals) and np.count_nonzero(got.any(axis=1)) == rows.shape[0]
    n, kind = formats.read_info(os.path.join(d, "idx_half"))
    rec = np.fromfile(os.path.join(d, "idx_half"), dtype=formats.HALF_DTYPE)
    assert (n, kind) == (len(half.kmers), 3) and rec["low"].tolist() == half.half[0] and rec["tax"].tolist() == half.half[1]
    by_letter_5 = [k for k in full.kmers if bc.letter(k, 5) != bc.PAD]
    assert len(by_letter_5) < n < len(full.kmers)
    tp, tc = formats.read_trie(os.path.join(d, "idx_half"))
    assert tp.tolist() == half.trie[0] and tc.tolist()[:-1] == half.trie[1][:-1] and int(tc[-1]) + 1 == half.trie[1][-1] == 2
    assert int(tc.sum()) == n - 1 and sum(half.trie[1]) == n
    ix = formats.make_index(km, tid, content)
    formats.write_index_halved(ix, str(tmp_path / "h"))
    for s in ("", "_info.txt", "_trie.txt", "_f.txt"):
        assert open(str(tmp_path / "h") + s, "rb").read() == open(os.path.join(d, "idx_half") + s, "rb").read(), s


# ---- the families' claims ----------------------------------------------------------------------------------------------------------------
def _raw_pairs(c):
    out = []
    for step in c.steps:
        if step[0] == "add":
            for s, t in zip(step[1], step[2]):
                out += [(k, t) for k in (bc.protein_windows(s, c.K) if step[3] else bc.dna_windows(s, c.K, c.frames))]
    return out


def test_unique():
    for c in _cases("unique"):
        e, raw = bc.expect(c), _raw_pairs(c)
        assert e.stats["pairs_in"] == len(raw) and e.stats["bricks"] == 1, c.name
        if "records" in c.claim:
            assert e.stats["records_out"] == c.claim["records"], c.name
        if "pairs_in" in c.claim:
            assert len(raw) == c.claim["pairs_in"], c.name
        if "runs" in c.claim:                                           # every distinct pair comes that many times
            counts = sorted(raw.count(p) for p in set(raw))
            assert counts == sorted(c.claim["runs"]), c.name
        if "taxa_of_kmer" in c.claim:
            assert sorted(e.kmers.count(k) for k in set(e.kmers)) == sorted(c.claim["taxa_of_kmer"]), c.name
            assert len(raw) == 2 * len(e.kmers)
        if "order" in c.claim:
            tax = c.steps[0][2]
            ranks = [c.content.rank(t) for t in tax]
            assert ranks != sorted(ranks) and len({k for k, _ in raw}) < len(set(raw)), c.name     # k-mers shared between taxa
            assert (ranks == sorted(ranks, reverse=True)) == (c.claim["order"] == "descending"), c.name
        if "rows_unsorted" in c.claim:
            assert c.content.rows != sorted(c.content.rows) and sorted(e.freq) == [1, 2, 3, 4], c.name
        if "zero_rows" in c.claim:
            assert all(c.content.rows.index(c.content.rows[r]) < r for r in c.claim["zero_rows"]), c.name
            assert not set(e.freq) & set(c.claim["zero_rows"]) and set(e.freq) == {1, 2, 4}, c.name
    assert {c.name.split("/")[1] for c in _cases("unique")} == {"all equal", "none equal", "runs tiny", "runs encoded", "ranks", "descending", "interleaved",
                                                               "content unsorted", "content repeats"}


def test_illegal_letters():
    assert len(bc.near_misses()) >= 2 and {s for _, _, s in bc.near_misses()} == {2, 3}   # the splits the codon table can produce
    assert (7, 25, 3) in bc.near_misses()
    for c in _cases("illegal"):
        e, raw = bc.expect(c), _raw_pairs(c)
        K = c.K
        if "positions" in c.claim:                                      # for every letter position a dropped k-mer whose only '_' is there
            alone = {tuple(j for j in range(K) if bc.letter(k, j) == bc.ILLEGAL) for k, _ in raw}
            assert {(j,) for j in range(K)} <= alone, c.name                   # K = 25: letter 12, in both words, among them
            assert not any(bc.has_illegal(k, K) for k in e.kmers) and 0 < len(e.kmers) < len(set(raw)), c.name
        if "kept" in c.claim:
            want = c.claim["kept"]
            assert len(want) == len({(a, b) for a, b, _ in bc.near_misses()}) * (K - 1) and set(want) <= set(e.kmers), c.name
            for k in want:                                              # five ones in a row, yet no letter is '_'
                assert any((k >> s) & 31 == 31 for s in range(5 * K - 4) if s % 5) and not bc.has_illegal(k, K), c.name
            seams = {s for k in want for s in range(5 * K - 4) if s % 5 and (k >> s) & 31 == 31}
            assert K == 12 or {62, 63} & seams, c.name                  # ... across the two words of a 128-bit key too
        if "bricks" in c.claim:
            assert (e.stats["bricks"], e.stats["merges"]) == (2, 1), c.name
            first, second = ([k for k in (bc.dna_windows(s, K, c.frames)) if not bc.has_illegal(k, K)] for s in c.steps[0][1])
            sizes = {"0, n": (False, True), "n, 0": (True, False), None: (False, False)}[c.claim.get("run_sizes")]
            assert (bool(first), bool(second)) == sizes, c.name
            assert (e.stats["records_out"] == 0) == (c.claim.get("records") == 0), c.name
            if c.claim.get("records") == 0:
                assert e.kmers == [] and e.trie == ([], []) and e.freq == {} and e.error is None and e.stats["pairs_in"] > 0, c.name
    assert {c.frames for c in _cases("illegal")} == {1, 3}


def test_tiny_and_long():
    for c in _cases("tiny"):
        e = bc.expect(c)
        if "windows" in c.claim:
            sizes = [len(s) for s in c.steps[0][1]]
            assert set(c.claim["windows"]) <= set(sizes) and min(sizes) == 1 and c.claim["windows"] == (bc.ENC_LONG_MIN - 1, bc.ENC_LONG_MIN, bc.ENC_LONG_MIN + 1)
            assert e.stats["pairs_in"] == sum(sizes) and e.stats["records_out"] < sum(sizes), c.name
            continue
        mode = c.name.split("/")[1]
        seqs = c.steps[0][1]
        tiny = [len(s) in bc.TINY[mode] for s in seqs]
        assert any(tiny) and e.stats["records_out"] > 0, c.name
        where = c.claim["where"]
        if where == "lengths":
            assert {len(s) for s in seqs} == set(bc.TINY[mode]) | {max(bc.TINY[mode]) + 1}, c.name
        elif where == "first":
            assert tiny[0] and not any(tiny[1:]) and e.stats["bricks"] == 1, c.name
        elif where == "last":
            assert tiny[-1] and not any(tiny[:-1]) and e.stats["bricks"] == 1, c.name
        elif where == "alone":
            assert e.stats["bricks"] == len(seqs) and e.stats["merges"] == len(seqs) - 1, c.name
        else:
            assert all(tiny) and e.stats["bricks"] == 1, c.name
    # the lengths whose k-mers the host makes: the read geometry (kLow = 1) emits from 3 letters, 5 bases, 9 bases (--one)
    assert bc.TINY == {"protein": (1, 2), "dna": (3, 4), "one": (3, 4, 5, 6, 7, 8)}


def test_brick_cuts():
    seen = set()
    for c in _cases("bricks"):
        e = bc.expect(c)
        assert (e.stats["bricks"], e.stats["merges"]) == (c.claim["bricks"], c.claim["merges"]) and e.stats["merges"] == e.stats["bricks"] - 1, c.name
        seen.add(e.stats["bricks"])
        which = c.name.split("/")[1]
        sizes = [len(s) for st in c.steps for s in st[1]]
        if which == "exact":
            assert sum(sizes) == c.brick and e.stats["bricks"] == 1
        elif which == "over by one":
            assert sum(sizes) == c.brick + 1
        elif which == "single larger":
            assert sizes[0] > c.brick and sizes[1] + sizes[2] <= c.brick
        elif which == "alphabet":
            assert e.stats["pairs_in"] < c.brick and [st[3] for st in c.steps] == [False, True]
    assert set(bc.BRICK_COUNTS) <= seen and bc.BRICK_COUNTS == (2, 3, 5, 7, 8, 9)


def _merged_once(c):
    (_, a, _), (_, b, _) = c.steps[:2]
    path = bc.merge_path(a, b)
    out = [(a if s == "A" else b)[i] for s, i in path]
    return a, b, path, out


def test_merge():
    sizes, remainders, twins, places = set(), set(), set(), set()
    for c in _cases("merge"):
        e = bc.expect(c)
        if len(c.steps) != 2 or c.steps[0][0] != "index":
            continue
        a, b, path, out = _merged_once(c)
        assert a == sorted(set(a)) and b == sorted(set(b)) and out == sorted(out), c.name
        assert [x for i, x in enumerate(out) if i == 0 or x != out[i - 1]] == list(zip(e.kmers, e.taxids)), c.name
        dup = [i for i in range(1, len(out)) if out[i] == out[i - 1]]
        assert all(path[i - 1][0] == "A" and path[i][0] == "B" for i in dup), c.name           # ties: A first
        what = c.name.split("/")[1]
        if what.startswith("sizes"):
            sizes.add((len(a), len(b)))
            assert not dup
        elif what.startswith("remainder"):
            remainders.add(len(out) % bc.MERGE_ITEMS)
            assert len(dup) == 1 and len(out) // bc.MERGE_ITEMS == 2
        elif what.startswith("twins"):
            twins.add(len(a))
            assert a == b and len(dup) == len(a) and len(e.kmers) == len(a)
        elif what.startswith("single twin"):
            assert dup == [c.claim["twin_at"][1]] and path[dup[0]] [0] == "B", c.name
            places.add(dup[0] - 1)
        elif what in ("A below B", "B below A"):
            assert (a[-1] < b[0]) == (what == "A below B") and (b[-1] < a[0]) == (what == "B below A") and not dup
    assert sizes == {(x, y) for x in bc.SIZE_EDGES for y in bc.SIZE_EDGES} and bc.SIZE_EDGES == (0, 1, 7, 8, 9)
    assert remainders == set(range(bc.MERGE_ITEMS))
    assert twins == set(range(1, 34)) | {bc.MERGE_BLOCK - 1, bc.MERGE_BLOCK, bc.MERGE_BLOCK + 1}
    # the twin's A copy is a thread's last output and its B copy the next thread's first (phase 7), and every other phase; and the same
    # across two workgroups
    assert {p % bc.MERGE_ITEMS for p in places} == set(range(bc.MERGE_ITEMS)) and bc.MERGE_BLOCK - 1 in places
    assert all(p >= 2 * bc.MERGE_ITEMS - 1 for p in places)
    for c in _cases("merge", same_kmer="A larger"):
        (_, a, _), (_, b, _) = c.steps
        assert a[0][0] == b[0][0] and a[0][1] > b[0][1] and bc.merge_path(a, b)[0] == ("B", 0)
    for c in _cases("merge", same_kmer="twin inside"):
        a, b, path, out = _merged_once(c)
        k = bc.ukey(5, c.K)
        run = [i for i, x in enumerate(out) if x[0] == k]
        dup = [i for i in run[1:] if out[i] == out[i - 1]]
        assert len(run) == 10 and len(dup) == 1 and run[1] < dup[0] < run[-1] and out[dup[0]] == (k, 40)
        assert [s for s, _ in path[dup[0] - 1:dup[0] + 1]] == ["A", "B"]
    W = 1 << 64
    for c in [bc.case(n) for n in bc.case_names("merge") if "/words/" in n]:
        a, b, path, out = _merged_once(c)
        keys = [k for k, _ in sorted(set(a + b))]
        los, his = [k % W for k in keys], [k // W for k in keys]
        which = c.claim["words"]
        if which == "equal hi":
            assert len(set(his)) == 1 and los == sorted(los) and any(x >> 63 for x in los) and any(not x >> 63 for x in los)
        elif which == "equal lo":
            assert len(set(los)) == 1 and his == sorted(his)
        else:                                                           # the low word alone, or compared first, orders them wrongly
            assert los != sorted(los) and sorted(keys, key=lambda k: (k % W, k // W)) != keys
    for c in [bc.case(n) for n in bc.case_names("merge") if "/mixed/" in n]:
        e = bc.expect(c)
        assert e.stats["merges"] == c.claim["merges"] and e.stats["bricks"] == c.claim.get("bricks", 0), c.name
        assert e.stats["records_out"] < e.stats["index_in"] + e.stats["pairs_in"], c.name                  # duplicates between the sources


def test_trie():
    for c in _cases("trie"):
        e = bc.expect(c)
        assert tuple(e.trie[1]) == c.claim["counts"] and e.trie[0] == sorted(set(e.trie[0])), c.name
        shift = 5 * (c.K - bc.TRIE_LETTERS)
        which = c.name.split("/")[1]
        if which == "bit shift":
            assert all((x ^ y) == 1 << shift or bin(x ^ y).count("1") > 1 and (x ^ y) >> shift for x, y in zip(e.kmers, e.kmers[1:]))
            assert e.kmers[0] ^ e.kmers[1] == 1 << shift
        elif which == "bit below shift":
            assert e.kmers[0] ^ e.kmers[1] == 1 << (shift - 1) and e.kmers[2] ^ e.kmers[3] == 1 << (shift - 1)
        elif which == "runs":
            assert e.trie[1][:4] == [1, bc.BLOCK - 1, bc.BLOCK, bc.BLOCK + 1] and e.trie[1][-1] == 3


def test_frequencies():
    assert {K: bc.freq_ranks(K) for K in bc.KS} == {12: (1260, 1261), 25: (630, 631)}
    sides = set()
    for c in _cases("freq"):
        e, K = bc.expect(c), c.K
        n = c.content.n_ranks
        sides.add((K, n * (K + 1) <= bc.FREQ_LDS_CELLS))
        assert c.claim["lds"] == (n * (K + 1) <= bc.FREQ_LDS_CELLS), c.name
        if "ranks at" in c.name:
            assert n * (K + 1) <= bc.FREQ_LDS_CELLS < (n + 1) * (K + 1), c.name
        if "ranks past" in c.name:
            assert (n - 1) * (K + 1) <= bc.FREQ_LDS_CELLS < n * (K + 1), c.name
        ranks = {c.content.rank(t) for t in e.taxids}
        assert {1, n - 1} <= ranks, c.name
        trailing, inner_alone, inner_over_run = set(), set(), set()
        for k in e.kmers:
            let = [bc.letter(k, j) for j in range(K)]
            t = next((j for j in range(K) if let[j] != bc.PAD), K)
            inner = [j for j in range(t, K) if let[j] == bc.PAD]
            if not inner:
                trailing.add(t)
            elif len(inner) == 1:
                (inner_alone if t == 0 else inner_over_run).add(inner[0])
        assert trailing == set(range(K + 1)) and inner_alone == set(range(1, K)) and inner_over_run == set(range(2, K)), c.name
        assert bc.padded([], K) in e.kmers, c.name                      # the all-'^' k-mer, from the sequences ^^^ and ^
        if "repeated" in c.name:
            assert c.content.rows.count(3) == 2 and not {5, 6} & set(e.freq), c.name
    assert sides == {(12, True), (12, False), (25, True), (25, False)}


def test_load_checks():
    seen = set()
    for c in _cases("load"):
        e = bc.expect(c)
        bad = c.claim["bad"]
        seen.add(c.name.split("/")[1])
        if bad is None:
            assert e.error is None and e.stats["index_in"] == sum(len(s[1]) for s in c.steps), c.name
            continue
        assert e.error[0] == 0 and ("record %d " % bad) in e.error[1], c.name
        recs = c.steps[0][1]
        faults = [i for i in range(len(recs)) if not c.content.knows(recs[i][1]) or (i and not recs[i - 1] < recs[i])]
        assert faults[0] == bad, c.name
        if "two bad" in c.name:
            assert len(faults) >= 2 and (c.steps[0][2] == 0 or faults[0] < c.steps[0][2] <= faults[-1]), c.name
        if "between chunks" in c.name:
            assert bad == c.steps[0][2]
        if "id " in c.name:
            assert "does not list" in e.error[1] and (recs[bad][1] < min(c.content.rows) or recs[bad][1] > max(c.content.rows)), c.name
        W = 1 << 64
        if "hi only" in c.name:
            assert recs[bad][0] // W < recs[bad - 1][0] // W and recs[bad][0] % W > recs[bad - 1][0] % W
        if "lo only" in c.name:
            assert recs[bad][0] // W == recs[bad - 1][0] // W and recs[bad][0] % W < recs[bad - 1][0] % W
    for c in _cases("load", bad=None):
        if "second run" in c.name:
            assert c.steps[1][1][0] < c.steps[0][1][-1] and len(c.steps) == 2
    assert seen >= {"swap", "duplicate", "descending id", "id below", "id above", "between chunks", "chunk of one", "two bad", "two bad, two chunks",
                    "hi only", "lo only", "second run below"}


def test_delete():
    for c in _cases("delete"):
        e = bc.expect(c)
        n = c.claim["n"]
        assert e.stats["index_in"] == n and e.stats["dropped_delete"] == n - len(e.kmers), c.name
        which = c.claim["drop"]
        if which == "every":
            assert e.stats["dropped_delete"] == n and e.kmers == [] and e.error is None and e.hist[0] == ([0] * (c.content.n_rows + 1), 0), c.name
        elif which == "unknown ids":
            assert e.stats["dropped_delete"] == 0 and not any(c.content.knows(t) for t in c.steps[1][1]), c.name
        elif which == "top rank":
            assert c.content.rank(c.steps[1][1][0]) == c.content.n_ranks - 1 and 0 < e.stats["dropped_delete"] < n, c.name
        else:
            assert 0 < e.stats["dropped_delete"] < n, c.name


def _rank_digits(c):
    ranks = np.asarray([c.content.rank(t) for _, t in c.steps[0][1]])
    return [set(((ranks >> (8 * p)) & 255).tolist()) for p in range(bc.RANK_BITS // 8)]


def test_every_nth():
    seen_P, seen_sizes, seen_chunks = set(), set(), set()
    for c in _cases("nth"):
        e = bc.expect(c)
        which, arg, P = c.claim["which"], c.claim["arg"], c.claim["P"]
        recs = c.steps[0][1]
        taxa = [t for _, t in recs]
        largest = max(taxa.count(t) for t in set(taxa))
        if which == "percentage":
            seen_P.add(P)
            if P == 100.0:
                assert e.error == ("finish", "strategy 1 leaves no record of the %d" % len(recs)), c.name
            elif P in (0.0, 150.0):
                assert e.stats["dropped_shrink"] == 0, c.name
            else:
                share = e.stats["dropped_shrink"] / len(recs)
                assert abs(share - abs(P) / 100) < 0.02, (c.name, share)
            continue
        assert e.error is None and 0 < e.stats["dropped_shrink"] < len(recs), c.name
        if which == "taxon size":
            seen_sizes.add(largest)
            assert largest == arg and (arg in bc.nth_table(P, arg)) == (arg % 2 == 0), c.name
        elif which == "chunk":
            seen_chunks.add(c.edit_chunk)
            assert c.edit_chunk == arg and len(recs) > 2 * arg and (arg < 3 or len(recs) % arg), c.name
        elif which == "drop positions":                                  # a dropped record ends a chunk, another opens the next
            kept = set(zip(e.kmers, e.taxids))
            gone = [i for i, r in enumerate(recs) if r not in kept]
            assert {c.edit_chunk - 1, c.edit_chunk} <= set(gone) and 2 * c.edit_chunk - 1 in gone, c.name
            first = [i for i in gone if i < c.edit_chunk]
            assert all(taxa[:i].count(taxa[i]) % 2 == 1 for i in gone), c.name                               # P = 50: a taxon's even ordinals
            assert any(taxa.index(taxa[i]) < c.edit_chunk <= i for i in gone) and first, c.name               # ... whose first lies a chunk back
        elif which == "one rank":
            assert len(set(taxa)) == 1 and len(recs) > 2 * bc.TILE32 and all(len(d) == 1 for d in _rank_digits(c)), c.name
        else:
            d = _rank_digits(c)
            what = c.name.split("/")[1]
            if what == "multiples of 256":
                assert d[0] == {0} and len(d[1]) == 6 and d[2] == {0}, c.name
            elif what.startswith("multiples of 65536"):
                assert c.content.n_ranks == 70000 and d[2] == {0, 1} and d[0] == {0}, c.name
            elif what.startswith("top ranks"):
                assert c.content.n_ranks == bc.MAX_TAXA - 1 and d[2] == {63} and max(c.content.rank(t) for t in taxa) == bc.MAX_TAXA - 2, c.name
            else:
                n = c.content.n_ranks
                assert (n <= bc.FREQ_LDS_CELLS) == ("at the LDS limit" in what) and abs(n - bc.FREQ_LDS_CELLS) <= 1, c.name
                assert max(c.content.rank(t) for t in taxa) == n - 1, c.name
    assert seen_P == set(bc.PERCENTAGES) and bc.PERCENTAGES == (50.0, 25.0, float(np.float32(66.67)), 99.0, -37.5, 0.0, 150.0, 100.0)
    assert seen_sizes == {31, 32, 33, 63, 64, 65} and seen_chunks == {1, 2, bc.TILE32 - 1, bc.TILE32, bc.TILE32 + 1}


def test_halved():
    six = bc.HALF_SIX_PADS
    for c in _cases("halved"):
        e = bc.expect(c)
        recs = c.steps[0][1]
        gone = [r for r in recs if r[0] & 0x3FFFFFFF == six]
        letter5 = [r for r in recs if bc.letter(r[0], 5) == bc.PAD and r[0] & 0x3FFFFFFF != six]
        assert letter5 and set(letter5) <= set(zip(e.kmers, e.taxids)), c.name              # the rule of letter 5 alone would drop these
        assert e.stats["dropped_shrink"] == len(gone) and sum(e.trie[1]) == len(e.kmers) and 0 not in e.trie[1], c.name
        assert e.hist[0] == "halved", c.name
        which = c.claim["which"]
        if which == "six pads":
            assert any(bc.letter(k, 6) != bc.PAD for k, _ in gone)
        elif which == "all pads":
            assert (bc.padded([], 12), 33) in gone or any(k == bc.padded([], 12) for k, _ in gone)
        elif which == "dropped first":
            assert recs[0] in gone and (recs[0][0] >> 30) in e.trie[0]
        elif which == "first prefix dropped":                            # no entry of no records for the prefix that lost them all
            assert recs[0] in gone and (recs[0][0] >> 30) not in e.trie[0]
        elif which == "dropped last":
            assert recs[-1] in gone
        elif which == "first of its prefix":
            p = gone[0][0] >> 30
            assert min(r for r in recs if r[0] >> 30 == p) in gone and p in e.trie[0]
        elif which == "content repeats":
            assert set(e.half[1]) <= {1, 2, 4} and not {3, 5} & set(e.freq)
        if which != "content repeats":
            assert gone or which == "letter 5"


def test_taxa_histogram():
    for c in _cases("hist"):
        e = bc.expect(c)
        which = c.claim["which"]
        n_rows = c.content.n_rows
        if which == "runs":
            bins, distinct = e.hist[0]
            assert [i for i, x in enumerate(bins) if x] == [1, 2, 3, bc.TAXA_LDS_BINS - 1, bc.TAXA_LDS_BINS, bc.TAXA_LDS_BINS + 1, n_rows]
            assert bins[1] == 2 and distinct == 8 and e.kmers[-1] == e.kmers[-3] != e.kmers[-4], c.name
        elif which == "longest refused":
            assert e.hist[n_rows].startswith("the k-mer that ends at record %d carries %d records" % (sum(bc.HIST_RUNS) + n_rows - 1, n_rows)), c.name
            assert e.hist[n_rows + 1] == bc.expect(bc.case(c.name.replace("longest refused", "runs"))).hist[0], c.name
        elif which == "few bins":
            assert e.hist[5][0] == [0, 2, 1, 1, 2] and e.hist[4] == "the k-mer that ends at record 4 carries 4 records or more", c.name
            assert e.hist[0][0][:5] == e.hist[5][0] and 5 < bc.TAXA_LDS_BINS
        elif which == "equal words":
            W = 1 << 64
            ks = sorted(set(e.kmers))
            assert any(x // W == y // W for x, y in zip(ks, ks[1:])) and any(x % W == y % W for x, y in zip(ks, ks[1:])) and e.hist[0][0][2] == 5
        else:
            plain = bc.expect(bc.case(c.name.replace(which, "runs")))
            assert e.hist[0] != plain.hist[0] and e.stats["dropped_delete" if which == "after delete" else "dropped_shrink"] > 0, c.name


# ---- the large family ------------------------------------------------------------------------------------------------------------------------
def _same_expect(a, b, K, n_rows):
    for x, y in zip(bc.arrays(a, K), bc.arrays(b, K)):
        assert np.array_equal(x, y)
    for x, y in zip(bc.freq_sparse(a.freq, K), bc.freq_sparse(b.freq, K)):
        assert np.array_equal(x, y)
    assert a.stats == b.stats
    for nb in a.hist:
        assert list(a.hist[nb][0]) == list(b.hist[nb][0]) and a.hist[nb][1] == b.hist[nb][1]
    if a.half is not None:
        assert [int(x) for x in a.half[0]] == b.half[0] and [int(x) for x in a.half[1]] == b.half[1]


@pytest.mark.parametrize("K", bc.KS)
def test_large_merge_scaled_down(K):
    """the construction of the full-size case at M = 3000: its analytic result is the plain reference's"""
    c = bc.large_merge(K, **bc.SMALL_MERGE)
    _same_expect(c.expected, bc.reference(c), K, c.content.n_rows)
    assert c.claim["twins"] == len(range(0, bc.SMALL_MERGE["M"], 6)) and c.expected.stats["dropped_delete"] > 0
    # full size: more merged outputs than one pass of the capped grid takes, written down without building the case
    M = bc.LARGE_MERGE["M"]
    outputs = len(range(0, M, 2)) + len(range(0, M, 3))
    assert outputs > bc.GRID_CAP * bc.BLOCK * bc.MERGE_ITEMS and outputs - bc.GRID_CAP * bc.BLOCK * bc.MERGE_ITEMS < 100_000
    assert (1 << 22) > bc.GRID_CAP * bc.BLOCK and len(range(0, M, 3)) > (1 << 22)            # the second run loads in chunks a thread loops over
    assert (M // bc.LARGE_MERGE["T"] + 1) * bc.stride(K) < 1 << (5 * K)
    prefixes = (M // bc.LARGE_MERGE["T"] + 1) * bc.stride(K) >> (5 * (K - bc.TRIE_LETTERS))
    assert prefixes > 2000


@pytest.mark.parametrize("K", bc.KS)
def test_large_brick_scaled_down(K):
    """every string of 3 letters over 5 as a sequence: the analytic result is the plain reference's; full size: one brick just past
    one pass of the capped grid (bld_flag_kernel, bld_scatter_kernel and the sort over all key bits)"""
    c = bc.large_brick(K, **bc.SMALL_BRICK)
    _same_expect(c.expected, bc.reference(c), K, c.content.n_rows)
    A, L = bc.SMALL_BRICK["A"], bc.SMALL_BRICK["L"]
    assert c.expected.stats["pairs_in"] == A ** L * L and c.expected.stats["records_out"] == 3 * sum(A ** i for i in range(1, L)) + A ** L
    A, L = bc.LARGE_BRICK["A"], bc.LARGE_BRICK["L"]
    assert bc.GRID_CAP * bc.BLOCK < A ** L * L < 1.3 * bc.GRID_CAP * bc.BLOCK and L >= 3       # every sequence goes through the encoder


@pytest.mark.parametrize("K,strategy", [(12, 1), (12, 2), (12, 3), (25, 1), (25, 3)])
def test_large_shrink_scaled_down(K, strategy):
    c = bc.large_shrink(K, strategy, bc.LARGE_P, **bc.SMALL_SHRINK)
    _same_expect(c.expected, bc.reference(c), K, c.content.n_rows)
    decided = c.claim["decided"]
    if strategy == 2:                                                    # '^' at letter 5 over a real letter stays, six '^' go
        assert decided == {"one letter": True, "distinct": True, "inner pad": True, "pads": False}
    elif strategy == 3:
        assert decided["one letter"] is False and decided["distinct"] is True and len(set(decided.values())) == 2
    else:
        assert 0 < decided["ordinals dropped"] < bc.SMALL_SHRINK["n_perm"] * 4
    n = bc.LARGE_SHRINK["n_perm"] * len(bc.shrink_templates(K)) * bc.LARGE_SHRINK["T"]
    assert 0 < n - bc.GRID_CAP * bc.BLOCK < 10_000                       # full size: just past one pass of the capped grid
    assert sorted(bc.case_names("large", large=True)) == sorted(["large/brick/K12", "large/brick/K25", "large/merge/K12", "large/merge/K25", "large/shrink 1/K12", "large/shrink 2/K12",
                                                                  "large/shrink 3/K12", "large/shrink 1/K25", "large/shrink 3/K25"])
