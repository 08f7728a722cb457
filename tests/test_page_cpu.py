"""The index pager without a device: its symbols are declared, exported and bound; the driver's argument rules for
--page-index hold (they are said before any device call); and tests/page_corpus.py is what it claims to be -- every good case
passes kasa_index_create's checks as restated in numpy, every refusal case violates exactly the one it names, at the place
it names."""
import os
import re
import subprocess

import numpy as np
import pytest

from kasa_amd import build as hipbuild
from kasa_amd import capi, formats, partition
from tests import helpers
from tests import lookup_corpus as lc
from tests import page_corpus as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = os.path.join(helpers.GOLDEN, "pairs")
NEW = ["kasa_index_pager_create", "kasa_index_pager_load", "kasa_index_pager_index", "kasa_index_pager_stats", "kasa_index_pager_tile",
       "kasa_index_pager_destroy", "kasa_ctx_set_index", "kasa_batch_pool_keep", "kasa_index_fetch"]


# ------------------------------------------------------------------------------------------------ the surface
def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "kasa_hip.h")).read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), name      # every one returns a status
        assert name in capi.EXPORTS and hasattr(L, name), name
    for cls, methods in ((capi.IndexPager, ("load", "index", "stats", "close")), (capi.Context, ("set_index", "pool_keep")),
                         (capi.DeviceIndex, ("fetch_arrays",)), (partition.PagedExchange, ("run_batch", "coherence", "close"))):
        for m in methods:
            assert callable(getattr(cls, m)), (cls, m)


def test_corpus_constants_are_the_librarys():
    assert capi.pager_tile() == (pc.T, pc.LDS_TAXA)
    # two workgroups per CU: 160 KiB of LDS, the widest tile's staging (20-byte records), 64 bytes of the tile's own words
    assert (5 + pc.T * 5 + 1) * 4 + 64 + pc.LDS_TAXA * 8 <= 160 * 1024 // 2 < (5 + pc.T * 5 + 1) * 4 + 64 + (pc.LDS_TAXA + 256) * 8


# ------------------------------------------------------------------------------------------------ the driver's argument rules
def _identify(extra):
    exe = hipbuild.build_host()
    cmd = [exe, "identify", "-c", os.path.join(PAIRS, "content.txt"), "-d", os.path.join(PAIRS, "idx"), "-i", os.path.join(PAIRS, "reads.fastq"), "-n", "1"] + list(extra)
    env = {k: v for k, v in os.environ.items() if k not in ("KASA_INDEX_PART_RECORDS", "KASA_INDEX_PAGE_RECORDS")}
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, env=env)


def _error(r):
    errors = [line for line in r.stderr.splitlines() if line.startswith("ERROR: ")]
    assert r.returncode == 1 and len(errors) == 1, (r.returncode, r.stderr)
    return errors[0]


@pytest.mark.parametrize("first", [True, False], ids=["before", "after"])
def test_page_index_is_refused_with_partition_devices(first):
    mine, other = ["--page-index"], ["--partition-devices", "0,0"]
    msg = _error(_identify(mine + other if first else other + mine))
    assert "--page-index" in msg and "--partition-devices" in msg


@pytest.mark.parametrize("value", ["", "0", "x", "12x", "4294967280", "99999999999"])
def test_page_records_wants_a_number(value):
    assert "--page-records" in _error(_identify(["--page-index", "--page-records", value]))


def test_parameters_file_keys(tmp_path):
    """PageIndex: true becomes --page-index, PageRecords: n becomes --page-records n.  Seen before any device call: pages of one
    record cannot be cut between the golden index's trie entries, and only a paged run looks at KASA_INDEX_PAGE_RECORDS."""
    exe = hipbuild.build_host()
    y = tmp_path / "config.yaml"
    base = f"Mode: identify\nIndex: {os.path.join(PAIRS, 'idx')}\nContentFile: {os.path.join(PAIRS, 'content.txt')}\nInputFileOrFolder: {os.path.join(PAIRS, 'reads.fastq')}\n"
    env = dict({k: v for k, v in os.environ.items() if k != "KASA_INDEX_PART_RECORDS"}, KASA_INDEX_PAGE_RECORDS="1")

    def run():
        return subprocess.run([exe, "--parameters", str(y)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=env)
    y.write_text(base + "PageIndex: true\nPageRecords: 0\n")
    assert "--page-records" in _error(run())
    y.write_text(base + "PageIndex: true\nPageRecords: 5000\n")
    assert "cannot be cut into partitions of at most 1 records" in _error(run())
    y.write_text(base + "PageIndex: false\n")
    assert "cannot be cut" not in run().stderr


# ------------------------------------------------------------------------------------------------ the corpus
def test_the_corpus_covers_what_it_lists():
    names = pc.good_names()
    for form, K, halved in pc.FORMS:
        for n in pc.SIZES:
            assert pc.case("%s size %d" % (form, n)).n == n
        assert sum(n.startswith(form + " edge") for n in names) == 6
    kinds = {w for n in pc.refusal_names() for w in [n.split(" refused ")[1].split(" at ")[0]]}
    assert kinds == {"unsorted", "duplicate", "wide", "unknown", "tix", "trie"}
    assert all(sum(n.endswith(place) for n in pc.refusal_names()) == 2 * 5 + 4 for place in pc.PLACES)


@pytest.mark.parametrize("name", pc.good_names())
def test_good_case_is_an_index(name):
    c = pc.case(name)
    v = pc.violations(c)
    assert v == {"order": 0, "unknown": 0, "tix": 0}, v
    assert pc.trie_describes(c)
    rec = c.records()
    assert rec.dtype.itemsize == c.record_bytes and rec.shape[0] == c.n == int(c.trie_count.sum())
    keys = pc.full_keys(c)
    assert all(k >> pc.BITS[c.K] == 0 for k in keys)
    # the file's records give the keys back; formats.make_index of the pairs is this index (sorted, unique, the same trie)
    ix = formats.make_index(lc.keys_from_ints(keys, c.K > 12), c.content.taxids[c.tix.astype(np.int64)], c.content)
    assert ix.n == c.n and lc.key_ints(ix.kmer) == keys
    assert np.array_equal(ix.trie_prefix, c.trie_prefix) and np.array_equal(ix.trie_count, c.trie_count)
    if c.halved:
        assert capi.index_records(ix, True).tobytes() == rec.tobytes()
    else:
        assert np.array_equal(ix.taxid, c.taxid) and capi.index_records(ix).tobytes() == rec.tobytes()
    k_, tax, meta, table, tb = pc.expected(name)
    assert np.array_equal(tax, ix.tax) and tb == lc.table_bits(c.n) and table.shape[0] == 1 << tb
    assert int(table[-1]) == c.n and (np.diff(table.astype(np.int64)) >= 0).all()
    low, high = (meta & 15, meta >> 4) if c.K == 12 else (meta & 255, meta >> 8)
    assert low[0] == 0 and high[0] == 0 and int(low.max()) <= c.K and (high <= c.K).all()


def _kind_at(c, i):
    keys = pc.full_keys(c)
    if i == 0 or keys[i] >> (5 * (c.K - 6)) != keys[i - 1] >> (5 * (c.K - 6)):
        return "P"
    return "T" if keys[i] == keys[i - 1] else "K"


@pytest.mark.parametrize("form,K,halved", pc.FORMS)
def test_named_places_hold_what_the_names_say(form, K, halved):
    T = pc.T
    for kind, at in pc.EDGES:
        c = pc.case("%s edge %s at %d" % (form, kind, at))
        assert _kind_at(c, at) == kind and c.n > T
        assert all(_kind_at(c, i) == "K" for i in range(T - 3, T + 3) if i != at)
    c = pc.case("%s forty" % form)
    keys = pc.full_keys(c)
    run = [i for i in range(c.n) if keys[i] == keys[T]]
    assert run == list(range(T - 20, T + 20)) and len(set(c.tix[run].tolist())) == 40
    for n_taxa in (pc.LDS_TAXA, pc.LDS_TAXA + 1):
        c = pc.case("%s taxa %d" % (form, n_taxa))
        assert c.content.n_taxa == n_taxa and c.n > T and len(set(c.tix.tolist())) > 500 and int(c.tix.max()) > n_taxa // 2
    c = pc.case("%s entries of one" % form)
    starts = np.concatenate(([0], np.cumsum(c.trie_count.astype(np.int64))))
    ones = {int(s) for s, n in zip(starts[:-1], c.trie_count) if n == 1}
    assert {T - 1, T} <= ones
    c = pc.case("%s entry over three tiles" % form)
    starts = np.concatenate(([0], np.cumsum(c.trie_count.astype(np.int64))))
    assert any(s // T + 2 == (e - 1) // T for s, e in zip(starts[:-1], starts[1:]))
    c = pc.case("%s 1000 entries in a tile" % form)
    starts = np.concatenate(([0], np.cumsum(c.trie_count.astype(np.int64))))[:-1]
    assert int(((starts >= T) & (starts < 2 * T)).sum()) >= 1000          # entries that begin inside the second tile


@pytest.mark.parametrize("name", pc.refusal_names())
def test_refusal_case_violates_what_it_names(name):
    c = pc.case(name)
    what, place = name.split(" refused ")[1].split(" at ")
    at = pc.PLACES[place]
    assert c.n == pc.REFUSAL_N and int(c.trie_count.sum()) == c.n
    v = pc.violations(c)
    if what == "tix":
        assert v["tix"] == 1 and int(c.tix[at]) == c.content.n_taxa and c.refusal == pc.BAD_TIX
    elif what == "unknown":
        assert v == {"order": 0, "unknown": 1, "tix": 0} and c.refusal == pc.UNKNOWN_TAX
    elif what == "trie" and not c.halved:
        assert v == {"order": 0, "unknown": 0, "tix": 0} and not pc.trie_describes(c) and c.refusal == pc.TRIE_DIFFERS
    else:
        assert v["order"] >= 1 and v["unknown"] == 0 and v["tix"] == 0 and c.refusal == pc.NOT_SORTED
        if what == "wide":
            assert pc.full_keys(c)[at] >> pc.BITS[c.K] == 1
