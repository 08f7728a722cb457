"""The index pager on the device (kasa_index_pager_*, kasa_ctx_set_index, kasa_batch_pool_keep, partition.PagedExchange,
`kasa_identify identify --page-index`).

A slot must hold exactly what kasa_index_create makes of the same records -- byte for byte, for every case of
tests/page_corpus.py and for the golden indices --, whatever the slot held before; a refusal is kasa_index_create's, leaves
the slot empty and harms nothing; and a batch run slice by slice against partitions that come and go equals the run against
the whole index bit for bit.  No test provokes a fault: the refusals are status codes the host reads from a counter block."""
import ctypes as C
import gzip
import lzma
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from kasa_amd import build as hipbuild
from kasa_amd import capi, formats, partition, reads
from tests import helpers
from tests import page_corpus as pc
from tests.test_coherence import COH
from tests.test_gpu_cpp_host import FLAGS, PAIRS, _read, unpack, wants_coverage
from tests.test_gpu_parity import synthetic_world

pytestmark = pytest.mark.gpu

KASA_E_ARG, KASA_E_STATE, KASA_E_LIMIT = 1, 4, 5
MAX_RECORDS = 3 * pc.T + 16                                       # the largest corpus case: an entry over three tiles
GOLD = os.path.join(helpers.GOLDEN, "pairs")


# ------------------------------------------------------------------------------------------------ helpers
_PAGERS = {}


def _pager(record_bytes, content, max_records=MAX_RECORDS):
    """one pager per (record size, content) for the whole module: every load goes into a slot others have used"""
    key = (record_bytes, content.n_taxa, max_records)
    if key not in _PAGERS:
        _PAGERS[key] = capi.IndexPager(max_records, record_bytes, content.taxids, slots=2)
    return _PAGERS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_pagers():
    yield
    for p in _PAGERS.values():
        p.close()
    _PAGERS.clear()


def _create(c):
    """kasa_index_create on a corpus case's records -> (status, message, DeviceIndex or None)"""
    rec, ids = c.records(), np.ascontiguousarray(c.content.taxids, dtype=np.uint32)
    tp, tc = np.ascontiguousarray(c.trie_prefix, dtype=np.uint32), np.ascontiguousarray(c.trie_count, dtype=np.uint64)
    h = C.c_void_p()
    rc = capi.lib().kasa_index_create(C.c_int(0), capi._p(rec), C.c_uint64(c.n), C.c_int(c.record_bytes), capi._p(tp), capi._p(tc), C.c_uint64(tp.shape[0]),
                                      capi._p(ids), C.c_uint32(ids.shape[0]), C.byref(h))
    if rc:
        return rc, capi.lib().kasa_last_error().decode(), None
    d = capi.DeviceIndex.__new__(capi.DeviceIndex)
    d.h, d.device, d.n_taxa, d.n, d.wide = h, 0, int(ids.shape[0]), c.n, c.K > 12
    return 0, "", d


def _load(pg, slot, part_id, c):
    pg.load(slot, part_id, c.records(), c.trie_prefix, c.trie_count)


def _assert_same_arrays(got, want, what):
    for name, a, b in zip(("keys", "taxa", "meta", "table"), got[:4], want[:4]):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name)
    assert got[4] == want[4], (what, "tb")


_NEXT_ID = [1000]


def _fresh_id():
    _NEXT_ID[0] += 1
    return _NEXT_ID[0]


# ------------------------------------------------------------------------------------------------ slot against kasa_index_create
@pytest.mark.parametrize("name", pc.good_names())
def test_slot_equals_created_index(name):
    c = pc.case(name)
    pg = _pager(c.record_bytes, c.content)
    before = pg.stats()
    _load(pg, 0, _fresh_id(), c)
    after = pg.stats()
    assert after["loads"] == before["loads"] + 1 and after["bytes"] - before["bytes"] >= c.n * c.record_bytes
    assert after["lds_table"] == (not c.halved and c.content.n_taxa <= pc.LDS_TAXA)
    got = pg.index(0).fetch_arrays()
    rc, msg, dix = _create(c)
    assert rc == 0, msg
    _assert_same_arrays(got, dix.fetch_arrays(), name)
    dix.close()
    _assert_same_arrays(got, pc.expected(name), name + " (restatement)")


@pytest.mark.parametrize("stem", ["idx", "idx25", "idx_half"])
def test_golden_index_in_a_slot(stem):
    """the reference's own files: the 64-bit index, the one of `build --kH 25`, the halved one of `shrink -s 2` as it lies on disk"""
    d, ix = helpers.load_case("pairs", stem)
    n, kind = formats.read_info(os.path.join(d, stem))
    rb = {0: 12, 128: 20, 3: 6}[kind]
    raw = np.fromfile(os.path.join(d, stem), dtype=np.uint8)
    assert raw.shape[0] == n * rb
    pg = capi.IndexPager(n, rb, ix.content.taxids, slots=1)
    pg.load(0, 7, raw, ix.trie_prefix, ix.trie_count)
    dix = capi.DeviceIndex(ix)
    _assert_same_arrays(pg.index(0).fetch_arrays(), dix.fetch_arrays(), stem)
    pg.load(0, 7, raw, ix.trie_prefix, ix.trie_count)
    assert pg.stats()["hits"] == 1 and pg.stats()["loads"] == 1
    dix.close(); pg.close()


@pytest.mark.parametrize("form,K,halved", pc.FORMS)
def test_slot_reuse_leaves_nothing_behind(form, K, halved):
    big, one = pc.case("%s entry over three tiles" % form), pc.case("%s size 1" % form)
    pg = _pager(big.record_bytes, big.content)
    _load(pg, 1, _fresh_id(), big)
    assert pg.index(1).n == big.n
    _load(pg, 1, _fresh_id(), one)
    rc, msg, dix = _create(one)
    assert rc == 0, msg
    got = pg.index(1).fetch_arrays()
    assert got[3].shape[0] == 256 and got[4] == 8
    _assert_same_arrays(got, dix.fetch_arrays(), form)
    dix.close()


# ------------------------------------------------------------------------------------------------ hits and the bind rule
def test_hits_and_the_bind_rule():
    a, b = pc.case("k12 size %d" % (pc.T + 1)), pc.case("k12 size %d" % pc.T)
    pg = capi.IndexPager(MAX_RECORDS, 12, a.content.taxids, slots=2)
    _load(pg, 0, 5, a)
    s0 = pg.stats()
    _load(pg, 0, 5, a)                                                # the same partition: a hit, nothing is copied
    s1 = pg.stats()
    assert (s1["loads"], s1["hits"], s1["bytes"]) == (s0["loads"], s0["hits"] + 1, s0["bytes"]) == (1, 1, s0["bytes"])
    with pytest.raises(RuntimeError) as e:
        pg.index(1)                                                   # an empty slot
    assert e.value.code == KASA_E_STATE
    ctx = capi.Context(pg.index(0), 12, 7, 3)                          # a context made on a slot is bound to it
    with pytest.raises(RuntimeError) as e:
        _load(pg, 0, 6, b)
    assert e.value.code == KASA_E_STATE and "bound" in str(e.value)
    assert pg.index(0).n == a.n                                       # ... and the slot is as it was
    _load(pg, 1, 6, b)
    ctx.set_index(pg.index(1))                                        # rebinding releases slot 0 and takes slot 1
    _load(pg, 0, 7, b)
    with pytest.raises(RuntimeError) as e:
        _load(pg, 1, 8, a)
    assert e.value.code == KASA_E_STATE
    ctx.close()                                                       # destroying the context releases its slot
    _load(pg, 1, 8, a)
    rc, msg, dix = _create(a)
    _assert_same_arrays(pg.index(1).fetch_arrays(), dix.fetch_arrays(), "after the bind rule")
    # the other refusals of kasa_ctx_set_index: key width and number of taxa
    wide = pc.case("k25 size 2")
    rc, msg, dw = _create(wide)
    ctx = capi.Context(dix, 12, 7, 3)
    with pytest.raises(RuntimeError) as e:
        ctx.set_index(dw)
    assert e.value.code == KASA_E_ARG
    more = pc.case("k12 taxa %d" % pc.LDS_TAXA)
    rc, msg, dm = _create(more)
    with pytest.raises(RuntimeError) as e:
        ctx.set_index(dm)
    assert e.value.code == KASA_E_ARG
    ctx.close(); dm.close(); dw.close(); dix.close(); pg.close()


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("name", pc.refusal_names())
def test_refusal_is_kasa_index_creates(name):
    c = pc.case(name)
    good = pc.case("%s size 2" % name.split(" ")[0])
    rc, msg, dix = _create(c)
    assert rc == KASA_E_ARG and dix is None and c.refusal in msg, msg
    pg = _pager(c.record_bytes, c.content)
    before = pg.stats()
    _load(pg, 0, _fresh_id(), good)
    with pytest.raises(RuntimeError) as e:
        _load(pg, 0, _fresh_id(), c)
    assert e.value.code == rc and str(e.value) == msg                  # the code and the text, violation counts included
    with pytest.raises(RuntimeError) as e:
        pg.index(0)                                                    # the slot is empty
    assert e.value.code == KASA_E_STATE
    after = pg.stats()
    assert after["refused"] == before["refused"] + 1 and after["loads"] == before["loads"] + 1
    _load(pg, 0, _fresh_id(), good)                                     # the next good load lands
    rc, msg, dix = _create(good)
    _assert_same_arrays(pg.index(0).fetch_arrays(), dix.fetch_arrays(), name)
    dix.close()


@pytest.mark.parametrize("form,K,halved", pc.FORMS)
def test_more_records_than_a_slot_holds(form, K, halved):
    c = pc.case("%s size %d" % (form, pc.T + 1))
    pg = capi.IndexPager(pc.T, c.record_bytes, c.content.taxids, slots=1)
    with pytest.raises(RuntimeError) as e:
        _load(pg, 0, 1, c)
    assert e.value.code == KASA_E_LIMIT and str(pc.T + 1) in str(e.value)
    with pytest.raises(RuntimeError) as e:
        pg.index(0)
    assert e.value.code == KASA_E_STATE
    _load(pg, 0, 2, pc.case("%s size %d" % (form, pc.T)))
    assert pg.index(0).n == pc.T
    pg.close()


def test_a_sole_record_with_a_bit_beyond_the_width():
    """kasa_index_create's order check begins at record 1 and never looks at a sole record; the pager does (its table marks are
    guarded either way).  Not compared with kasa_index_create."""
    c = pc.case("k12 size 1")
    rec = c.records().copy()
    rec["kmer"] |= np.uint64(1 << 60)
    pg = _pager(12, c.content)
    with pytest.raises(RuntimeError) as e:
        pg.load(0, _fresh_id(), rec, c.trie_prefix, c.trie_count)
    assert e.value.code == KASA_E_ARG and pc.NOT_SORTED in str(e.value)


# ------------------------------------------------------------------------------------------------ PagedExchange against the whole index
_WHOLE = {}


def _whole(key, ix, batch, kh, kl, frames, unique=False, coherence=False):
    """the unpartitioned run, once per setting: (scores CSR, profile limbs, coherence or None)"""
    if key not in _WHOLE:
        dix = capi.DeviceIndex(ix)
        ctx = capi.Context(dix, kh, kl, frames)
        ctx.run_batch(batch.bases, batch.offsets, True, unique=unique, seg_read=batch.seg_read, n_reads=batch.n)
        _WHOLE[key] = (ctx.scores(), ctx.profile_limbs().copy(), ctx.coherence().copy() if coherence else None)
        ctx.close(); dix.close()
    return _WHOLE[key]


def _assert_same_run(ctx, whole):
    (off, tax, sc), limbs, _ = whole
    o2, t2, s2 = ctx.scores()
    assert np.array_equal(off, o2) and np.array_equal(tax, t2) and np.array_equal(sc.view(np.uint32), s2.view(np.uint32))
    assert np.array_equal(limbs, ctx.profile_limbs())


@pytest.mark.parametrize("n_parts,slots", [(1, 2), (2, 2), (3, 2), (7, 2), (3, 1)])
def test_paged_golden_index(n_parts, slots):
    d, ix = helpers.load_case("pairs")
    batch = reads.parse_reads(os.path.join(d, "reads.fastq"))
    whole = _whole("pairs", ix, batch, 12, 7, 3, coherence=True)
    parts, cuts = partition.split_index(ix, n_parts)
    ex = partition.PagedExchange(parts, cuts, 12, 7, 3, slots=slots)
    _assert_same_run(ex.run_batch(batch), whole)
    visited = len(ex.loaded)
    assert visited == n_parts                                           # (the golden reads reach every partition)
    s = ex.pager.stats()
    assert s["loads"] == visited and s["hits"] == 0
    coh = ex.coherence()
    assert np.array_equal(coh.view(np.uint32), whole[2].view(np.uint32))
    # a second batch: partitions that still sit in a slot are not copied again
    ex.owner.profile_reset()
    _assert_same_run(ex.run_batch(batch), whole)
    s2 = ex.pager.stats()
    if n_parts <= slots:
        assert s2["loads"] == visited and s2["hits"] == 2 * visited     # (the coherence sweep and the second batch: all hits)
    else:
        assert s2["loads"] > visited and s2["loads"] + s2["hits"] == 3 * visited
    ex.close()


@pytest.mark.parametrize("setting", ["six", "unique", "wide", "halved"])
def test_paged_settings(setting):
    kh, kl, frames, unique, stem, halved = {"six": (12, 7, 6, False, "idx", False), "unique": (12, 7, 3, True, "idx", False),
                                            "wide": (25, 7, 3, False, "idx25", False), "halved": (12, 7, 3, False, "idx_half", True)}[setting]
    d, ix = helpers.load_case("pairs", stem)
    batch = reads.parse_reads(os.path.join(d, "reads_dup.fastq" if unique else "reads.fastq"))
    whole = _whole(setting, ix, batch, kh, kl, frames, unique=unique)
    parts, cuts = partition.split_index(ix, 3)
    ex = partition.PagedExchange(parts, cuts, kh, kl, frames, halved=halved)
    assert ex.pager.record_bytes == (6 if halved else 20 if setting == "wide" else 12)
    _assert_same_run(ex.run_batch(batch, unique=unique), whole)
    ex.close()


def _parts_at(ix, bounds):
    """partitions of ix between the `_trie` entries `bounds` (0 .. m), as partition.split_index builds them"""
    ends = np.concatenate(([0], np.cumsum(ix.trie_count.astype(np.int64))))
    parts, cuts = [], []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        a, b = int(ends[lo]), int(ends[hi])
        parts.append(formats.Index(ix.kmer[a:b], ix.taxid[a:b], ix.tax[a:b], ix.trie_prefix[lo:hi], ix.trie_count[lo:hi], ix.content, ix.freq))
        cuts.append(0 if lo == 0 else int(ix.trie_prefix[lo]))
    return parts, np.asarray(cuts, dtype=np.uint64)


def test_a_partition_no_read_touches_is_never_loaded():
    ix, batch = synthetic_world(83, 10, 9000, 600)
    whole = _whole("synthetic 600", ix, batch, 12, 7, 3)
    # the queries' 30-bit prefixes, from a plain run's sorted k-mers; a `_trie` entry none of them has is the middle partition
    dix = capi.DeviceIndex(ix)
    ctx = capi.Context(dix, 12, 7, 3)
    ctx.upload(batch.bases, batch.offsets); ctx.encode(); ctx.sort_and_range()
    km, _ = ctx.queries()
    ctx.close(); dix.close()
    asked = np.unique(km >> np.uint64(30))
    m = ix.trie_prefix.shape[0]
    # (a slice takes the queries from its partition's first prefix up to the next partition's: none may lie in between either)
    inside = np.searchsorted(asked, ix.trie_prefix[1:].astype(np.uint64)) - np.searchsorted(asked, ix.trie_prefix[:-1].astype(np.uint64))
    lonely = [t for t in range(m // 3, 2 * m // 3) if inside[t] == 0]
    assert lonely, "every entry of the middle third is asked for: choose another world"
    t = lonely[0]
    parts, cuts = _parts_at(ix, [0, t, t + 1, m])
    ex = partition.PagedExchange(parts, cuts, 12, 7, 3)
    _assert_same_run(ex.run_batch(batch), whole)
    assert ex.loaded == [0, 2]
    s = ex.pager.stats()
    assert s["loads"] == 2 and s["hits"] == 0
    ex.close()


def test_pools_of_two_slices_are_kept():
    """Slices whose records have lists in the pool: the one worker overwrites its pool with the next slice, so the import reads
    the owner's copies (kasa_batch_pool_keep), every one in a place of its own."""
    ix, batch = synthetic_world(83, 10, 9000, 600)
    # every k-mer of the world under every one of its ten taxa: more segments than a record holds itself, so lists in the pool
    ix = formats.make_index(np.tile(ix.kmer, 10), np.repeat(ix.content.taxids[1:], ix.n), ix.content)
    whole = _whole("crowded 600", ix, batch, 12, 7, 3)
    parts, cuts = partition.split_index(ix, 4)
    ex = partition.PagedExchange(parts, cuts, 12, 7, 3)
    ctx = ex.run_batch(batch)
    _assert_same_run(ctx, whole)
    # the same sweep by hand, looking at the pools
    owner, w = ex.owner, ex.worker
    owner.profile_reset()
    owner.upload(batch.bases, batch.offsets); owner.encode(); owner.sort_and_range()
    ptr, n, kb = owner.queries_device()
    starts = owner.slice_starts(cuts)
    inbox, rw = owner.records_inbox(n * owner.rec_words), owner.rec_words
    kept, stale = [], []
    for j in range(4):
        at, nq = int(starts[j]), int(starts[j + 1] - starts[j])
        ex._bind(j)
        w.set_sorted_device(ptr + at * kb, nq)
        w.group_to(inbox + at * rw * 4)
        owner.profile_absorb(w)
        rp, nrw, pp, npw = w.records_device()
        kept.append((rp, nrw, owner.pool_keep(pp, npw), npw))
        stale.append((rp, nrw, pp, npw))
    assert sum(p[3] > 1 for p in kept) >= 2, [p[3] for p in kept]        # a pool in at least two slices
    assert len({p[2] for p in kept}) == 4 and all(k[2] != s[2] for k, s in zip(kept, stale))
    owner.records_import_device(kept)
    owner.score(True)
    _assert_same_run(owner, whole)
    ex.close()


# ------------------------------------------------------------------------------------------------ the driver
def _stats_line(stdout):
    m = re.search(r"OUT: Paged index on device \d+: (\d+) partitions, (\d+) batches, (\d+) visits, (\d+) loads, (\d+) hits, ([0-9.e+-]+) GB copied, copy ([0-9.e+-]+) s, prepare ([0-9.e+-]+) s", stdout)
    assert m, stdout
    return tuple(int(x) for x in m.groups()[:5])


@pytest.mark.parametrize("case", PAIRS, ids=[c[0] for c in PAIRS])
def test_driver_pages_the_golden_index(case, tmp_path):
    exe = hipbuild.build_host()
    stem, infile, fmt, kh, kl, frames, thr, beasts, idx, uniq = unpack(case)
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    cmd = ["timeout", "-k", "10", "120", exe, "identify", "-c", os.path.join(GOLD, "content.txt"), "-d", os.path.join(GOLD, idx), "-i", os.path.join(GOLD, infile),
           "-q", out, "-p", prof, FLAGS[fmt], "-b", str(beasts), "-k", str(kh), str(kl), "-m", "4", "-n", "1", "-t", str(tmp_path), "--page-index", "-v"]
    cmd += {6: ["--six"], 1: ["--one"]}.get(frames, []) + (["-e"] if uniq else []) + (["--coverage"] if wants_coverage(case) else [])
    cmd += ["--threshold", str(thr)] if thr else []
    n_rec = int(open(os.path.join(GOLD, idx + "_info.txt")).read().split()[0])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=150, env=dict(os.environ, KASA_INDEX_PAGE_RECORDS=str(n_rec // 5 + 1)))
    assert r.returncode == 0, r.stderr
    assert _read(out) == _read(os.path.join(GOLD, "out_" + stem))
    assert _read(prof) == _read(os.path.join(GOLD, "prof_" + stem.rsplit(".", 1)[0] + ".csv"))
    n_parts, n_batches, visits, loads, hits = _stats_line(r.stdout)
    assert n_parts >= 5 and n_batches >= 1 and visits <= n_parts * n_batches
    assert loads + hits == visits and (loads < visits) == (hits > 0)


def test_driver_pages_with_coherence(tmp_path):
    exe = hipbuild.build_host()
    stem, infile, fmt, kh, kl, frames, beasts, idx = COH[0]
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    cmd = ["timeout", "-k", "10", "120", exe, "identify", "-c", os.path.join(GOLD, "content.txt"), "-d", os.path.join(GOLD, idx), "-i", os.path.join(GOLD, infile),
           "-q", out, "-p", prof, FLAGS[fmt], "-b", str(beasts), "-k", str(kh), str(kl), "-m", "4", "-n", "1", "--coherence", "--page-index", "-v"]
    n_rec = int(open(os.path.join(GOLD, idx + "_info.txt")).read().split()[0])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=150, env=dict(os.environ, KASA_INDEX_PAGE_RECORDS=str(n_rec // 5 + 1)))
    assert r.returncode == 0, r.stderr
    assert _read(out) == _read(os.path.join(GOLD, "out_" + stem))
    assert _read(prof) == _read(os.path.join(GOLD, "prof_" + stem.rsplit(".", 1)[0] + ".csv"))
    n_parts, n_batches, visits, loads, hits = _stats_line(r.stdout)
    assert n_parts >= 5 and visits % 2 == 0 and n_batches < visits <= 2 * n_parts * n_batches   # the second sweep visits the same partitions


def test_driver_pages_across_batches_and_pieces(tmp_path):
    """the reference's batches and a sequence read in pieces (tests/golden/batches: m1 and long), the index in pages of 30000"""
    exe = hipbuild.build_host()
    src, d = os.path.join(helpers.GOLDEN, "batches"), str(tmp_path)
    for f in ("content.txt.gz", "idx_f.txt.gz"):
        with gzip.open(os.path.join(src, f), "rb") as g, open(os.path.join(d, f[:-3]), "wb") as o:
            shutil.copyfileobj(g, o)
    for f in ("idx", "idx_info.txt", "idx_trie", "idx_trie.txt", "reads.fastq.gz"):
        shutil.copy(os.path.join(src, f), os.path.join(d, f))
    with lzma.open(os.path.join(src, "long.fasta.xz"), "rb") as g, open(os.path.join(d, "long.fasta"), "wb") as o:
        shutil.copyfileobj(g, o)
    for infile, gold in (("reads.fastq.gz", "m1"), ("long.fasta", "long")):
        out, prof = os.path.join(d, "out.jsonl"), os.path.join(d, "prof.csv")
        cmd = ["timeout", "-k", "10", "300", exe, "identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-i", os.path.join(d, infile), "-q", out, "-p", prof,
               "--jsonl", "-b", "100", "-m", "1", "-n", "1", "-v", "--page-index"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=330, env=dict(os.environ, KASA_INDEX_PAGE_RECORDS="30000"))
        assert r.returncode == 0, r.stderr
        n_parts, n_batches, visits, loads, hits = _stats_line(r.stdout)
        assert n_parts >= 3 and n_batches >= 2 and loads + hits == visits
        with gzip.open(os.path.join(src, "out_%s.jsonl.gz" % gold), "rb") as f:
            assert _read(out) == f.read().decode("latin-1")
        assert _read(prof) == _read(os.path.join(src, "prof_%s.csv" % gold))
