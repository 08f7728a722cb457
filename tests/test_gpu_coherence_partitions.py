"""--coherence over a range-partitioned index (kasa_batch_coherence_begin / _match_depth_device / _finish,
partition.LocalExchange.coherence, kasa_identify with KASA_INDEX_PART_RECORDS).

A k-mer's match length needs at least the 6 letters of a `_trie` entry in common with an index entry, and partitions are
cut between `_trie` entries: its depth against the whole index is its depth against the partition that owns its 30-bit
prefix and 0 against every other one.  The first test states that on the CPU; the others compare the partitioned device
run with the oracle and with the unpartitioned run.  Every comparison is bit equality."""
import bisect
import functools
import os
import subprocess

import numpy as np
import pytest

from kasa_amd import capi, formats, partition, reads
from oracle import oracle
from tests import helpers
from tests.test_coherence import COH, FLAGS, _device_coherence, _oracle_run
from tests.test_oracle_golden import _read

END = 1 << (5 * formats.TRIE_LETTERS)                       # one past the last 30-bit prefix
PAIRS = os.path.join(helpers.GOLDEN, "pairs")


# ------------------------------------------------------------------------------------------------ the premise, on the CPU
def _ints(km):
    """k-mers as Python integers (a 128-bit key has no numpy integer)."""
    if formats.is_wide(km):
        return [(int(h) << 64) | int(l) for l, h in zip(km["lo"].tolist(), km["hi"].tolist())]
    return [int(x) for x in km.tolist()]


def _depth(q, idx, K, kh, kl):
    """The depth step in plain words: letters in common with the two neighbours of the k-mer's place in the sorted index
    (searchsorted, here bisect over integers); at least 6, at most kHigh, cut before the first '^' (letter 30), 0 below kLow."""
    out = np.zeros(len(q), dtype=np.uint8)
    for i, k in enumerate(q):
        lo = bisect.bisect_left(idx, k)
        L = 0
        for nb in (lo, lo - 1):
            if 0 <= nb < len(idx):
                x = k ^ idx[nb]
                L = max(L, K if x == 0 else K - (x.bit_length() + 4) // 5)
        d = 0
        if L >= formats.TRIE_LETTERS:
            d = L = min(L, kh)
            for kk in range(kl, L + 1):
                if (k >> (5 * (K - kk))) & 31 == 30:
                    d = kk - 1
                    break
            if d < kl:
                d = 0
        out[i] = d
    return out


def _owner_of(q, cuts, K):
    pre = np.asarray([k >> (5 * (K - formats.TRIE_LETTERS)) for k in q], dtype=np.uint64)
    return np.searchsorted(np.asarray(cuts, dtype=np.uint64), pre, side="right") - 1


@pytest.mark.parametrize("n_parts", [2, 3, 7])
@pytest.mark.parametrize("idx,kh", [("idx", 12), ("idx25", 25)])
def test_depth_against_the_whole_index_is_the_depth_against_the_owning_partition(idx, kh, n_parts):
    d, ix = helpers.load_case("pairs", idx)
    batch = reads.parse_reads(os.path.join(d, "reads.fastq"))
    km, _ = oracle.encode(batch.bases, batch.offsets, oracle.params(kh, 7, 3, K=ix.K))
    q = _ints(km)
    whole = _depth(q, _ints(ix.kmer), ix.K, kh, 7)
    parts, cuts = partition.split_index(ix, n_parts)
    assert sum(p.n for p in parts) == ix.n and all(p.n > 0 for p in parts)
    own = _owner_of(q, cuts, ix.K)
    assert own.min() >= 0 and own.max() < n_parts
    for j, p in enumerate(parts):
        dj = _depth(q, _ints(p.kmer), ix.K, kh, 7)
        assert np.array_equal(dj[own == j], whole[own == j])
        assert not dj[own != j].any()
    assert len(np.unique(own[whole > 0])) >= 2              # more than one partition has something to say


# ------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _golden(stem):
    """(index, batch, the oracle's coherence or the exception it ends with) of a COH case: computed once."""
    case = next(c for c in COH if c[0] == stem)
    _, infile, _, kh, kl, frames, _, idx = case
    d, ix = helpers.load_case("pairs", idx)
    batch = reads.parse_reads(os.path.join(d, infile))
    _, _, coh, ml = _oracle_run(ix, batch, kh, kl, frames, True)
    coh.setflags(write=False); ml.setflags(write=False)
    return ix, batch, coh, ml


def _exchange(ix, n_parts, kh, kl, frames, resident, protein=False):
    parts, cuts = partition.split_index(ix, n_parts)
    ex = partition.LocalExchange(parts, cuts, kh, kl, frames, device_resident=resident)
    ex.owner.set_protein(protein)
    return ex


def _partitioned(ix, batch, kh, kl, frames, n_parts, resident):
    ex = _exchange(ix, n_parts, kh, kl, frames, resident, bool(batch.protein))
    try:
        ex.run_batch(batch)
        return ex.coherence()
    finally:
        ex.close()


@pytest.mark.gpu
@pytest.mark.parametrize("resident", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n_parts", [2, 3, 7])
@pytest.mark.parametrize("case", COH, ids=[c[0] for c in COH])
def test_partitioned_coherence_equals_the_oracle(case, n_parts, resident):
    stem, infile, fmt, kh, kl, frames, beasts, idx = case
    ix, batch, coh, _ = _golden(stem)
    got = _partitioned(ix, batch, kh, kl, frames, n_parts, resident)
    assert got.dtype == np.float32 and got.shape == (batch.n,)
    assert np.array_equal(got.view(np.uint32), coh.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _wide():
    d, ix = helpers.load_case("pairs", "idx25")
    batch = reads.parse_reads(os.path.join(d, "reads.fastq"))
    whole = _device_coherence(ix, batch, 25, 7, 3)
    whole.setflags(write=False)
    return ix, batch, whole


@pytest.mark.gpu
@pytest.mark.parametrize("resident", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n_parts", [2, 3, 7])
def test_partitioned_coherence_wide_index_equals_the_unpartitioned_run(n_parts, resident):
    ix, batch, whole = _wide()
    got = _partitioned(ix, batch, 25, 7, 3, n_parts, resident)
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))
    assert (whole > 0).any() and len(np.unique(whole)) > 2


def _quirky_world(frames, seed):
    """The generator of tests/test_coherence.py::test_device_coherence_many_chunks_and_quirks: many chunks of the parallel
    walk, runs of reads without k-mers, foreign reads, reads matching on one strand only, a last read matching on both."""
    from tests.test_gpu_parity import synthetic_world
    rng = np.random.default_rng(9200 + seed)
    ix, base = synthetic_world(300 + seed, 6, 6000, 1500)
    comp = np.zeros(256, dtype=np.uint8); comp[[65, 67, 71, 84]] = [84, 71, 67, 65]
    parts = []
    for r in range(base.n):
        s = base.bases[base.offsets[r]:base.offsets[r + 1]]
        u = rng.random()
        if u < 0.08:
            s = s[:int(rng.integers(1, 22))]                            # no k-mers at all
        elif u < 0.20:
            s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=150)]   # foreign
        elif u < 0.30:
            s = s[:int(rng.integers(23, 60))]
        parts.append(s)
    last = base.bases[base.offsets[0]:base.offsets[1]][:75]
    parts.append(np.concatenate((last, comp[last[::-1]])))               # matches on both strands
    return ix, _batch_of(parts)


def _batch_of(seqs):
    off = np.concatenate(([0], np.cumsum([len(x) for x in seqs]))).astype(np.int64)
    bases = np.concatenate(seqs) if seqs else np.zeros(0, dtype=np.uint8)
    return reads.ReadBatch(bases, off, None, np.asarray([len(x) + 1 for x in seqs], dtype=np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("frames,seed", [(3, 0), (6, 1), (1, 2)])
def test_the_walks_quirks_through_partitions(frames, seed):
    ix, batch = _quirky_world(frames, seed)
    _, _, coh, _ = oracle.identify_batch_coherence(ix, batch.bases, batch.offsets, oracle.params(12, 7, frames), True)
    got = _partitioned(ix, batch, 12, 7, frames, 4, True)
    assert np.array_equal(got.view(np.uint32), coh.view(np.uint32))
    assert len(np.unique(coh)) > 5


@pytest.mark.gpu
@pytest.mark.parametrize("resident", [False, True], ids=["host", "device"])
def test_batches_without_a_match_and_without_a_kmer(resident):
    _, ix = helpers.load_case("pairs")
    ex = _exchange(ix, 3, 12, 7, 3, resident)
    try:
        nothing = _batch_of([np.full(100, ord("N"), dtype=np.uint8)] * 70)        # k-mers, none of them in the index
        ctx = ex.run_batch(nothing)
        assert ctx.n_kmers > 0
        got = ex.coherence()
        assert got.shape == (70,) and not got.view(np.uint32).any()
        short = _batch_of([np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)] * 5)     # too short for a single k-mer
        ctx = ex.run_batch(short)
        assert ctx.n_kmers == 0
        got = ex.coherence()
        assert got.shape == (5,) and not got.view(np.uint32).any()
    finally:
        ex.close()


def _most_parts(ix):
    """As many partitions as split_index cuts without leaving one empty."""
    for n in range(ix.trie_prefix.shape[0], 0, -1):
        parts, cuts = partition.split_index(ix, n)
        if all(p.n > 0 for p in parts):
            return parts, cuts
    raise AssertionError("no split")


def _sparse_world():
    """Two short reads and an index of a few dozen `_trie` entries -- those the reads' k-mers fall into and a few others --
    cut into as many partitions as split_index allows."""
    from tests.test_gpu_parity import synthetic_world
    full, base = synthetic_world(311, 6, 6000, 50)
    batch = _batch_of([base.bases[base.offsets[r]:base.offsets[r] + 48] for r in (0, 1)])
    km, _ = oracle.encode(batch.bases, batch.offsets, oracle.params(12, 7, 3))
    hit = np.isin(full.trie_prefix, formats.key_shr(km, 5 * (12 - formats.TRIE_LETTERS)).astype(np.uint32))
    rest = np.flatnonzero(~hit)
    keep_t = np.union1d(np.flatnonzero(hit), rest[::max(1, rest.shape[0] // 8)])
    keep = np.zeros(full.n, dtype=bool)
    starts = full.trie_start.astype(np.int64)
    for t in keep_t:
        keep[starts[t]:starts[t] + int(full.trie_count[t])] = True
    ix = formats.make_index(full.kmer[keep], full.taxid[keep], full.content)
    return ix, batch, km


@pytest.mark.gpu
def test_partitions_that_own_no_query():
    """Most partitions find no k-mer of theirs among the batch's and must leave every depth byte alone."""
    ix, batch, km = _sparse_world()
    parts, cuts = _most_parts(ix)
    assert len(parts) >= 8
    per_part = np.diff(partition.slice_starts(np.sort(km), cuts, 12))
    assert (per_part == 0).any() and (per_part > 0).sum() >= 2
    _, _, coh, _ = oracle.identify_batch_coherence(ix, batch.bases, batch.offsets, oracle.params(12, 7, 3), True)
    ex = partition.LocalExchange(parts, cuts, 12, 7, 3, device_resident=True)
    try:
        ex.run_batch(batch)
        got = ex.coherence()
    finally:
        ex.close()
    assert np.array_equal(got.view(np.uint32), coh.view(np.uint32))
    assert (coh > 0).any()


@pytest.mark.gpu
def test_partitions_report_where_the_reference_throws(tmp_path):
    d, ix = helpers.load_case("pairs")
    batch = reads.parse_reads(os.path.join(d, "reads.fastq"))
    want = _read(os.path.join(d, "coh_six_throws.err"))
    with pytest.raises(RuntimeError) as e:
        _partitioned(ix, batch, 12, 7, 6, 3, True)
    assert "ERROR: " + str(e.value) + "\n" == want
    r = _driver(["-d", os.path.join(d, "idx"), "-i", os.path.join(d, "reads.fastq"), "--tsv", "--six", "--coherence",
                 "-q", str(tmp_path / "o"), "-p", str(tmp_path / "p")], ix.n // 3 + 1)
    assert r.returncode == 1
    assert want.strip() in r.stderr
    assert _partitions_reported(r.stdout) >= 3


def _device_bytes(ptr, nbytes, device=0):
    out = np.empty(nbytes, dtype=np.uint8)
    if nbytes:
        capi._check(capi.lib().kasa_device_read(capi.C.c_int(device), out.ctypes.data_as(capi.C.c_void_p), capi.C.c_void_p(ptr), capi.C.c_size_t(nbytes)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("idx,kh", [("idx", 12), ("idx25", 25)])
def test_match_depth_device_alone(idx, kh):
    d, ix = helpers.load_case("pairs", idx)
    batch = reads.parse_reads(os.path.join(d, "reads.fastq"))
    dix = capi.DeviceIndex(ix)
    ctx = capi.Context(dix, kh, 7, 3)
    parts, cuts = partition.split_index(ix, 3)
    pdix = [capi.DeviceIndex(p) for p in parts]
    pctx = [capi.Context(x, kh, 7, 3) for x in pdix]
    ends = [int(c) for c in cuts[1:]] + [END]
    try:
        ctx.run_batch(batch.bases, batch.offsets, True)
        ptr, n, dp = ctx.coherence_begin()
        assert n == ctx.n_kmers and n > 0
        assert not _device_bytes(dp, n).any()                             # begin hands out zeros
        ctx.match_depth_device(0, END, ptr, n, dp)
        whole = _device_bytes(dp, n)
        if kh == 12:                                                      # (the 128-bit oracle needs the stock binary's comparator quirk)
            assert np.array_equal(whole, _golden("coh.jsonl")[3])
        km = _device_bytes(ptr, n * ix.kmer.dtype.itemsize).view(ix.kmer.dtype)
        own = _owner_of(_ints(km), cuts, ix.K)
        assert len(np.unique(own[whole > 0])) >= 2
        # one call per partition into a buffer of the caller's
        buf = capi.DeviceBuffer(n)
        buf.write(np.zeros(n, dtype=np.uint8))
        for j, c in enumerate(pctx):
            c.match_depth_device(int(cuts[j]), ends[j], ptr, n, buf.ptr)
        assert np.array_equal(buf.read(), whole)
        # a call for ONE partition changes nothing outside its range
        for j, c in enumerate(pctx):
            buf.write(np.full(n, 0xEE, dtype=np.uint8))
            c.match_depth_device(int(cuts[j]), ends[j], ptr, n, buf.ptr)
            assert np.array_equal(buf.read(), np.where(own == j, whole, 0xEE).astype(np.uint8))
        # an empty range is no work and no error
        buf.write(np.full(n, 0xEE, dtype=np.uint8))
        pctx[0].match_depth_device(5, 5, ptr, n, buf.ptr)
        assert (buf.read() == 0xEE).all()
        buf.close()
        # the owner's batch is as it was: the walk over the bytes of the whole index gives the unpartitioned scores
        got = ctx.coherence_finish()
        assert np.array_equal(got.view(np.uint32), ctx.coherence().view(np.uint32))
    finally:
        for c in pctx:
            c.close()
        for x in pdix:
            x.close()
        ctx.close(); dix.close()


def _driver(args, part_records, extra=()):
    from kasa_amd import build as hipbuild
    exe = hipbuild.build_host()
    cmd = [exe, "identify", "-c", os.path.join(PAIRS, "content.txt"), "-n", "1", "-v"] + list(args) + list(extra)
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                          env=dict(os.environ, KASA_INDEX_PART_RECORDS=str(part_records)))


def _partitions_reported(stdout):
    for line in stdout.splitlines():
        if line.startswith("OUT: Index of ") and " partitions" in line:
            return int(line.split()[6])
    return 0


@functools.lru_cache(maxsize=None)
def _records(idx):
    return helpers.load_case("pairs", idx)[1].n


@pytest.mark.gpu
@pytest.mark.parametrize("host_text", [False, True], ids=["device_text", "host_text"])
@pytest.mark.parametrize("case", COH, ids=[c[0] for c in COH])
def test_cpp_host_coherence_over_partitions_files_byte_identical(case, host_text, tmp_path):
    stem, infile, fmt, kh, kl, frames, beasts, idx = case
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    args = ["-d", os.path.join(PAIRS, idx), "-i", os.path.join(PAIRS, infile), "-q", out, "-p", prof, FLAGS[fmt], "-b", str(beasts),
            "-k", str(kh), str(kl), "-m", "4", "--coherence"] + {6: ["--six"], 1: ["--one"]}.get(frames, [])
    r = _driver(args, _records(idx) // 5 + 1, ["--host-text"] if host_text else [])
    assert r.returncode == 0, r.stderr
    assert _partitions_reported(r.stdout) >= 5
    assert _read(out) == _read(os.path.join(PAIRS, "out_" + stem))
    assert _read(prof) == _read(os.path.join(PAIRS, "prof_" + stem.rsplit(".", 1)[0] + ".csv"))


@pytest.mark.gpu
@pytest.mark.parametrize("host_text", [False, True], ids=["device_text", "host_text"])
def test_cpp_host_filter_with_coherence_over_partitions(host_text, tmp_path):
    c, x = str(tmp_path / "c"), str(tmp_path / "x")
    r = _driver(["-d", os.path.join(PAIRS, "idx"), "-i", os.path.join(PAIRS, "reads.fastq"), "--jsonl", "-b", "100", "--coherence",
                 "--coherenceThreshold", "11.99", "--errorThreshold", "0.46", "--filter", c, x, "-p", str(tmp_path / "p2")],
                _records("idx") // 5 + 1, ["--host-text"] if host_text else [])
    assert r.returncode == 0, r.stderr
    assert _partitions_reported(r.stdout) >= 5
    assert _read(c + ".fastq", True) == _read(os.path.join(PAIRS, "cflt_clean.fastq"), True)
    assert _read(x + ".fastq", True) == _read(os.path.join(PAIRS, "cflt_cont.fastq"), True)


@pytest.mark.gpu
def test_misuse_is_an_error_not_a_fault():
    d, ix = helpers.load_case("pairs")
    dix = capi.DeviceIndex(ix)
    ctx, other = capi.Context(dix, 12, 7, 3), capi.Context(dix, 12, 7, 3)
    try:
        batch = reads.parse_reads(os.path.join(d, "reads.fastq"))
        ctx.upload(batch.bases, batch.offsets)
        with pytest.raises(RuntimeError, match="kasa_batch_coherence_begin: batch not sorted"):
            ctx.coherence_begin()
        ctx.run_batch(batch.bases, batch.offsets, True)
        with pytest.raises(RuntimeError, match="kasa_batch_coherence_finish: no kasa_batch_coherence_begin on this batch"):
            ctx.coherence_finish()
        ptr, n, dp = ctx.coherence_begin()
        for c in (ctx, other):                                            # the owner itself or another context: n is the batch's
            with pytest.raises(RuntimeError, match="kasa_batch_match_depth_device: n = %d, the batch these k-mers belong to has %d" % (n - 1, n)):
                c.match_depth_device(0, END, ptr, n - 1, dp)
            with pytest.raises(RuntimeError, match="kasa_batch_match_depth_device: n = %d" % (n + 1000)):
                c.match_depth_device(0, END, ptr, n + 1000, dp)
        with pytest.raises(RuntimeError, match="is not a range of 30-bit prefixes"):
            other.match_depth_device(7, 6, ptr, n, dp)
        with pytest.raises(RuntimeError, match="is not a range of 30-bit prefixes"):
            other.match_depth_device(0, END + 1, ptr, n, dp)
        other.match_depth_device(0, END, ptr, n, dp)
        want = ctx.coherence_finish()                                     # the refused calls have left the seam usable
        assert np.array_equal(want.view(np.uint32), _golden("coh.jsonl")[2].view(np.uint32))
        with pytest.raises(RuntimeError, match="no kasa_batch_coherence_begin"):   # one finish per begin
            ctx.coherence_finish()
        ctx.coherence_begin()
        ctx.upload(batch.bases, batch.offsets)                            # a new batch ends the seam of the old one
        ctx.encode(); ctx.sort_and_range(); ctx.lookup_score(True)
        with pytest.raises(RuntimeError, match="no kasa_batch_coherence_begin"):
            ctx.coherence_finish()
        dup = reads.parse_reads(os.path.join(d, "reads_dup.fastq"))
        ctx.run_batch(dup.bases, dup.offsets, True, unique=True)
        with pytest.raises(RuntimeError, match="kasa_batch_coherence_begin: not together with -e"):
            ctx.coherence_begin()
        pairs = reads.parse_pairs(os.path.join(d, "pair_1.fastq"), os.path.join(d, "pair_2.fastq"))
        ctx.run_batch(pairs.bases, pairs.offsets, True, seg_read=pairs.seg_read, n_reads=pairs.n)
        with pytest.raises(RuntimeError, match="kasa_batch_coherence_begin: paired-end input is not supported"):
            ctx.coherence_begin()
        with pytest.raises(RuntimeError, match="no kasa_batch_coherence_begin"):
            ctx.coherence_finish()
    finally:
        other.close(); ctx.close(); dix.close()
