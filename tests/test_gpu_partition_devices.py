"""`kasa_identify --partition-devices a,b,...`: the index in range partitions, every partition ONCE on the device of its slot,
every slot also an owner of batches; and the library calls that carry it (kasa_batch_match_depth_stage +
kasa_batch_coherence_fold, kasa_profile_absorb between any two contexts, kasa_device_copy).

A device may be named twice (`0,0` = two slots on device 0): that is how one card runs all of it -- every crossing is a copy
there too, only from the device to itself.  The cases over `0,1` need two devices and are skipped on one card.
Every comparison is byte identity with files the reference binary wrote (tests/golden/pairs, tests/golden/batches)."""
import functools
import gzip
import lzma
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from kasa_amd import build as hipbuild, capi, partition, reads
from tests import helpers
from tests.test_coherence import COH
from tests.test_gpu_coherence_partitions import END, _device_bytes, _ints, _owner_of
from tests.test_oracle_golden import PAIRS, WIDE, _read, unpack, wants_coverage

pytestmark = pytest.mark.gpu

D = os.path.join(helpers.GOLDEN, "pairs")
FLAGS = {"json": "--json", "jsonl": "--jsonl", "tsv": "--tsv", "kraken": "--kraken"}
SLOT_LISTS = ["0,0", "0,1"]


def _need(slots):
    devices = {int(x) for x in slots.split(",")}
    have = capi.device_count()
    assert have > 0
    if max(devices) >= have:
        pytest.skip("--partition-devices %s needs %d devices, %d visible" % (slots, max(devices) + 1, have))


def _host(args, part_records=None, mode="identify"):
    exe = hipbuild.build_host()
    env = {k: v for k, v in os.environ.items() if k != "KASA_INDEX_PART_RECORDS"}
    if part_records is not None:
        env["KASA_INDEX_PART_RECORDS"] = str(part_records)
    r = subprocess.run([exe, mode] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    return r


def _placement(stdout):
    """(partitions, slots, the slot list) of the verbose line; the number of partitions is its seventh token, as in the line of
    the index that lives whole on every device."""
    lines = [l for l in stdout.splitlines() if l.startswith("OUT: Index of ")]
    assert len(lines) == 1, stdout
    m = re.fullmatch(r"OUT: Index of (\d+) records in (\d+) partitions over (\d+) device slots \(([0-9,]+)\)", lines[0])
    assert m, lines[0]
    assert int(lines[0].split()[6]) == int(m.group(2))
    return int(m.group(2)), int(m.group(3)), m.group(4)


def _batches_per_owner(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("OUT: Batches per owner:")]
    assert len(lines) == 1, stdout
    return [int(x) for x in lines[0].split(":", 2)[2].split()]


@functools.lru_cache(maxsize=None)
def _records(idx):
    return int(open(os.path.join(D, idx + "_info.txt")).read().split()[0])


def _pair_args(case, out, prof, tmp):
    stem, infile, fmt, kh, kl, frames, thr, beasts, idx, uniq = unpack(case)
    a = ["-c", os.path.join(D, "content.txt"), "-d", os.path.join(D, idx), "-i", os.path.join(D, infile), "-q", out, "-p", prof, FLAGS[fmt],
         "-b", str(beasts), "-k", str(kh), str(kl), "-m", "4", "-n", "1", "-t", str(tmp), "-v"]
    a += (["--six"] if frames == 6 else []) + (["--one"] if frames == 1 else []) + (["-e"] if uniq else [])
    a += (["--coverage"] if wants_coverage(case) else []) + (["--threshold", str(thr)] if thr else [])
    return a


def _pair(stem):
    return next(c for c in PAIRS if c[0] == stem)


# ---- 1 (and 9 over two devices): the cut forced by the environment, two slots -------------------------------------------
@pytest.mark.parametrize("slots", SLOT_LISTS)
@pytest.mark.parametrize("stem", ["b100.jsonl", "six.jsonl", "unique.jsonl", "cov.jsonl"])   # three frames, --six, -e, --coverage
def test_five_partitions_in_uneven_runs_on_two_slots(stem, slots, tmp_path):
    _need(slots)
    case = _pair(stem)
    idx = unpack(case)[8]
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    r = _host(_pair_args(case, out, prof, tmp_path) + ["--partition-devices", slots], _records(idx) // 5 + 1)
    n_parts, n_slots, listed = _placement(r.stdout)
    assert n_parts >= 5 and n_slots == 2 and listed == slots
    assert _read(out) == _read(os.path.join(D, "out_" + stem))
    assert _read(prof) == _read(os.path.join(D, "prof_" + stem.rsplit(".", 1)[0] + ".csv"))


# ---- 2: no cut by the environment: the slots alone force it -------------------------------------------------------------
def test_three_slots_cut_an_index_that_fits_into_three(tmp_path):
    case = _pair("b100.jsonl")
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    r = _host(_pair_args(case, out, prof, tmp_path) + ["--partition-devices", "0,0,0"])
    assert _placement(r.stdout) == (3, 3, "0,0,0")
    assert sum(_batches_per_owner(r.stdout)) == 1
    assert _read(out) == _read(os.path.join(D, "out_b100.jsonl"))
    assert _read(prof) == _read(os.path.join(D, "prof_b100.csv"))


# ---- 3: the 128-bit index (64-byte records) -----------------------------------------------------------------------------
def test_wide_index_over_two_slots(tmp_path):
    stem, kh, kl, frames = next(w for w in WIDE if (w[1], w[2], w[3]) == (25, 7, 3))
    d, ix = helpers.load_case("pairs", "idx25")
    batch = reads.parse_reads(os.path.join(d, "reads.fastq"))
    res, nq = helpers.oracle_identify(ix, batch, kh, kl, frames, closed_form=True)
    text, ptext = helpers.render(ix, batch, helpers.csr_from_dense(res.M), res.count_all, res.count_unique, nq, "jsonl", kh, kl, frames, 0.0, 100)
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    r = _host(["-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx25"), "-i", os.path.join(d, "reads.fastq"), "-q", out, "-p", prof,
               "--jsonl", "-b", "100", "-n", "1", "-k", "25", "7", "-v", "--partition-devices", "0,0"])
    assert _placement(r.stdout) == (2, 2, "0,0")
    assert _read(out) == text
    assert _read(prof) == ptext


# ---- 4 (and 9): --coherence, --filter with --coherenceThreshold ---------------------------------------------------------
@pytest.mark.parametrize("slots", SLOT_LISTS)
@pytest.mark.parametrize("stem", ["coh.jsonl", "coh_dup6.tsv"])
def test_coherence_over_two_slots(stem, slots, tmp_path):
    _need(slots)
    _, infile, fmt, kh, kl, frames, beasts, idx = next(c for c in COH if c[0] == stem)
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    args = ["-c", os.path.join(D, "content.txt"), "-n", "1", "-v", "-d", os.path.join(D, idx), "-i", os.path.join(D, infile), "-q", out, "-p", prof,
            FLAGS[fmt], "-b", str(beasts), "-k", str(kh), str(kl), "-m", "4", "--coherence"] + {6: ["--six"], 1: ["--one"]}.get(frames, [])
    r = _host(args + ["--partition-devices", slots], _records(idx) // 5 + 1)
    n_parts, n_slots, _ = _placement(r.stdout)
    assert n_parts >= 5 and n_slots == 2
    assert _read(out) == _read(os.path.join(D, "out_" + stem))
    assert _read(prof) == _read(os.path.join(D, "prof_" + stem.rsplit(".", 1)[0] + ".csv"))


@pytest.mark.parametrize("slots", SLOT_LISTS)
def test_filter_with_coherence_threshold_over_two_slots(slots, tmp_path):
    _need(slots)
    c, x = str(tmp_path / "c"), str(tmp_path / "x")
    r = _host(["-c", os.path.join(D, "content.txt"), "-n", "1", "-v", "-d", os.path.join(D, "idx"), "-i", os.path.join(D, "reads.fastq"), "--jsonl", "-b", "100",
               "--coherence", "--coherenceThreshold", "11.99", "--errorThreshold", "0.46", "--filter", c, x, "-p", str(tmp_path / "p2"),
               "--partition-devices", slots], _records("idx") // 5 + 1)
    assert _placement(r.stdout)[0] >= 5
    assert _read(c + ".fastq", True) == _read(os.path.join(D, "cflt_clean.fastq"), True)
    assert _read(x + ".fastq", True) == _read(os.path.join(D, "cflt_cont.fastq"), True)


@pytest.mark.parametrize("n_parts", [2, 3, 7])
@pytest.mark.parametrize("idx,kh", [("idx", 12), ("idx25", 25)])
def test_depth_stage_and_fold_equal_the_depth_against_the_whole_index(idx, kh, n_parts):
    """kasa_batch_match_depth_stage on every partition's context + kasa_batch_coherence_fold on the owner leave the bytes that
    kasa_batch_match_depth_device over the whole index leaves, and the walk over them gives the unpartitioned scores."""
    d, ix = helpers.load_case("pairs", idx)
    batch = reads.parse_reads(os.path.join(d, "reads.fastq"))
    dix = capi.DeviceIndex(ix)
    ctx = capi.Context(dix, kh, 7, 3)
    parts, cuts = partition.split_index(ix, n_parts)
    pdix = [capi.DeviceIndex(p) for p in parts]
    pctx = [capi.Context(x, kh, 7, 3) for x in pdix]
    ends = [int(c) for c in cuts[1:]] + [END]
    try:
        ctx.run_batch(batch.bases, batch.offsets, True)
        with pytest.raises(RuntimeError, match="kasa_batch_coherence_fold: no kasa_batch_coherence_begin on this batch"):
            ctx.coherence_fold(0, 0)
        ptr, n, dp = ctx.coherence_begin()
        assert n == ctx.n_kmers and n > 16
        buf = capi.DeviceBuffer(n)
        buf.write(np.zeros(n, dtype=np.uint8))
        ctx.match_depth_device(0, END, ptr, n, buf.ptr)
        whole = buf.read()
        km = _device_bytes(ptr, n * ix.kmer.dtype.itemsize).view(ix.kmer.dtype)
        own = _owner_of(_ints(km), cuts, ix.K)
        assert len(np.unique(own[whole > 0])) >= 2                          # more than one partition has something to say
        with pytest.raises(RuntimeError, match="kasa_batch_match_depth_stage: n = %d, the batch these k-mers belong to has %d" % (n - 1, n)):
            pctx[0].match_depth_stage(0, END, ptr, n - 1)
        with pytest.raises(RuntimeError, match="kasa_batch_coherence_fold: n = %d, the batch has %d" % (n - 1, n)):
            ctx.coherence_fold(buf.ptr, n - 1)
        for j, c in enumerate(pctx):
            theirs = c.match_depth_stage(int(cuts[j]), ends[j], ptr, n)
            assert theirs not in (0, dp, ptr)                               # bytes of the partition's own
            assert np.array_equal(_device_bytes(theirs, n), np.where(own == j, whole, 0).astype(np.uint8))
            ctx.coherence_fold(theirs, n)
        assert np.array_equal(_device_bytes(dp, n), whole)
        # a second fold of the same bytes changes nothing (a maximum), and an empty range gives zeros
        ctx.coherence_fold(pctx[0].match_depth_stage(int(cuts[0]), ends[0], ptr, n), n)
        ctx.coherence_fold(pctx[0].match_depth_stage(5, 5, ptr, n), n)
        assert np.array_equal(_device_bytes(dp, n), whole)
        buf.close()
        got = ctx.coherence_finish()
        assert np.array_equal(got.view(np.uint32), ctx.coherence().view(np.uint32))
        assert (got > 0).any()
    finally:
        for c in pctx:
            c.close()
        for x in pdix:
            x.close()
        ctx.close(); dix.close()


# ---- 5: several batches, a sequence in pieces; both owners take batches, their profiles are summed at the end of the file
def test_batches_and_pieces_are_shared_by_both_owners(tmp_path):
    src = os.path.join(helpers.GOLDEN, "batches")
    d = str(tmp_path)
    for f in ("content.txt.gz", "idx_f.txt.gz"):
        with gzip.open(os.path.join(src, f), "rb") as g, open(os.path.join(d, f[:-3]), "wb") as o:
            shutil.copyfileobj(g, o)
    for f in ("idx", "idx_info.txt", "idx_trie", "idx_trie.txt", "reads.fastq.gz"):
        shutil.copy(os.path.join(src, f), os.path.join(d, f))
    with lzma.open(os.path.join(src, "long.fasta.xz"), "rb") as g, open(os.path.join(d, "long.fasta"), "wb") as o:
        shutil.copyfileobj(g, o)
    for infile, gold in (("reads.fastq.gz", "m1"), ("long.fasta", "long")):
        out, prof = os.path.join(d, "out.jsonl"), os.path.join(d, "prof.csv")
        r = _host(["-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-i", os.path.join(d, infile), "-q", out, "-p", prof,
                   "--jsonl", "-b", "100", "-m", "1", "-n", "1", "-v", "--partition-devices", "0,0"], 30000)
        n_parts, n_slots, _ = _placement(r.stdout)
        assert n_parts >= 2 and n_slots == 2
        per_owner = _batches_per_owner(r.stdout)
        assert len(per_owner) == 2 and min(per_owner) >= 1, per_owner
        assert sum(per_owner) == sum(1 for l in r.stdout.splitlines() if l.startswith("OUT: Batch of "))
        with gzip.open(os.path.join(src, "out_%s.jsonl.gz" % gold), "rb") as f:
            assert _read(out) == f.read().decode("latin-1")
        assert _read(prof) == _read(os.path.join(src, "prof_%s.csv" % gold))


# ---- 6: identify_multiple ------------------------------------------------------------------------------------------------
def test_identify_multiple_over_two_slots(tmp_path):
    ind = tmp_path / "in"
    ind.mkdir()
    cases = {"sampleA.fastq": ("reads.fastq", "b100"), "sampleB.fasta": ("reads.fasta", "fasta"), "sampleC.fastq": ("reads_dup.fastq", "dup"),
             "sampleD.fasta": ("exampleInput.fasta", "exampleInput")}
    for f, (orig, _) in cases.items():
        shutil.copy(os.path.join(D, orig), str(ind / f))
    r = _host(["-c", os.path.join(D, "content.txt"), "-d", os.path.join(D, "idx"), "-i", str(ind) + "/", "-q", str(tmp_path / "rtt_"), "-p", str(tmp_path / "prof_"),
               "--jsonl", "-b", "100", "-n", "2", "-v", "--partition-devices", "0,0"], _records("idx") // 5 + 1, mode="identify_multiple")
    assert _placement(r.stdout)[1] == 2
    for f, (_, stem) in cases.items():
        name = f.rsplit(".", 1)[0]
        assert _read(str(tmp_path / ("rtt_" + name + ".jsonl"))) == _read(os.path.join(D, "out_" + stem + ".jsonl")), f
        assert _read(str(tmp_path / ("prof_" + name + ".csv"))) == _read(os.path.join(D, "prof_" + stem + ".csv")), f


# ---- 7: slices without a query -------------------------------------------------------------------------------------------
def test_one_short_read_leaves_most_partitions_an_empty_slice(tmp_path):
    """The first 45 bases of one read: a few dozen k-mers (counted by the oracle's encoder), fewer than the 40 and more
    partitions, so some partitions get a slice without a query, and so does the owner's import.  The files are those of the
    same command without partitions."""
    fq = open(os.path.join(D, "reads.fastq")).read().split("\n")
    one = str(tmp_path / "one.fastq")
    open(one, "w").write("\n".join([fq[0], fq[1][:45], fq[2], fq[3][:45]]) + "\n")
    batch = reads.parse_reads(one)
    from oracle import oracle
    n_parts = 40
    km, _ = oracle.encode(batch.bases, batch.offsets, oracle.params(12, 7, 3))
    assert batch.n == 1 and 0 < len(km) < n_parts
    got = {}
    for name, extra, part in (("whole", [], None), ("spread", ["--partition-devices", "0,0"], _records("idx") // n_parts + 1)):
        out, prof = str(tmp_path / (name + ".jsonl")), str(tmp_path / (name + ".csv"))
        r = _host(["-c", os.path.join(D, "content.txt"), "-d", os.path.join(D, "idx"), "-i", one, "-q", out, "-p", prof, "--jsonl", "-b", "100", "-n", "1", "-v",
                   "--coherence"] + extra, part)
        got[name] = (_read(out), _read(prof))
        if extra:
            assert _placement(r.stdout)[0] >= n_parts
            assert "OUT: Number of k-mers in input: %d " % len(km) in r.stdout
    assert got["spread"] == got["whole"]
    assert '"Coherence"' in got["whole"][0] and '"tax ID"' in got["whole"][0]          # the read still finds its taxon


# ---- 8: kasa_profile_absorb between two contexts that both ran batches ---------------------------------------------------
def _limb_ints(limbs):
    """Per cell (unique, total, the 128-bit sum of count_all) as Python integers."""
    return [(int(u), int(t), sum(int(x) << (32 * i) for i, x in enumerate(a))) for u, t, *a in limbs.tolist()]


def test_profile_absorb_adds_the_tables_of_another_owner():
    d, ix = helpers.load_case("pairs")
    dix = capi.DeviceIndex(ix)
    a, b = capi.Context(dix, 12, 7, 3), capi.Context(dix, 12, 7, 3)
    try:
        first = reads.parse_reads(os.path.join(d, "reads.fastq"))
        second = reads.parse_reads(os.path.join(d, "reads_dup.fastq"))
        a.run_batch(first.bases, first.offsets, True)
        b.run_batch(second.bases, second.offsets, False)
        la, lb = _limb_ints(a.profile_limbs()), _limb_ints(b.profile_limbs())
        (_, cua, cta), (_, cub, ctb) = a.profile(), b.profile()
        assert cua.any() and cub.any() and not np.array_equal(cua, cub)
        a.profile_absorb(b)
        want = [tuple(x + y for x, y in zip(p, q)) for p, q in zip(la, lb)]
        assert _limb_ints(a.profile_limbs()) == want                       # count_all: the exact 128-bit sums, limb by limb
        ca, cu, ct = a.profile()
        assert np.array_equal(cu, cua + cub) and np.array_equal(ct, cta + ctb)
        assert np.array_equal(ca.reshape(-1), np.asarray([float(v[2] >> 64) + float(v[2] & (2 ** 64 - 1)) * 2.0 ** -64 for v in want]))   # (as kasa_profile_fetch rounds)
        assert not b.profile_limbs().any()                                 # the source is empty afterwards
        a.profile_absorb(b)                                                # ... and absorbing nothing changes nothing
        assert _limb_ints(a.profile_limbs()) == want
    finally:
        a.close(); b.close(); dix.close()
