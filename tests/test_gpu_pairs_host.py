"""`kasa_identify -1 <file> -2 <file> --device-pairs` against the files the reference binary wrote and against the same driver
without the flag: both files are parsed into pools on the device, paired there (kasa_pair_*), the bytes are the same; what the
device leaves to the host (a chunk it does not take, --filter, --coherence, two device slots) gives the same bytes too and
says so under -v.  (There is no reference file for pairs with --filter: that run is held against the driver's own host path,
--partition-devices against both; pairs with --coherence end with the driver's own error on either path.)"""
import os

import numpy as np
import pytest

from tests.test_gpu_device_inflate_host import _bgzf
from tests.test_gpu_device_parse_host import PAIRS_DIR, _run
from tests.test_oracle_golden import _read

pytestmark = pytest.mark.gpu

HOST_LINE = "OUT: --device-pairs: the host parser"
P1, P2 = os.path.join(PAIRS_DIR, "pair_1.fastq"), os.path.join(PAIRS_DIR, "pair_2.fastq")
MISMATCH = "The paired-end files hold different numbers of reads"


def _identify(f1, f2, out, prof, extra, flag=("--device-pairs",)):
    return ["identify", "-c", os.path.join(PAIRS_DIR, "content.txt"), "-d", os.path.join(PAIRS_DIR, "idx"), "-1", f1, "-2", f2, "-q", out, "-p", prof, "-v",
            "--jsonl", "-b", "100"] + list(flag) + extra


def _golden(stem):
    return _read(os.path.join(PAIRS_DIR, "out_" + stem + ".jsonl")), _read(os.path.join(PAIRS_DIR, "prof_" + stem + ".csv"))


@pytest.mark.parametrize("stem,extra", [("pair", []), ("pair6", ["--six"])], ids=["pair", "pair6"])
@pytest.mark.parametrize("block", [None, "600"], ids=["one-chunk", "chunks"])
def test_golden_pairs(stem, extra, block, tmp_path):
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    r = _run(_identify(P1, P2, out, prof, extra), env={"KASA_READ_BLOCK": block} if block else None)
    assert HOST_LINE not in r.stdout and "--device-parse: the host parser" not in r.stdout, r.stdout
    assert (_read(out), _read(prof)) == _golden(stem)


@pytest.mark.parametrize("stem,extra", [("pair", []), ("pair6", ["--six"])], ids=["pair", "pair6"])
@pytest.mark.parametrize("which", ["both", "first", "second"])
def test_golden_pairs_as_bgzf(stem, extra, which, tmp_path):
    """--device-inflate: each file in the form it has -- both BGZF, or one BGZF and the other plain FASTQ"""
    f1 = _bgzf(P1, str(tmp_path / "p1.gz"), block=499) if which in ("both", "first") else P1
    f2 = _bgzf(P2, str(tmp_path / "p2.gz"), block=499) if which in ("both", "second") else P2
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    r = _run(_identify(f1, f2, out, prof, extra + ["--device-inflate"]), env={"KASA_READ_BLOCK": "600", "KASA_HOST_TIMING": "1"})
    assert HOST_LINE not in r.stdout, r.stdout
    assert ("--device-inflate: the host path is used for file" in r.stdout) == (which != "both")
    assert (_read(out), _read(prof)) == _golden(stem)


def _synthetic_pairs(tmp_path, n=2000, tab_at=None, empty_line_at=None, drop_last_of_2=False):
    """n pairs cut out of the golden database's genomes: mate 1 of 100 letters, mate 2 of 200 (the pools drift apart)"""
    records = open(os.path.join(PAIRS_DIR, "db.fasta")).read().split(">")[1:]
    g = "".join(records[0].split("\n")[1:]).encode()          # the first genome, its lines joined
    assert len(g) > 1000
    rng = np.random.default_rng(99)
    r1, r2 = [], []
    for r in range(n):
        p, q = (int(x) for x in rng.integers(0, len(g) - 200, 2))
        a, b = g[p:p + 100], g[q:q + 200]
        if tab_at == r:
            b = b[:70] + b"\t" + b[71:]
        r1.append(b"@s%d/1\n%s\n+\n%s\n" % (r, a, b"I" * len(a)))
        r2.append((b"\n" if empty_line_at == r else b"") + b"@s%d/2\n%s\n+\n%s\n" % (r, b, b"I" * len(b)))
    if drop_last_of_2:
        r2.pop()
    f1, f2 = tmp_path / "s_1.fastq", tmp_path / "s_2.fastq"
    f1.write_bytes(b"".join(r1))
    f2.write_bytes(b"".join(r2))
    return str(f1), str(f2)


ENV = {"KASA_READ_BLOCK": "1500", "KASA_MAX_BATCH_KMERS": "75000"}


def _both_ways(tmp_path, f1, f2, rc=0):
    runs = []
    for flag in ((), ("--device-pairs",)):
        out, prof = str(tmp_path / ("out" + str(len(flag)))), str(tmp_path / ("prof" + str(len(flag))))
        r = _run(_identify(f1, f2, out, prof, ["-n", "2"], flag), env=ENV, rc=rc)
        runs.append((r, _read(out) if rc == 0 else None, _read(prof) if rc == 0 else None))
    return runs


def test_pools_that_drift_and_a_dozen_batches(tmp_path):
    f1, f2 = _synthetic_pairs(tmp_path)
    (host, out0, prof0), (dev, out1, prof1) = _both_ways(tmp_path, f1, f2)
    assert HOST_LINE not in dev.stdout, dev.stdout[-2000:]
    batches = [l for l in dev.stdout.splitlines() if l.startswith("OUT: Batch of ")]
    assert len(batches) >= 10 and batches == [l for l in host.stdout.splitlines() if l.startswith("OUT: Batch of ")]
    assert out1 == out0 and prof1 == prof0 and out0.count("\n") == 2000


def test_a_tab_in_a_read_of_file_2(tmp_path):
    """some dozen chunks in: exit 1 and the reference's message either way; the device hands over first"""
    f1, f2 = _synthetic_pairs(tmp_path, n=300, tab_at=200)
    (host, _, _), (dev, _, _) = _both_ways(tmp_path, f1, f2, rc=1)
    for r in (host, dev):
        assert "ERROR: Spaces or tabs inside read, please check your input." in r.stderr
    assert HOST_LINE + " takes over from byte" in dev.stdout and " of file 2 (a space or tab in a sequence line)" in dev.stdout
    assert HOST_LINE not in host.stdout


def test_a_record_the_host_tolerates_and_the_device_refuses(tmp_path):
    """an empty line before a FASTQ record of file 2: the host parser takes over and the bytes are the host path's"""
    f1, f2 = _synthetic_pairs(tmp_path, n=600, empty_line_at=400)
    (host, out0, prof0), (dev, out1, prof1) = _both_ways(tmp_path, f1, f2)
    assert HOST_LINE + " takes over from byte" in dev.stdout and " of file 2 (" in dev.stdout
    assert out1 == out0 and prof1 == prof0 and out0.count("\n") == 600


def test_file_2_one_record_short(tmp_path):
    f1, f2 = _synthetic_pairs(tmp_path, n=300, drop_last_of_2=True)
    (host, _, _), (dev, _, _) = _both_ways(tmp_path, f1, f2, rc=1)
    assert MISMATCH in host.stderr and MISMATCH in dev.stderr


@pytest.mark.parametrize("why,extra", [("--filter", None), ("more than one device slot", ["--partition-devices", "0,0"])], ids=["filter", "partition-0,0"])
def test_what_stays_with_the_host_parser(why, extra, tmp_path):
    got = []
    for flag in ((), ("--device-pairs",)):
        tag = str(len(flag))
        out, prof = str(tmp_path / ("out" + tag)), str(tmp_path / ("prof" + tag))
        more = ["--filter", str(tmp_path / ("c" + tag)), str(tmp_path / ("x" + tag))] if extra is None else extra
        r = _run(_identify(P1, P2, out, prof, more, flag))
        assert (HOST_LINE + " is used (" + why in r.stdout) == bool(flag), r.stdout
        files = [_read(out), _read(prof)]
        if extra is None:
            files += [open(os.path.join(tmp_path, f), "rb").read() for f in sorted(os.listdir(tmp_path)) if f.startswith(("c" + tag, "x" + tag))]
            assert len(files) > 2
        got.append(files)
    assert got[0] == got[1]
    if why == "more than one device slot":
        assert tuple(got[1]) == _golden("pair")


def test_coherence_stays_with_the_host_parser(tmp_path):
    """The driver scores no pairs with --coherence (kasa_batch_coherence refuses them): with the flag the run says that the
    host parser is used and ends as it does without.  Single-end input under --device-pairs is --device-parse's case and
    gives the reference's bytes."""
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    ends = []
    for flag in ((), ("--device-pairs",)):
        r = _run(_identify(P1, P2, out, prof, ["--coherence", "-m", "4", "-n", "1"], flag), rc=1)
        assert (HOST_LINE + " is used (--coherence)" in r.stdout) == bool(flag), r.stdout
        ends.append(r.stderr)
    assert ends[0] == ends[1] and "paired-end input is not supported" in ends[0]
    r = _run(["identify", "-c", os.path.join(PAIRS_DIR, "content.txt"), "-d", os.path.join(PAIRS_DIR, "idx"), "-i", os.path.join(PAIRS_DIR, "reads.fastq"), "-q", out, "-p", prof,
              "-v", "--jsonl", "-b", "100", "--device-pairs", "--coherence", "-m", "4", "-n", "1"])
    assert "OUT: --device-parse: the host parser is used (--coherence)" in r.stdout
    assert _read(out) == _read(os.path.join(PAIRS_DIR, "out_coh.jsonl")) and _read(prof) == _read(os.path.join(PAIRS_DIR, "prof_coh.csv"))


def test_single_end_input_is_device_parse(tmp_path):
    """--device-pairs implies --device-parse: one file goes through the one pool"""
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    r = _run(["identify", "-c", os.path.join(PAIRS_DIR, "content.txt"), "-d", os.path.join(PAIRS_DIR, "idx"), "-i", os.path.join(PAIRS_DIR, "reads.fastq"), "-q", out, "-p", prof,
              "-v", "--jsonl", "-b", "100", "--device-pairs"], env={"KASA_READ_BLOCK": "1500", "KASA_HOST_TIMING": "1"})
    assert "the host parser" not in r.stdout and "device-parse" in r.stdout
    assert _read(out) == _read(os.path.join(PAIRS_DIR, "out_b100.jsonl")) and _read(prof) == _read(os.path.join(PAIRS_DIR, "prof_b100.csv"))


@pytest.mark.parametrize("block", [None, "600"], ids=["one-chunk", "chunks"])
def test_pair_dump_device_equals_pair_dump(block, tmp_path):
    env = {"KASA_READ_BLOCK": block} if block else {}
    host = _run(["pair-dump", P1, P2, "2"], env=env).stdout.split("\n", 2)[2]       # (the driver's two banner lines come first)
    dev = _run(["pair-dump-device", P1, P2, "2"], env=env).stdout.split("\n", 2)[2]
    assert dev == host and host.count("\n") == 13
