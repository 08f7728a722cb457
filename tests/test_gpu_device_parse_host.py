"""`kasa_identify ... --device-parse` against the files the reference binary wrote: the input's text is parsed on the device
(kasa_parse_*), the batches are the reference's, the bytes are the same; the combinations the device parser leaves to the host
(a chunk it does not take, paired-end, --filter, --coherence, two device slots) give the same bytes too and say so under -v."""
import gzip
import lzma
import os
import shutil
import subprocess

import pytest

from kasa_amd import build as hipbuild, capi
from tests import helpers
from tests.test_oracle_golden import PAIRS, _read, unpack

pytestmark = pytest.mark.gpu

FLAGS = {"json": "--json", "jsonl": "--jsonl", "tsv": "--tsv", "kraken": "--kraken"}
PAIRS_DIR = os.path.join(helpers.GOLDEN, "pairs")
BATCHES = os.path.join(helpers.GOLDEN, "batches")
HOST_LINE = "OUT: --device-parse: the host parser"         # what -v prints when the host parser is used after all


def _run(args, env=None, rc=0):
    assert capi.device_count() > 0, "no HIP device visible"
    exe = hipbuild.build_host()
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert r.returncode == rc, r.stderr[-2000:]
    return r


def _identify(infile, out, prof, extra, index="idx", d=PAIRS_DIR):
    return ["identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, index), "-i", infile, "-q", out, "-p", prof, "-v", "--device-parse"] + extra


ONE_OF_EACH = [next(c for c in PAIRS if unpack(c)[2] == fmt and unpack(c)[1] == "reads.fastq") for fmt in ("tsv", "json", "jsonl", "kraken")]


@pytest.mark.parametrize("case", ONE_OF_EACH + [c for c in PAIRS if c[0] in ("fasta.jsonl", "edge_crlf.jsonl", "edge_multi.jsonl", "edge_noeol.jsonl")],
                         ids=lambda c: c[0])
def test_golden_pairs(case, tmp_path):
    stem, infile, fmt, kh, kl, frames, thr, beasts, idx, uniq = unpack(case)
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    r = _run(_identify(os.path.join(PAIRS_DIR, infile), out, prof, [FLAGS[fmt], "-b", str(beasts), "-k", str(kh), str(kl), "-m", "4", "-n", "1"], idx))
    assert HOST_LINE not in r.stdout, r.stdout
    assert _read(out) == _read(os.path.join(PAIRS_DIR, "out_" + stem))
    assert _read(prof) == _read(os.path.join(PAIRS_DIR, "prof_" + stem.rsplit(".", 1)[0] + ".csv"))


@pytest.mark.parametrize("stage", ["pinned", "pageable"])
def test_gzipped_input_in_dozens_of_chunks(stage, tmp_path):
    raw = open(os.path.join(PAIRS_DIR, "reads.fastq"), "rb").read()
    gz = str(tmp_path / "reads.fastq.gz")
    with open(gz, "wb") as f:
        f.write(gzip.compress(raw))
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    r = _run(_identify(gz, out, prof, ["--jsonl", "-b", "100", "-n", "3"]), env={"KASA_READ_BLOCK": "1500", "KASA_PARSE_STAGE": stage, "KASA_HOST_TIMING": "1"})
    assert HOST_LINE not in r.stdout
    assert "upload-text" in r.stdout and "device-parse" in r.stdout
    assert _read(out) == _read(os.path.join(PAIRS_DIR, "out_b100.jsonl"))
    assert _read(prof) == _read(os.path.join(PAIRS_DIR, "prof_b100.csv"))


@pytest.fixture(scope="module")
def batches_case(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dp_batches"))
    for f in ("content.txt.gz", "idx_f.txt.gz"):
        with gzip.open(os.path.join(BATCHES, f), "rb") as g, open(os.path.join(d, f[:-3]), "wb") as o:
            shutil.copyfileobj(g, o)
    for f in ("idx", "idx_info.txt", "idx_trie", "idx_trie.txt", "reads.fastq.gz"):
        shutil.copy(os.path.join(BATCHES, f), os.path.join(d, f))
    with lzma.open(os.path.join(BATCHES, "long.fasta.xz"), "rb") as g, open(os.path.join(d, "long.fasta"), "wb") as o:
        shutil.copyfileobj(g, o)
    return d


def _gz_text(name):
    with gzip.open(os.path.join(BATCHES, name), "rb") as f:
        return f.read().decode("latin-1")


def test_the_reference_batches(batches_case, tmp_path):
    """-m 1 cuts this input into several batches: the takes out of the pool follow the reference's boundaries."""
    import json
    d = batches_case
    out, prof = str(tmp_path / "out.jsonl"), str(tmp_path / "prof.csv")
    r = _run(_identify(os.path.join(d, "reads.fastq.gz"), out, prof, ["--jsonl", "-b", "100", "-m", "1", "-n", "1"], d=d), env={"KASA_READ_BLOCK": "200000"})
    assert HOST_LINE not in r.stdout
    sizes = [int(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("OUT: Batch of ")]
    assert sizes == json.load(open(os.path.join(BATCHES, "batches.json")))["m1"]
    assert _read(out) == _gz_text("out_m1.jsonl.gz")
    assert _read(prof) == _read(os.path.join(BATCHES, "prof_m1.csv"))


def test_a_sequence_read_in_pieces_falls_back(batches_case, tmp_path):
    import json
    d = batches_case
    out, prof = str(tmp_path / "out.jsonl"), str(tmp_path / "prof.csv")
    r = _run(_identify(os.path.join(d, "long.fasta"), out, prof, ["--jsonl", "-b", "100", "-m", "1", "-n", "1"], d=d), env={"KASA_READ_BLOCK": "100000"})
    assert "OUT: --device-parse: the host parser takes over from byte" in r.stdout and "read in pieces" in r.stdout, r.stdout
    sizes = [int(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("OUT: Batch of ")]
    assert sizes == json.load(open(os.path.join(BATCHES, "long.json")))["long"]["batches"]
    assert _read(out) == _gz_text("out_long.jsonl.gz")
    assert _read(prof) == _read(os.path.join(BATCHES, "prof_long.csv"))


def test_paired_end_filter_and_coherence_use_the_host_parser(tmp_path):
    d = PAIRS_DIR
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    base = ["identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-p", prof, "-v", "--device-parse", "--jsonl", "-b", "100"]
    r = _run(base + ["-1", os.path.join(d, "pair_1.fastq"), "-2", os.path.join(d, "pair_2.fastq"), "-q", out])
    assert HOST_LINE + " is used (paired-end input)" in r.stdout
    assert _read(out) == _read(os.path.join(d, "out_pair.jsonl")) and _read(prof) == _read(os.path.join(d, "prof_pair.csv"))
    c, x = str(tmp_path / "c"), str(tmp_path / "x")
    r = _run(base + ["-i", os.path.join(d, "reads.fastq"), "--filter", c, x])
    assert HOST_LINE + " is used (--filter" in r.stdout
    assert _read(c + ".fastq", True) == _read(os.path.join(d, "flt_clean.fastq"), True)
    assert _read(x + ".fastq", True) == _read(os.path.join(d, "flt_cont.fastq"), True)
    r = _run(base + ["-i", os.path.join(d, "reads.fastq"), "-q", out, "--coherence", "-m", "4", "-n", "1"])
    assert HOST_LINE + " is used (--coherence)" in r.stdout
    assert _read(out) == _read(os.path.join(d, "out_coh.jsonl")) and _read(prof) == _read(os.path.join(d, "prof_coh.csv"))


@pytest.mark.parametrize("slots", [["--partition-devices", "0,0"], ["--devices", "0,1"]], ids=["partition-0,0", "devices-0,1"])
def test_more_than_one_device_slot_uses_the_host_parser(slots, tmp_path):
    """The pool serves one slot only, so the host parser feeds a run over several.  --partition-devices 0,0 is two slots on
    the one device (copies only); --devices makes a communicator, which wants two devices."""
    if slots[0] == "--devices" and capi.device_count() < 2:
        pytest.skip("--devices 0,1 needs 2 devices")
    d = PAIRS_DIR
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    r = _run(_identify(os.path.join(d, "reads.fastq"), out, prof, ["--jsonl", "-b", "100"] + slots))
    assert HOST_LINE + " is used (more than one device slot)" in r.stdout
    assert _read(out) == _read(os.path.join(d, "out_b100.jsonl")) and _read(prof) == _read(os.path.join(d, "prof_b100.csv"))


@pytest.mark.parametrize("name", ["reads.fastq", "reads.fasta", "edge_crlf.fasta", "edge_multi.fastq", "edge_noeol.fasta", "exampleInput.fasta", "reads_prot.fasta"])
@pytest.mark.parametrize("block", [None, "1500"])
def test_parse_dump_device_equals_parse_dump(name, block, tmp_path):
    path = os.path.join(PAIRS_DIR, name)
    env = {"KASA_READ_BLOCK": block} if block else {}
    host = _run(["parse-dump", path, "2"], env=env).stdout.split("== streamed\n")[1]
    dev = _run(["parse-dump-device", path, "2"], env=env).stdout
    assert dev.split("\n", 2)[2] == host and len(host) > 100     # (the driver's two banner lines come first)


def test_a_tab_in_a_read_ends_with_the_reference_message(tmp_path):
    raw = open(os.path.join(PAIRS_DIR, "reads.fastq"), "rb").read().split(b"\n")
    raw[4 * 20 + 1] = raw[4 * 20 + 1][:50] + b"\t" + raw[4 * 20 + 1][51:]
    bad = tmp_path / "tab.fastq"
    bad.write_bytes(b"\n".join(raw))
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    for extra in ([], ["--device-parse"]):
        r = _run(["identify", "-c", os.path.join(PAIRS_DIR, "content.txt"), "-d", os.path.join(PAIRS_DIR, "idx"), "-i", str(bad), "-q", out, "-p", prof, "--jsonl", "-v"] + extra,
                 env={"KASA_READ_BLOCK": "1500"}, rc=1)
        assert "ERROR: Spaces or tabs inside read, please check your input." in r.stderr
        if extra:
            assert "the host parser takes over" in r.stdout and "space or tab" in r.stdout
