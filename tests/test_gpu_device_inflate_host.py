"""`kasa_identify ... --device-inflate` on BGZF forms of the golden inputs: the file goes up compressed, is inflated and
parsed on the device (kasa_bgzf_parse_append), the batches are the reference's and the bytes are the golden files'; input
that is not BGZF and the combinations the device path leaves to the host give the same bytes and say so under -v; a corrupt
member ends the run."""
import gzip
import json
import os

import pytest

from tests import inflate_corpus as corpus
from tests.test_gpu_device_parse_host import BATCHES, FLAGS, ONE_OF_EACH, PAIRS_DIR, _gz_text, _run, batches_case  # noqa: F401
from tests.test_oracle_golden import PAIRS, _read, unpack

pytestmark = pytest.mark.gpu

HOST_LINE = "OUT: --device-inflate: the host path is used"
PARSE_HOST_LINE = "OUT: --device-parse: the host parser"


def _bgzf(src, dst, block=997, eof=True):
    data = open(src, "rb").read()
    with open(dst, "wb") as f:
        f.write(corpus.stream(data, block=block, level=6) + (corpus.formats.BGZF_EOF if eof else b""))
    return dst


def _identify(infile, out, prof, extra, index="idx", d=PAIRS_DIR):
    return ["identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, index), "-i", infile, "-q", out, "-p", prof, "-v", "--device-inflate"] + extra


@pytest.mark.parametrize("case", ONE_OF_EACH + [c for c in PAIRS if c[0] in ("fasta.jsonl", "edge_crlf.jsonl", "edge_multi.jsonl", "edge_noeol.jsonl")],
                         ids=lambda c: c[0])
def test_golden_pairs(case, tmp_path):
    stem, infile, fmt, kh, kl, frames, thr, beasts, idx, uniq = unpack(case)
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    gz = _bgzf(os.path.join(PAIRS_DIR, infile), str(tmp_path / (infile + ".gz")))
    r = _run(_identify(gz, out, prof, [FLAGS[fmt], "-b", str(beasts), "-k", str(kh), str(kl), "-m", "4", "-n", "1"], idx),
             env={"KASA_READ_BLOCK": "1500", "KASA_HOST_TIMING": "1"})
    assert HOST_LINE not in r.stdout and PARSE_HOST_LINE not in r.stdout, r.stdout
    assert " inflate " in [l for l in r.stdout.splitlines() if l.startswith("OUT: host timing")][0]
    assert _read(out) == _read(os.path.join(PAIRS_DIR, "out_" + stem))
    assert _read(prof) == _read(os.path.join(PAIRS_DIR, "prof_" + stem.rsplit(".", 1)[0] + ".csv"))


def test_the_reference_batches(batches_case, tmp_path):
    d = batches_case
    raw = str(tmp_path / "reads.fastq")
    with gzip.open(os.path.join(d, "reads.fastq.gz"), "rb") as g, open(raw, "wb") as o:
        o.write(g.read())
    gz = _bgzf(raw, str(tmp_path / "reads.bgzf.gz"), block=65280)
    out, prof = str(tmp_path / "out.jsonl"), str(tmp_path / "prof.csv")
    r = _run(_identify(gz, out, prof, ["--jsonl", "-b", "100", "-m", "1", "-n", "1"], d=d), env={"KASA_READ_BLOCK": "200000"})
    assert HOST_LINE not in r.stdout and PARSE_HOST_LINE not in r.stdout
    sizes = [int(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("OUT: Batch of ")]
    assert sizes == json.load(open(os.path.join(BATCHES, "batches.json")))["m1"]
    assert _read(out) == _gz_text("out_m1.jsonl.gz")
    assert _read(prof) == _read(os.path.join(BATCHES, "prof_m1.csv"))


def test_plain_gzip_takes_the_host_path(tmp_path):
    raw = open(os.path.join(PAIRS_DIR, "reads.fastq"), "rb").read()
    gz = str(tmp_path / "reads.fastq.gz")
    with open(gz, "wb") as f:
        f.write(gzip.compress(raw))
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    r = _run(_identify(gz, out, prof, ["--jsonl", "-b", "100", "-n", "3"]), env={"KASA_READ_BLOCK": "1500"})
    assert HOST_LINE + " (gzip without a BC subfield" in r.stdout
    assert _read(out) == _read(os.path.join(PAIRS_DIR, "out_b100.jsonl")) and _read(prof) == _read(os.path.join(PAIRS_DIR, "prof_b100.csv"))
    r = _run(_identify(os.path.join(PAIRS_DIR, "reads.fastq"), out, prof, ["--jsonl", "-b", "100", "-n", "3"]))
    assert HOST_LINE + " (the input is not gzip)" in r.stdout
    assert _read(out) == _read(os.path.join(PAIRS_DIR, "out_b100.jsonl")) and _read(prof) == _read(os.path.join(PAIRS_DIR, "prof_b100.csv"))


def test_paired_end_filter_and_coherence_take_the_host_path(tmp_path):
    d = PAIRS_DIR
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    gz = {n: _bgzf(os.path.join(d, n), str(tmp_path / (n + ".gz"))) for n in ("reads.fastq", "pair_1.fastq", "pair_2.fastq")}
    base = ["identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-p", prof, "-v", "--device-inflate", "--jsonl", "-b", "100"]
    r = _run(base + ["-1", gz["pair_1.fastq"], "-2", gz["pair_2.fastq"], "-q", out])
    assert HOST_LINE + " (paired-end input)" in r.stdout
    assert _read(out) == _read(os.path.join(d, "out_pair.jsonl")) and _read(prof) == _read(os.path.join(d, "prof_pair.csv"))
    c, x = str(tmp_path / "c"), str(tmp_path / "x")
    r = _run(base + ["-i", gz["reads.fastq"], "--filter", c, x])
    assert HOST_LINE + " (--filter" in r.stdout
    assert _read(c + ".fastq", True) == _read(os.path.join(d, "flt_clean.fastq"), True)
    assert _read(x + ".fastq", True) == _read(os.path.join(d, "flt_cont.fastq"), True)
    r = _run(base + ["-i", gz["reads.fastq"], "-q", out, "--coherence", "-m", "4", "-n", "1"])
    assert HOST_LINE + " (--coherence)" in r.stdout
    assert _read(out) == _read(os.path.join(d, "out_coh.jsonl")) and _read(prof) == _read(os.path.join(d, "prof_coh.csv"))


def test_a_sequence_read_in_pieces_falls_back_into_the_gz(batches_case, tmp_path):
    """the host parser goes on inside the .gz: the reader seeks to the span that holds the first unparsed byte"""
    d = batches_case
    gz = _bgzf(os.path.join(d, "long.fasta"), str(tmp_path / "long.fasta.gz"), block=65280)
    out, prof = str(tmp_path / "out.jsonl"), str(tmp_path / "prof.csv")
    r = _run(_identify(gz, out, prof, ["--jsonl", "-b", "100", "-m", "1", "-n", "1"], d=d), env={"KASA_READ_BLOCK": "100000"})
    assert "OUT: --device-parse: the host parser takes over from byte" in r.stdout and "read in pieces" in r.stdout, r.stdout
    assert HOST_LINE not in r.stdout
    sizes = [int(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("OUT: Batch of ")]
    assert sizes == json.load(open(os.path.join(BATCHES, "long.json")))["long"]["batches"]
    assert _read(out) == _gz_text("out_long.jsonl.gz")
    assert _read(prof) == _read(os.path.join(BATCHES, "prof_long.csv"))


def test_a_corrupt_member_ends_the_run(tmp_path):
    data = open(os.path.join(PAIRS_DIR, "reads.fastq"), "rb").read()
    ms = corpus.members(data, block=997, level=6)
    k = 11
    ms[k] = corpus.edit_member(ms[k], crc=int.from_bytes(ms[k][-8:-4], "little") ^ 0x100)
    gz = str(tmp_path / "bad.fastq.gz")
    with open(gz, "wb") as f:
        f.write(b"".join(ms) + corpus.formats.BGZF_EOF)
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    r = _run(_identify(gz, out, prof, ["--jsonl", "-b", "100"]), env={"KASA_READ_BLOCK": "1500"}, rc=1)
    assert "ERROR: a CRC-32 mismatch in BGZF member %d" % k in r.stderr, r.stderr
