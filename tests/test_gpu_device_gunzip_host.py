"""`kasa_identify ... --device-gunzip` on plain gzip forms of the golden inputs: the file goes up compressed span by span, is
inflated (kasa_gzip_parse_append: chunks, confirmed block chain, resolved windows) and parsed on the device, the batches are
the reference's and the bytes are the golden files'.  KASA_READ_BLOCK=1500 makes the stream cross many spans, so blocks are
cut by span ends and the stream's state (bit position, window, CRC) is carried; the `flushed` form has a block every 700 bytes
of text, gzip.compress writes one block for these inputs, which no span of 1500 bytes holds.  BGZF input with the same flag
goes member by member, the combinations the device path leaves to the host say so under -v and give the same bytes, and a
corrupt stream ends the run."""
import gzip
import json
import os
import zlib

import pytest

from tests import gzip_corpus, inflate_corpus
from tests.test_gpu_device_parse_host import BATCHES, FLAGS, ONE_OF_EACH, PAIRS_DIR, _gz_text, _run, batches_case  # noqa: F401
from tests.test_oracle_golden import PAIRS, _read, unpack

pytestmark = pytest.mark.gpu

GUNZIP_LINE = "OUT: --device-gunzip: the stream is inflated on the device"
HOST_LINE = "OUT: --device-gunzip: the host path is used"
INFLATE_HOST_LINE = "OUT: --device-inflate: the host path is used"
PARSE_HOST_LINE = "OUT: --device-parse: the host parser"


def _plain(src, dst, form="gzip"):
    data = open(src, "rb").read()
    if form == "gzip":
        gz = gzip.compress(data, 6)
    else:
        payload, _ = gzip_corpus.flushed(data, 700, zlib.Z_SYNC_FLUSH)
        gz = gzip_corpus.member(data, payload)
    assert gzip.decompress(gz) == data
    with open(dst, "wb") as f:
        f.write(gz)
    return dst


def _bgzf(src, dst, block=997):
    with open(dst, "wb") as f:
        f.write(inflate_corpus.stream(open(src, "rb").read(), block=block, level=6) + inflate_corpus.formats.BGZF_EOF)
    return dst


def _identify(infile, out, prof, extra, index="idx", d=PAIRS_DIR):
    return ["identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, index), "-i", infile, "-q", out, "-p", prof, "-v", "--device-gunzip"] + extra


def _stats(stdout):
    line = [l for l in stdout.splitlines() if l.startswith("OUT: --device-gunzip: chunks ")]
    assert len(line) == 1, stdout
    w = line[0].replace(",", "").split()
    assert w[2:9:2] == ["chunks", "confirmed", "rejected", "rounds"], line
    return dict(chunks=int(w[3]), confirmed=int(w[5]), rejected=int(w[7]), rounds=int(w[9]))


@pytest.mark.parametrize("form", ["gzip", "flushed"])
@pytest.mark.parametrize("case", ONE_OF_EACH + [c for c in PAIRS if c[0] in ("fasta.jsonl", "edge_crlf.jsonl", "edge_multi.jsonl", "edge_noeol.jsonl")],
                         ids=lambda c: c[0])
def test_golden_pairs(case, form, tmp_path):
    stem, infile, fmt, kh, kl, frames, thr, beasts, idx, uniq = unpack(case)
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    gz = _plain(os.path.join(PAIRS_DIR, infile), str(tmp_path / (infile + ".gz")), form)
    r = _run(_identify(gz, out, prof, [FLAGS[fmt], "-b", str(beasts), "-k", str(kh), str(kl), "-m", "4", "-n", "1"], idx),
             env={"KASA_READ_BLOCK": "1500", "KASA_HOST_TIMING": "1"})
    assert GUNZIP_LINE in r.stdout and HOST_LINE not in r.stdout and INFLATE_HOST_LINE not in r.stdout and PARSE_HOST_LINE not in r.stdout, r.stdout
    assert " inflate " in [l for l in r.stdout.splitlines() if l.startswith("OUT: host timing")][0]
    st = _stats(r.stdout)
    assert st["confirmed"] >= 1 and st["chunks"] >= st["confirmed"] and st["rejected"] == 0 and st["rounds"] == 1
    assert _read(out) == _read(os.path.join(PAIRS_DIR, "out_" + stem))
    assert _read(prof) == _read(os.path.join(PAIRS_DIR, "prof_" + stem.rsplit(".", 1)[0] + ".csv"))


def test_the_reference_batches(batches_case, tmp_path):
    d = batches_case
    out, prof = str(tmp_path / "out.jsonl"), str(tmp_path / "prof.csv")
    # (the case's own reads.fastq.gz is a plain gzip file)
    r = _run(_identify(os.path.join(d, "reads.fastq.gz"), out, prof, ["--jsonl", "-b", "100", "-m", "1", "-n", "1"], d=d), env={"KASA_READ_BLOCK": "200000"})
    assert GUNZIP_LINE in r.stdout and HOST_LINE not in r.stdout and INFLATE_HOST_LINE not in r.stdout and PARSE_HOST_LINE not in r.stdout
    sizes = [int(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("OUT: Batch of ")]
    assert sizes == json.load(open(os.path.join(BATCHES, "batches.json")))["m1"]
    assert _read(out) == _gz_text("out_m1.jsonl.gz")
    assert _read(prof) == _read(os.path.join(BATCHES, "prof_m1.csv"))


def test_small_chunks_in_the_driver(tmp_path):
    """KASA_GUNZIP_CHUNK=256: dozens of chunks a span, markers across chunk starts and across spans"""
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    gz = _plain(os.path.join(PAIRS_DIR, "reads.fastq"), str(tmp_path / "reads.fastq.gz"), "flushed")
    r = _run(_identify(gz, out, prof, ["--jsonl", "-b", "100", "-n", "3"]), env={"KASA_READ_BLOCK": "1500", "KASA_GUNZIP_CHUNK": "256"})
    st = _stats(r.stdout)
    assert st["confirmed"] > 5 and st["chunks"] > st["confirmed"]
    assert _read(out) == _read(os.path.join(PAIRS_DIR, "out_b100.jsonl")) and _read(prof) == _read(os.path.join(PAIRS_DIR, "prof_b100.csv"))


def test_bgzf_takes_the_member_path_and_text_the_parser(tmp_path):
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    gz = _bgzf(os.path.join(PAIRS_DIR, "reads.fastq"), str(tmp_path / "reads.bgzf.gz"))
    r = _run(_identify(gz, out, prof, ["--jsonl", "-b", "100", "-n", "3"]), env={"KASA_READ_BLOCK": "1500"})
    assert "OUT: --device-gunzip" not in r.stdout and INFLATE_HOST_LINE not in r.stdout and PARSE_HOST_LINE not in r.stdout, r.stdout
    assert _read(out) == _read(os.path.join(PAIRS_DIR, "out_b100.jsonl")) and _read(prof) == _read(os.path.join(PAIRS_DIR, "prof_b100.csv"))
    r = _run(_identify(os.path.join(PAIRS_DIR, "reads.fastq"), out, prof, ["--jsonl", "-b", "100", "-n", "3"]))
    assert INFLATE_HOST_LINE + " (the input is not gzip)" in r.stdout and "OUT: --device-gunzip" not in r.stdout and PARSE_HOST_LINE not in r.stdout
    assert _read(out) == _read(os.path.join(PAIRS_DIR, "out_b100.jsonl")) and _read(prof) == _read(os.path.join(PAIRS_DIR, "prof_b100.csv"))


def test_paired_end_filter_and_coherence_take_the_host_path(tmp_path):
    d = PAIRS_DIR
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    gz = {n: _plain(os.path.join(d, n), str(tmp_path / (n + ".gz"))) for n in ("reads.fastq", "pair_1.fastq", "pair_2.fastq")}
    base = ["identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-p", prof, "-v", "--device-gunzip", "--jsonl", "-b", "100"]
    r = _run(base + ["-1", gz["pair_1.fastq"], "-2", gz["pair_2.fastq"], "-q", out])
    assert HOST_LINE + " (paired-end input)" in r.stdout and GUNZIP_LINE not in r.stdout
    assert _read(out) == _read(os.path.join(d, "out_pair.jsonl")) and _read(prof) == _read(os.path.join(d, "prof_pair.csv"))
    c, x = str(tmp_path / "c"), str(tmp_path / "x")
    r = _run(base + ["-i", gz["reads.fastq"], "--filter", c, x])
    assert HOST_LINE + " (--filter" in r.stdout and GUNZIP_LINE not in r.stdout
    assert _read(c + ".fastq", True) == _read(os.path.join(d, "flt_clean.fastq"), True)
    assert _read(x + ".fastq", True) == _read(os.path.join(d, "flt_cont.fastq"), True)
    r = _run(base + ["-i", gz["reads.fastq"], "-q", out, "--coherence", "-m", "4", "-n", "1"])
    assert HOST_LINE + " (--coherence)" in r.stdout and GUNZIP_LINE not in r.stdout
    assert _read(out) == _read(os.path.join(d, "out_coh.jsonl")) and _read(prof) == _read(os.path.join(d, "prof_coh.csv"))


def test_device_pairs_one_mate_plain_gzip_one_bgzf(tmp_path):
    d = PAIRS_DIR
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    one = _plain(os.path.join(d, "pair_1.fastq"), str(tmp_path / "pair_1.fastq.gz"), "flushed")
    two = _bgzf(os.path.join(d, "pair_2.fastq"), str(tmp_path / "pair_2.fastq.gz"))
    r = _run(["identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-p", prof, "-v", "--device-gunzip", "--device-pairs", "--jsonl", "-b", "100",
              "-1", one, "-2", two, "-q", out], env={"KASA_READ_BLOCK": "1500"})
    assert "OUT: --device-gunzip: the stream of file 1 is inflated on the device" in r.stdout and "file 2 is inflated" not in r.stdout
    assert HOST_LINE not in r.stdout and INFLATE_HOST_LINE not in r.stdout and "the host parser" not in r.stdout, r.stdout
    assert _read(out) == _read(os.path.join(d, "out_pair.jsonl")) and _read(prof) == _read(os.path.join(d, "prof_pair.csv"))


def test_a_sequence_read_in_pieces_falls_back_into_the_gz(batches_case, tmp_path):
    """the host parser goes on inside the .gz: one long stream is read again from its first byte, the parsed text dropped"""
    d = batches_case
    gz = _plain(os.path.join(d, "long.fasta"), str(tmp_path / "long.fasta.gz"))
    out, prof = str(tmp_path / "out.jsonl"), str(tmp_path / "prof.csv")
    r = _run(_identify(gz, out, prof, ["--jsonl", "-b", "100", "-m", "1", "-n", "1"], d=d), env={"KASA_READ_BLOCK": "100000"})
    assert "OUT: --device-parse: the host parser takes over from byte" in r.stdout and "read in pieces" in r.stdout, r.stdout
    assert GUNZIP_LINE in r.stdout and HOST_LINE not in r.stdout
    sizes = [int(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("OUT: Batch of ")]
    assert sizes == json.load(open(os.path.join(BATCHES, "long.json")))["long"]["batches"]
    assert _read(out) == _gz_text("out_long.jsonl.gz")
    assert _read(prof) == _read(os.path.join(BATCHES, "prof_long.csv"))


def test_a_corrupt_stream_ends_the_run(tmp_path):
    gz = bytearray(gzip.compress(open(os.path.join(PAIRS_DIR, "reads.fastq"), "rb").read(), 6))
    gz[-6] ^= 1                                                        # the trailer's CRC-32
    path = str(tmp_path / "bad.fastq.gz")
    with open(path, "wb") as f:
        f.write(bytes(gz))
    out, prof = str(tmp_path / "out"), str(tmp_path / "prof.csv")
    r = _run(_identify(path, out, prof, ["--jsonl", "-b", "100"]), env={"KASA_READ_BLOCK": "1500"}, rc=1)
    assert "ERROR: a CRC-32 mismatch in gzip member 0" in r.stderr, r.stderr


def test_parse_dump_device_takes_a_plain_gz(tmp_path):
    from kasa_amd import build as hipbuild
    import subprocess
    exe = hipbuild.build_host()
    src = os.path.join(PAIRS_DIR, "reads.fastq")
    gz = _plain(src, str(tmp_path / "reads.fastq.gz"), "flushed")
    env = dict(os.environ, KASA_READ_BLOCK="1500")
    want = subprocess.run([exe, "parse-dump-device", src, "2"], stdout=subprocess.PIPE, check=True, env=env).stdout
    got = subprocess.run([exe, "parse-dump-device", gz, "2", "--device-gunzip"], stdout=subprocess.PIPE, check=True, env=env).stdout
    got, want = got[got.index(b"protein="):], want[want.index(b"protein="):]    # (behind the line that repeats the command)
    assert got == want and len(got) > 5000
