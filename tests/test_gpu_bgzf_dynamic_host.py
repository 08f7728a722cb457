"""`kasa_identify identify ... -q <file> --bgzf-dynamic`: decompressed, the file is byte for byte the file the same command line
writes without the flag (the golden files), it ends with BGZF's end-of-file block, and the batches the device wrote carry a
Huffman table of their own (BTYPE = 10); the flag implies --bgzf, its conditions included."""
import gzip
import json
import os

import pytest

from kasa_amd import formats
from tests.test_gpu_bgzf_host import BATCHES, PAIRS_DIR, _gz_text, _pairs, _run, _unpacked, batches_case  # noqa: F401 (batches_case: a fixture)
from tests.test_oracle_golden import _read

pytestmark = pytest.mark.gpu


def _btypes(path):
    """BTYPE of the first deflate block of every member but the EOF block"""
    z = open(path, "rb").read()
    assert z.endswith(formats.BGZF_EOF)
    return [(payload[0] >> 1) & 3 for _, payload, _, isize in formats.bgzf_members(z) if isize]


def _dynamic(args):
    return [a for a in args if a != "--bgzf"] + ["--bgzf-dynamic"]         # (the flag alone: it implies --bgzf)


def test_b100(tmp_path):
    out, prof = str(tmp_path / "out.gz"), str(tmp_path / "prof.csv")
    _run(_dynamic(_pairs("reads.fastq", out, prof, ["--jsonl", "-b", "100"])))
    assert _unpacked(out) == _read(os.path.join(PAIRS_DIR, "out_b100.jsonl"))
    assert _read(prof) == _read(os.path.join(PAIRS_DIR, "prof_b100.csv"))
    kinds = _btypes(out)
    assert kinds and 2 in kinds, kinds
    fixed = str(tmp_path / "fixed.gz")
    _run(_pairs("reads.fastq", fixed, prof, ["--jsonl", "-b", "100"]))
    assert gzip.decompress(open(fixed, "rb").read()) == gzip.decompress(open(out, "rb").read())
    assert 2 not in _btypes(fixed) and os.path.getsize(out) < os.path.getsize(fixed)


def test_three_batches_a_table_each(batches_case, tmp_path):
    d = batches_case
    out, prof = str(tmp_path / "out.gz"), str(tmp_path / "prof.csv")
    r = _run(["identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-i", os.path.join(d, "reads.fastq.gz"), "-q", out, "-p", prof,
              "--jsonl", "-b", "100", "-m", "1", "-n", "1", "-v", "--bgzf-dynamic"])
    sizes = [int(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("OUT: Batch of ")]
    assert sizes == json.load(open(os.path.join(BATCHES, "batches.json")))["m1"] and len(sizes) == 3
    assert _unpacked(out) == _gz_text("out_m1.jsonl.gz")
    assert _read(prof) == _read(os.path.join(BATCHES, "prof_m1.csv"))
    assert _btypes(out).count(2) >= 3                                   # every batch's stream begins with a block of 2048 bytes and more


def test_parameters_file_key(tmp_path):
    out, prof = str(tmp_path / "out.gz"), str(tmp_path / "prof.csv")
    y = tmp_path / "config.yaml"
    y.write_text(f"""Mode: identify
Index: "{os.path.join(PAIRS_DIR, 'idx')}"
ContentFile: {os.path.join(PAIRS_DIR, 'content.txt')}
kHigh: 12
kLow: 7
InputFileOrFolder: {os.path.join(PAIRS_DIR, 'reads.fastq')}
ProfileOutputfile: {prof}
ReadIDtoTaxIDOutputfile: {out}
ReadIDtoTaxIDOutputFormat: jsonl
NumberOfTaxaPerRead: 100
BgzfDynamic: true
""")
    _run(["--parameters", str(y)])
    assert _unpacked(out) == _read(os.path.join(PAIRS_DIR, "out_b100.jsonl"))
    assert 2 in _btypes(out)


def test_bgzf_dynamic_needs_q(tmp_path):
    r = _run(["identify", "-c", os.path.join(PAIRS_DIR, "content.txt"), "-d", os.path.join(PAIRS_DIR, "idx"), "-i", os.path.join(PAIRS_DIR, "reads.fastq"),
              "-p", str(tmp_path / "prof.csv"), "--jsonl", "--bgzf-dynamic"], rc=1)
    assert r.stderr.startswith("ERROR: ") and "--bgzf" in r.stderr and "-q" in r.stderr
    assert not os.path.exists(str(tmp_path / "prof.csv"))              # before any work
