"""`kasa_identify identify ... -q <file> --bgzf`: decompressed, the file is byte for byte the file the same command line
writes without the flag (the golden files of the reference binary); it ends with BGZF's end-of-file block and every member
carries the BC subfield -- whoever made the member: the device (kasa_batch_bgzf) or a host thread (zlib)."""
import gzip
import lzma
import os
import shutil
import subprocess

import pytest

from kasa_amd import build as hipbuild, capi, formats
from tests import helpers
from tests.test_oracle_golden import PAIRS, _read, unpack

pytestmark = pytest.mark.gpu

FLAGS = {"json": "--json", "jsonl": "--jsonl", "tsv": "--tsv", "kraken": "--kraken"}
PAIRS_DIR = os.path.join(helpers.GOLDEN, "pairs")
BATCHES = os.path.join(helpers.GOLDEN, "batches")


def _run(args, env=None, rc=0):
    assert capi.device_count() > 0, "no HIP device visible"
    exe = hipbuild.build_host()
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == rc, (r.stdout[-1000:], r.stderr[-2000:])
    return r


def _unpacked(path):
    """the file's text; checks what every --bgzf file has"""
    z = open(path, "rb").read()
    assert z.endswith(formats.BGZF_EOF)
    members = list(formats.bgzf_members(z))                            # (raises where a member has no BC subfield)
    assert all(h["subfield"] == b"BC" and h["length"] <= 65536 for h, _, _, _ in members)
    assert all(isize > 0 for _, _, _, isize in members[:-1]) and members[-1][3] == 0    # an empty text gives no member
    return gzip.decompress(z).decode("latin-1")


def _pairs(infile, out, prof, extra, index="idx"):
    return ["identify", "-c", os.path.join(PAIRS_DIR, "content.txt"), "-d", os.path.join(PAIRS_DIR, index), "-i", os.path.join(PAIRS_DIR, infile),
            "-q", out, "-p", prof, "--bgzf"] + extra


ONE_OF_EACH = [next(c for c in PAIRS if unpack(c)[2] == fmt and unpack(c)[1] == "reads.fastq") for fmt in ("tsv", "json", "jsonl", "kraken")]
B100 = next(c for c in PAIRS if c[0] == "b100.jsonl")


@pytest.mark.parametrize("case", ONE_OF_EACH, ids=lambda c: c[0])
def test_one_per_format(case, tmp_path):
    stem, infile, fmt, kh, kl, frames, thr, beasts, idx, uniq = unpack(case)
    out, prof = str(tmp_path / "out.gz"), str(tmp_path / "prof.csv")
    _run(_pairs(infile, out, prof, [FLAGS[fmt], "-b", str(beasts), "-k", str(kh), str(kl), "-m", "4", "-n", "1"], idx))
    assert _unpacked(out) == _read(os.path.join(PAIRS_DIR, "out_" + stem))
    assert _read(prof) == _read(os.path.join(PAIRS_DIR, "prof_" + stem.rsplit(".", 1)[0] + ".csv"))      # untouched


@pytest.mark.parametrize("extra,env", [([], {}), (["--host-text"], {}), ([], {"KASA_TEXT_PIECE": "4099"}), (["--device-parse"], {})],
                         ids=["b100", "host-text", "piece4099", "device-parse"])
def test_b100_and_who_writes_it(extra, env, tmp_path):
    out, prof = str(tmp_path / "out.gz"), str(tmp_path / "prof.csv")
    _run(_pairs("reads.fastq", out, prof, ["--jsonl", "-b", "100"] + extra), env=env)
    assert _unpacked(out) == _read(os.path.join(PAIRS_DIR, "out_b100.jsonl"))
    assert _read(prof) == _read(os.path.join(PAIRS_DIR, "prof_b100.csv"))


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
Bgzf: true
""")
    _run(["--parameters", str(y)])
    assert _unpacked(out) == _read(os.path.join(PAIRS_DIR, "out_b100.jsonl"))


def test_paired_end(tmp_path):
    out, prof = str(tmp_path / "out.gz"), str(tmp_path / "prof.csv")
    _run(["identify", "-c", os.path.join(PAIRS_DIR, "content.txt"), "-d", os.path.join(PAIRS_DIR, "idx"), "-1", os.path.join(PAIRS_DIR, "pair_1.fastq"),
          "-2", os.path.join(PAIRS_DIR, "pair_2.fastq"), "-q", out, "-p", prof, "--jsonl", "-b", "100", "--bgzf"])
    assert _unpacked(out) == _read(os.path.join(PAIRS_DIR, "out_pair.jsonl"))


@pytest.fixture(scope="module")
def batches_case(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bgzf_batches"))
    for f in ("content.txt.gz", "idx_f.txt.gz"):
        with gzip.open(os.path.join(BATCHES, f), "rb") as g, open(os.path.join(d, f[:-3]), "wb") as o:
            shutil.copyfileobj(g, o)
    for f in ("idx", "idx_info.txt", "idx_trie", "idx_trie.txt", "reads.fastq.gz"):
        shutil.copy(os.path.join(BATCHES, f), os.path.join(d, f))
    with lzma.open(os.path.join(BATCHES, "long2.fasta.xz"), "rb") as g, open(os.path.join(d, "long2.fasta"), "wb") as o:
        shutil.copyfileobj(g, o)
    return d


def _gz_text(name):
    with gzip.open(os.path.join(BATCHES, name), "rb") as f:
        return f.read().decode("latin-1")


def test_three_batches(batches_case, tmp_path):
    """-m 1 cuts the input into the reference's three batches: three device streams behind one another"""
    import json
    d = batches_case
    out, prof = str(tmp_path / "out.gz"), str(tmp_path / "prof.csv")
    r = _run(["identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-i", os.path.join(d, "reads.fastq.gz"), "-q", out, "-p", prof,
              "--jsonl", "-b", "100", "-m", "1", "-n", "1", "-v", "--bgzf"])
    sizes = [int(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("OUT: Batch of ")]
    assert sizes == json.load(open(os.path.join(BATCHES, "batches.json")))["m1"] and len(sizes) == 3
    assert _unpacked(out) == _gz_text("out_m1.jsonl.gz")
    assert _read(prof) == _read(os.path.join(BATCHES, "prof_m1.csv"))


def test_reads_finished_from_carried_pieces(batches_case, tmp_path):
    """long2: batches begin and end inside a sequence, so the host writes them -- the unfinished reads by its one-read writer"""
    d = batches_case
    out, prof = str(tmp_path / "out.gz"), str(tmp_path / "prof.csv")
    r = _run(["identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-i", os.path.join(d, "long2.fasta"), "-q", out, "-p", prof,
              "--jsonl", "-b", "100", "-m", "1", "-n", "1", "-v", "--six", "--bgzf"])
    assert "the last goes on in the next" in r.stdout and "the first goes on from the batch before" in r.stdout
    assert _unpacked(out) == _gz_text("out_long2_six.jsonl.gz")
    assert _read(prof) == _read(os.path.join(BATCHES, "prof_long2_six.csv"))


def test_partitions_on_two_device_slots(tmp_path):
    """--partition-devices 0,0: two owners on the one device, each with its own stream of the batches it takes"""
    out, prof = str(tmp_path / "out.gz"), str(tmp_path / "prof.csv")
    _run(_pairs("reads.fastq", out, prof, ["--jsonl", "-b", "100", "--partition-devices", "0,0"]))
    assert _unpacked(out) == _read(os.path.join(PAIRS_DIR, "out_b100.jsonl"))
    assert _read(prof) == _read(os.path.join(PAIRS_DIR, "prof_b100.csv"))


def test_identify_multiple(tmp_path):
    ind = tmp_path / "in"
    ind.mkdir()
    src = {"sampleA.fastq": ("reads.fastq", "b100"), "sampleB.fasta": ("reads.fasta", "fasta")}
    for f, (orig, _) in src.items():
        shutil.copy(os.path.join(PAIRS_DIR, orig), str(ind / f))
    _run(["identify_multiple", "-c", os.path.join(PAIRS_DIR, "content.txt"), "-d", os.path.join(PAIRS_DIR, "idx"), "-i", str(ind) + "/",
          "-q", str(tmp_path / "rtt_"), "-p", str(tmp_path / "prof_"), "--jsonl", "-b", "100", "-n", "2", "--bgzf"])
    for f, (_, stem) in src.items():
        assert _unpacked(str(tmp_path / ("rtt_" + f.rsplit(".", 1)[0] + ".jsonl"))) == _read(os.path.join(PAIRS_DIR, "out_" + stem + ".jsonl")), f


def test_bgzf_needs_q(tmp_path):
    r = _run(["identify", "-c", os.path.join(PAIRS_DIR, "content.txt"), "-d", os.path.join(PAIRS_DIR, "idx"), "-i", os.path.join(PAIRS_DIR, "reads.fastq"),
              "-p", str(tmp_path / "prof.csv"), "--jsonl", "--bgzf"], rc=1)
    assert r.stderr.startswith("ERROR: ") and "--bgzf" in r.stderr and "-q" in r.stderr
    assert not os.path.exists(str(tmp_path / "prof.csv"))              # before any work
