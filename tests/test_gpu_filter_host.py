"""`kasa_identify ... --filter <clean> <contaminants> --device-filter` against the files the reference binary wrote and against
the driver's own host path (--filter without the flag): the two files are split on the device batch by batch, the bytes are
the same; where the host has to write them after all (-v says so) they are the host path's."""
import gzip
import lzma
import os
import shutil
import subprocess

import pytest

from kasa_amd import build as hipbuild, capi, formats
from tests import filter_spec as spec, helpers

pytestmark = pytest.mark.gpu

PAIRS_DIR = os.path.join(helpers.GOLDEN, "pairs")
BATCHES = os.path.join(helpers.GOLDEN, "batches")
PARSER_LINE = "the host parser"
REWRITE_LINE = "OUT: --device-filter: the files are written by the host"
HOST_PATH_LINE = "OUT: --device-filter: the host path is used"
# --errorThreshold per edge file at which the host path puts reads into both files (read off the host path's own output)
EDGE_THRESHOLD = {"edge_crlf.fasta": "0.4", "edge_noeol.fasta": "0.3", "edge_multi.fastq": "0.14"}


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _run(args, env=None, rc=0):
    assert capi.device_count() > 0, "no HIP device visible"
    exe = hipbuild.build_host()
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert r.returncode == rc, r.stdout[-1000:] + r.stderr[-2000:]
    return r


def _filter(tmp_path, tag, infile, extra=(), env=None, device=True, with_q=True, sides=("c", "x"), d=PAIRS_DIR, inputs=None):
    """One run; returns (process, clean prefix, contaminants prefix)."""
    c = "_" if sides[0] == "_" else str(tmp_path / (tag + "_c"))
    x = "_" if sides[1] == "_" else str(tmp_path / (tag + "_x"))
    args = ["identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-p", str(tmp_path / (tag + ".csv")), "-v", "--jsonl", "-b", "100",
            "--filter", c, x] + (inputs or ["-i", infile]) + list(extra)
    if with_q:
        args += ["-q", str(tmp_path / (tag + ".out"))]
    if device:
        args.append("--device-filter")
    return _run(args, env=env), c, x


def _on_device(r):
    assert PARSER_LINE not in r.stdout and "written by the host" not in r.stdout and HOST_PATH_LINE not in r.stdout, r.stdout


FASTQ = ("reads.fastq", [], "flt_clean.fastq", "flt_cont.fastq")
FASTA = ("reads.fasta", ["--errorThreshold", "0.7"], "flta_clean.fasta", "flta_cont.fasta")
VARIANTS = {
    "plain": ([], None, True),
    "no-q": ([], None, False),
    "chunks": ([], {"KASA_READ_BLOCK": "1500"}, True),
    "batches": ([], {"KASA_MAX_BATCH_KMERS": "3000", "KASA_TEXT_PIECE": "777"}, True),
    "host-text": (["--host-text"], {"KASA_MAX_BATCH_KMERS": "3000"}, True),
    "host-rank": (["--host-rank"], None, False),
}


@pytest.mark.parametrize("case", [FASTQ, FASTA], ids=["fastq", "fasta"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_reference_files(case, variant, tmp_path):
    infile, thr, clean, cont = case
    extra, env, with_q = VARIANTS[variant]
    ext = os.path.splitext(clean)[1]
    r, c, x = _filter(tmp_path, "t", os.path.join(PAIRS_DIR, infile), thr + extra, env, with_q=with_q)
    _on_device(r)
    if variant in ("batches", "host-text"):
        assert sum(l.startswith("OUT: Batch of ") for l in r.stdout.splitlines()) > 2, r.stdout
    assert _bytes(c + ext) == _bytes(os.path.join(PAIRS_DIR, clean))
    assert _bytes(x + ext) == _bytes(os.path.join(PAIRS_DIR, cont))
    if with_q and not extra and infile == "reads.fastq":            # the per-read file leaves as before
        assert _bytes(str(tmp_path / "t.out")) == _bytes(os.path.join(PAIRS_DIR, "out_b100.jsonl"))


@pytest.mark.parametrize("sides", [("_", "x"), ("c", "_")], ids=["contaminants-only", "clean-only"])
def test_one_side(sides, tmp_path):
    r, c, x = _filter(tmp_path, "t", os.path.join(PAIRS_DIR, "reads.fastq"), sides=sides)
    _on_device(r)
    if sides[0] == "_":
        assert _bytes(x + ".fastq") == _bytes(os.path.join(PAIRS_DIR, "flt_cont.fastq"))
    else:
        assert _bytes(c + ".fastq") == _bytes(os.path.join(PAIRS_DIR, "flt_clean.fastq"))
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".fastq")) == ["t_x.fastq" if sides[0] == "_" else "t_c.fastq"]


def _is_bgzf_with_eof(data):
    assert data.endswith(formats.BGZF_EOF)
    sizes = [head["length"] for head, _, _, _ in formats.bgzf_members(data)]
    assert sizes and max(sizes) <= 65536 and sizes[-1] == 28


@pytest.mark.parametrize("extra", [[], ["--bgzf-dynamic"]], ids=["fixed", "dynamic"])
def test_gzip_gives_bgzf(extra, tmp_path):
    r, c, x = _filter(tmp_path, "t", os.path.join(PAIRS_DIR, "reads.fastq"), ["--gzip"] + extra, env={"KASA_MAX_BATCH_KMERS": "3000", "KASA_TEXT_PIECE": "500"})
    _on_device(r)
    for mine, ref in ((c + ".fastq.gz", "gflt_clean.fastq.gz"), (x + ".fastq.gz", "gflt_cont.fastq.gz")):
        data = _bytes(mine)
        _is_bgzf_with_eof(data)
        assert gzip.decompress(data) == gzip.open(os.path.join(PAIRS_DIR, ref)).read()


def test_device_inflate(tmp_path):
    exe = hipbuild.build_host()
    z = str(tmp_path / "reads.fastq.gz")
    assert subprocess.run([exe, "bgzf-dump", os.path.join(PAIRS_DIR, "reads.fastq"), z], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60).returncode == 0
    r, c, x = _filter(tmp_path, "t", z, ["--device-inflate"], env={"KASA_READ_BLOCK": "1500"})
    _on_device(r)
    assert "the host path is used" not in r.stdout
    assert _bytes(c + ".fastq") == _bytes(os.path.join(PAIRS_DIR, "flt_clean.fastq"))
    assert _bytes(x + ".fastq") == _bytes(os.path.join(PAIRS_DIR, "flt_cont.fastq"))


def _records_in(path, fasta):
    return len(spec.records(_bytes(path), fasta))


@pytest.mark.parametrize("name", list(EDGE_THRESHOLD))
def test_edge_files_against_the_host_path(name, tmp_path):
    ext = os.path.splitext(name)[1]
    thr = ["--errorThreshold", EDGE_THRESHOLD[name]]
    _, hc, hx = _filter(tmp_path, "host", os.path.join(PAIRS_DIR, name), thr, device=False)
    r, c, x = _filter(tmp_path, "dev", os.path.join(PAIRS_DIR, name), thr, env={"KASA_READ_BLOCK": "300"})
    _on_device(r)
    assert _records_in(hc + ext, ext == ".fasta") >= 1 and _records_in(hx + ext, ext == ".fasta") >= 1, "choose a threshold that fills both files"
    assert _bytes(c + ext) == _bytes(hc + ext) and _bytes(x + ext) == _bytes(hx + ext)


def test_no_read_flagged_copies_the_input(tmp_path):
    src = os.path.join(PAIRS_DIR, "edge_noeol.fasta")
    thr = ["--errorThreshold", "0"]
    _, hc, hx = _filter(tmp_path, "host", src, thr, device=False)
    r, c, x = _filter(tmp_path, "dev", src, thr)
    assert REWRITE_LINE + " (no read was flagged" in r.stdout and PARSER_LINE not in r.stdout, r.stdout
    assert _bytes(c + ".fasta") == _bytes(hc + ".fasta") == _bytes(src) and not _bytes(src).endswith(b"\n")
    assert _bytes(x + ".fasta") == _bytes(hx + ".fasta") == b""


@pytest.mark.parametrize("name", ["edge_noeol.fasta", "reads.fastq"])
def test_every_scored_read_flagged(name, tmp_path):
    ext = os.path.splitext(name)[1]
    thr = ["--errorThreshold", "1"]
    _, hc, hx = _filter(tmp_path, "host", os.path.join(PAIRS_DIR, name), thr, device=False)
    r, c, x = _filter(tmp_path, "dev", os.path.join(PAIRS_DIR, name), thr)
    _on_device(r)
    assert _records_in(hx + ext, ext == ".fasta") >= 1
    assert _bytes(c + ext) == _bytes(hc + ext) and _bytes(x + ext) == _bytes(hx + ext)


@pytest.fixture(scope="module")
def batches_case(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("flt_batches"))
    for f in ("content.txt.gz", "idx_f.txt.gz"):
        with gzip.open(os.path.join(BATCHES, f), "rb") as g, open(os.path.join(d, f[:-3]), "wb") as o:
            shutil.copyfileobj(g, o)
    for f in ("idx", "idx_info.txt", "idx_trie", "idx_trie.txt"):
        shutil.copy(os.path.join(BATCHES, f), os.path.join(d, f))
    with lzma.open(os.path.join(BATCHES, "long.fasta.xz"), "rb") as g, open(os.path.join(d, "long.fasta"), "wb") as o:
        shutil.copyfileobj(g, o)
    return d


def test_takeover_leaves_the_files_to_the_host(batches_case, tmp_path):
    d = batches_case
    extra, env = ["-m", "1", "-n", "1"], {"KASA_READ_BLOCK": "100000"}
    _, hc, hx = _filter(tmp_path, "host", os.path.join(d, "long.fasta"), extra, env, device=False, d=d)
    r, c, x = _filter(tmp_path, "dev", os.path.join(d, "long.fasta"), extra, env, d=d)
    assert "OUT: --device-parse: the host parser takes over from byte" in r.stdout, r.stdout
    assert REWRITE_LINE + " (the host parser took over)" in r.stdout, r.stdout
    assert _bytes(c + ".fasta") == _bytes(hc + ".fasta") and _bytes(x + ".fasta") == _bytes(hx + ".fasta")
    assert len(_bytes(c + ".fasta")) + len(_bytes(x + ".fasta")) > 100000


FALLBACKS = {
    "paired-end": (["-1", os.path.join(PAIRS_DIR, "pair_1.fastq"), "-2", os.path.join(PAIRS_DIR, "pair_2.fastq")], [], "paired-end input", ("_1.fastq", "_2.fastq")),
    "coherence": (None, ["--coherence", "-m", "4", "-n", "1"], "--coherence", (".fastq",)),
    "partition-0,0": (None, ["--partition-devices", "0,0"], "more than one device slot", (".fastq",)),
}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_fallbacks_keep_the_host_path(case, tmp_path):
    inputs, extra, why, exts = FALLBACKS[case]
    src = os.path.join(PAIRS_DIR, "reads.fastq")
    _, hc, hx = _filter(tmp_path, "host", src, extra, device=False, inputs=inputs)
    r, c, x = _filter(tmp_path, "dev", src, extra, inputs=inputs)
    assert HOST_PATH_LINE + " (" + why + ")" in r.stdout, r.stdout
    assert "OUT: --device-parse: the host parser is used (" in r.stdout and REWRITE_LINE not in r.stdout
    for ext in exts:
        assert _bytes(c + ext) == _bytes(hc + ext) and _bytes(x + ext) == _bytes(hx + ext)
        assert len(_bytes(c + ext)) + len(_bytes(x + ext)) > 1000


def test_the_flag_needs_filter_and_the_pinned_line_stays(tmp_path):
    d = PAIRS_DIR
    base = ["identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-i", os.path.join(d, "reads.fastq"), "-p", str(tmp_path / "p.csv"), "-v", "--jsonl"]
    r = _run(base + ["--device-filter", "-q", str(tmp_path / "o")], rc=1)
    assert "ERROR: --device-filter splits the files of --filter: it needs --filter" in r.stderr, r.stderr
    r = _run(base + ["--device-parse", "--filter", str(tmp_path / "c"), str(tmp_path / "x")])
    assert "OUT: --device-parse: the host parser is used (--filter writes the reads back from host memory)" in r.stdout
    assert "--device-filter" not in r.stdout
    assert _bytes(str(tmp_path / "c.fastq")) == _bytes(os.path.join(d, "flt_clean.fastq"))
