"""tests/filter_spec.py (the record text of a read and the split of --filter) against the reference's own files and against
report.filter_reads; the C ABI of the device split is exported and declared."""
import os
import re

import pytest

from kasa_amd import capi, report
from tests import filter_spec as spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = os.path.join(ROOT, "tests", "golden", "pairs")
NEW_SYMBOLS = ("kasa_pool_keep_records", "kasa_pool_fetch_records", "kasa_batch_filter", "kasa_batch_filter_fetch_range", "kasa_filter_split")


def _read(name):
    with open(os.path.join(PAIRS, name), "rb") as f:
        return f.read()


def _via_report(tmp_path, name, flags):
    clean, cont = str(tmp_path / "clean"), str(tmp_path / "cont")
    report.filter_reads([os.path.join(PAIRS, name)], [i for i, f in enumerate(flags) if f], clean, cont)
    ext = os.path.splitext(name)[1]
    with open(clean + ext, "rb") as a, open(cont + ext, "rb") as b:
        return a.read(), b.read()


@pytest.mark.parametrize("name,clean,cont", [("reads.fastq", "flt_clean.fastq", "flt_cont.fastq"), ("reads.fasta", "flta_clean.fasta", "flta_cont.fasta")])
def test_reference_files(tmp_path, name, clean, cont):
    fasta = name.endswith(".fasta")
    recs = spec.records(_read(name), fasta)
    want_clean, want_cont = _read(clean), _read(cont)
    flagged = {spec.header_of(r) for r in spec.records(want_cont, fasta)}
    assert len({spec.header_of(r) for r in recs}) == len(recs), "the headers tell the reads apart"
    flags = [1 if spec.header_of(r) in flagged else 0 for r in recs]
    assert 0 < sum(flags) < len(recs)
    got_clean, got_cont, n_clean, n_cont = spec.split(recs, flags)
    assert (got_clean, got_cont) == (want_clean, want_cont)
    assert (n_clean, n_cont) == (len(recs) - sum(flags), sum(flags))
    assert _via_report(tmp_path, name, flags) == (want_clean, want_cont)


@pytest.mark.parametrize("name", ["edge_crlf.fasta", "edge_noeol.fasta", "edge_multi.fastq"])
def test_edge_files_every_second_read(tmp_path, name):
    text = _read(name)
    recs = spec.records(text, name.endswith(".fasta"))
    assert len(recs) >= 2
    flags = [r & 1 for r in range(len(recs))]
    clean, cont, _, _ = spec.split(recs, flags)
    assert (clean, cont) == _via_report(tmp_path, name, flags)
    assert clean and cont
    off = spec.offsets(recs)
    assert int(off[-1]) == len(clean) + len(cont) and all(r.endswith(b"\n") and b"\n\n" not in r for r in recs)


def test_record_text_rules():
    assert spec.records(b">a\r\nAC\r\n\r\n\n>b\nGG", True) == [b">a\r\nAC\r\n\r\n", b">b\nGG\n"]
    assert spec.records(b">\n\n\n>x\n", True) == [b">\n", b">x\n"]
    assert spec.records(b"@a\nAC\n+a\nII", False) == [b"@a\nAC\n+a\nII\n"]
    assert spec.split([b"1\n", b"22\n", b"333\n"], [0, 1, 0]) == (b"1\n333\n", b"22\n", 2, 1)


def test_symbols_exported_and_declared():
    with open(os.path.join(ROOT, "include", "kasa_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name in capi.EXPORTS, name
        assert re.search(r"^int %s\(" % name, header, re.M), name


def test_driver_knows_the_option(tmp_path):
    import subprocess
    from kasa_amd import build as hipbuild
    exe = hipbuild.build_host()
    run = lambda *a: subprocess.run([exe, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    reads_in = ["-i", os.path.join(PAIRS, "reads.fastq"), "-d", os.path.join(PAIRS, "nope")]
    r = run("identify", "--device-filter", "--filter", str(tmp_path / "c"), str(tmp_path / "x"), *reads_in)      # parsed: the run gets as far as the index
    assert r.returncode == 1 and "Info file for this index can not be found!" in r.stderr, r.stderr
    r = run("identify", "--device-filter", *reads_in)
    assert r.returncode == 1 and "--device-filter splits the files of --filter: it needs --filter" in r.stderr, r.stderr
    r = run("identify", "--device-filte", *reads_in)
    assert r.returncode == 1 and "unknown parameter" in r.stderr
    y = tmp_path / "config.yaml"
    y.write_text(f"Mode: identify\nIndex: {os.path.join(PAIRS, 'nope')}\nInputFileOrFolder: {os.path.join(PAIRS, 'reads.fastq')}\nDeviceFilter: true\n")
    r = run("--parameters", str(y))
    assert r.returncode == 1 and "--device-filter" in r.stdout + r.stderr, r.stdout + r.stderr
