"""CPU-only checks of the device parser's plumbing: the kasa_parse_* symbols are declared, exported and bound; the driver
knows --device-parse and keeps its messages; `parse-dump` (the host parser's tap) is what it was."""
import os
import re
import subprocess

import pytest

from kasa_amd import build as hipbuild, capi, reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kasa_parse_create", "kasa_parse_append", "kasa_parse_status", "kasa_parse_status_text", "kasa_parse_sizes", "kasa_parse_fetch",
           "kasa_parse_take", "kasa_parse_tile_bytes", "kasa_parse_stage_ms", "kasa_parse_destroy"]


def _driver():
    return hipbuild.build_host()              # cross-compiles where it is not built yet; a driver that does not compile fails the test


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "kasa_hip.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*\*?(kasa_parse_[a-z_]+)\(", header, re.M))
    assert declared == set(SYMBOLS)
    assert "typedef struct kasa_parser kasa_parser;" in header
    L = capi.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert s in capi.EXPORTS
    # host-only calls of the new surface work without a device
    T = capi.parse_tile_bytes()
    assert T >= 1024 and T % 1024 == 0
    assert L.kasa_parse_status_text(0) == b"parsable" and b"space or tab" in L.kasa_parse_status_text(6)
    for name in ("append", "status", "sizes", "fetch", "take", "stage_ms", "close"):
        assert callable(getattr(capi.Parser, name))
    assert callable(reads.parse_reads_device)


def test_no_pool_without_a_device():
    if capi.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(RuntimeError, match="no HIP device"):
        capi.Parser(0)


def test_driver_accepts_the_option_and_keeps_its_messages(tmp_path, golden_dir):
    exe = _driver()
    d = os.path.join(golden_dir, "pairs")
    run = lambda *a: subprocess.run([exe, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    # a missing input is reported as before, with the option before or after it
    for args in (["identify", "--device-parse", "-i", os.path.join(d, "nope.fastq")], ["identify", "-i", os.path.join(d, "nope.fastq"), "--device-parse"]):
        r = run(*args)
        assert r.returncode == 1 and "Input file not found" in r.stderr, r.stderr
    # the option is parsed (the run gets as far as the index), an unknown one still is not
    r = run("identify", "--device-parse", "-d", os.path.join(d, "nope"), "-i", os.path.join(d, "reads.fastq"))
    assert r.returncode == 1 and "Info file for this index can not be found!" in r.stderr, r.stderr
    r = run("identify", "--device-parsing")
    assert r.returncode == 1 and "unknown parameter" in r.stderr
    # ... and through --parameters
    y = tmp_path / "config.yaml"
    y.write_text(f"Mode: identify\nIndex: {os.path.join(d, 'nope')}\nInputFileOrFolder: {os.path.join(d, 'reads.fastq')}\nDeviceParse: true\n")
    r = run("--parameters", str(y))
    assert r.returncode == 1 and "--device-parse" in r.stdout and "Info file for this index can not be found!" in r.stderr, r.stdout + r.stderr


@pytest.mark.parametrize("name", ["reads.fastq", "reads.fasta", "edge_crlf.fasta", "edge_multi.fastq", "edge_noeol.fasta"])
def test_parse_dump_is_unchanged(name, golden_dir):
    exe = _driver()
    path = os.path.join(golden_dir, "pairs", name)
    r = subprocess.run([exe, "parse-dump", path, "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                       env=dict(os.environ, KASA_READ_BLOCK="1500", KASA_PARSE_CHUNK="400"))
    assert r.returncode == 0, r.stderr[-400:]
    ref = reads.parse_reads(path)
    want = "".join(f"{ref.names[i]}\t{int(ref.lengths[i])}\t{bytes(ref.bases[int(ref.offsets[i]):int(ref.offsets[i + 1])]).decode('latin-1')}\n" for i in range(ref.n))
    streamed = r.stdout.decode("latin-1").split("== streamed\n")[1]
    head, body = streamed.split("\n", 1)
    assert head.startswith("protein=%d" % (1 if ref.protein else 0)) and body == want
