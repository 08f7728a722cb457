"""CPU-only checks of the paired-end device path's plumbing: kasa_pair_take / kasa_pair_fetch are declared, exported and
bound; the driver knows --device-pairs; `pair-dump` (the host merge's tap) prints what `reads.parse_pairs` makes of two files."""
import os
import re
import subprocess

from kasa_amd import build as hipbuild, capi, reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kasa_pair_take", "kasa_pair_fetch"]


def pair_dump_text(ref) -> str:
    """What pair-dump / pair-dump-device print for a ReadBatch of pairs: protein line, then name, length, mate 1, mate 2."""
    o = ref.offsets
    mate = lambda s: bytes(ref.bases[int(o[s]):int(o[s + 1])]).decode("latin-1")
    return "protein=%d\n" % (1 if ref.protein else 0) + "".join(f"{ref.names[r]}\t{int(ref.lengths[r])}\t{mate(2 * r)}\t{mate(2 * r + 1)}\n" for r in range(ref.n))


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "kasa_hip.h")).read()
    declared = set(re.findall(r"^int\s+(kasa_pair_[a-z_]+)\(", header, re.M))
    assert declared == set(SYMBOLS)
    L = capi.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert s in capi.EXPORTS
    assert callable(capi.pair_take) and callable(capi.pair_fetch)
    assert callable(reads.parse_pairs_device)


def test_driver_accepts_the_option(tmp_path, golden_dir):
    exe = hipbuild.build_host()
    d = os.path.join(golden_dir, "pairs")
    run = lambda *a: subprocess.run([exe, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    pair = ["-1", os.path.join(d, "pair_1.fastq"), "-2", os.path.join(d, "pair_2.fastq")]
    # the option is parsed (the run gets as far as the index), a near miss still is not
    r = run("identify", "--device-pairs", "-d", os.path.join(d, "nope"), *pair)
    assert r.returncode == 1 and "Info file for this index can not be found!" in r.stderr, r.stderr
    r = run("identify", "--device-pair", "-d", os.path.join(d, "nope"), *pair)
    assert r.returncode == 1 and "unknown parameter" in r.stderr
    # ... and through --parameters
    y = tmp_path / "config.yaml"
    y.write_text(f"Mode: identify\nIndex: {os.path.join(d, 'nope')}\nInputFileOrFolder: {os.path.join(d, 'reads.fastq')}\nDevicePairs: true\n")
    r = run("--parameters", str(y))
    assert r.returncode == 1 and "--device-pairs" in r.stdout and "Info file for this index can not be found!" in r.stderr, r.stdout + r.stderr


def test_pair_dump_is_parse_pairs(golden_dir):
    exe = hipbuild.build_host()
    f1, f2 = (os.path.join(golden_dir, "pairs", n) for n in ("pair_1.fastq", "pair_2.fastq"))
    r = subprocess.run([exe, "pair-dump", f1, f2, "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=dict(os.environ, KASA_PARSE_CHUNK="400"))
    assert r.returncode == 0, r.stderr[-400:]
    ref = reads.parse_pairs(f1, f2)
    assert ref.n > 10
    assert r.stdout.decode("latin-1").split("\n", 2)[2] == pair_dump_text(ref)     # (the driver's two banner lines come first)
