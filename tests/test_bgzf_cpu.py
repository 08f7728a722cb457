"""BGZF on the host (no device): formats.bgzf_compress / bgzf_members and the driver's `bgzf-dump` tap make streams that every
gzip reader takes -- members that say their own length (BSIZE), hold at most 65 280 bytes each and inflate on their own."""
import glob
import gzip
import os
import random
import subprocess
import zlib

import pytest

from kasa_amd import build as hipbuild, formats
from tests import helpers

PAIRS_DIR = os.path.join(helpers.GOLDEN, "pairs")
BLOCK = 65280


def golden_texts():
    """every golden per-read file of tests/golden/pairs"""
    return sorted(f for ext in ("json", "jsonl", "tsv", "ktsv") for f in glob.glob(os.path.join(PAIRS_DIR, "out_*." + ext)))


def _random(n, seed):
    return random.Random(seed).randbytes(n)


def inputs():
    """name -> bytes: the smallest inputs at which each part of a block compressor can go wrong"""
    d = {"len%d" % n: b"kasa"[:n] for n in (0, 1, 2, 3, 4)}
    text = open(os.path.join(PAIRS_DIR, "out_default.json"), "rb").read() * 9
    for n in (65279, 65280, 65281, 3 * 65280 + 17):
        d["text%d" % n] = text[:n]
    d["zeros"] = bytes(200000)
    d["random70000"] = _random(70000, 1)
    d["period"] = bytes(range(256)) * 300
    d["runs"] = b"".join(bytes([65 + i]) * k + bytes([48 + i]) for i, k in enumerate((257, 258, 259, 260, 517)))
    r = _random(32769, 2)
    d["twice32768"] = r[:32768] * 2
    d["twice32769"] = r * 2
    r = _random(20000, 3)
    d["own_start"] = r + r[:10000]
    return d


INPUTS = inputs()


def check_stream(stream, data, device=False):
    """`stream` (no EOF block) is BGZF of `data`; returns the members' (BTYPE, length) list."""
    assert gzip.decompress(stream + formats.BGZF_EOF) == data          # (every member's CRC-32 and ISIZE)
    at, kinds = 0, []
    for head, payload, crc, isize in formats.bgzf_members(stream):
        assert head["length"] == head["bsize"] + 1 and head["length"] <= 65536
        assert head["subfield"] == b"BC" and head["xlen"] == 6 and head["mtime"] == 0 and head["os"] == 255
        assert 0 < isize <= BLOCK
        if device:
            assert at % BLOCK == 0                                      # block i covers [i 65280, ...)
            assert isize == min(BLOCK, len(data) - at)
        z = zlib.decompressobj(-15)
        piece = z.decompress(payload) + z.flush()
        assert z.eof and not z.unused_data
        assert piece == data[at:at + isize] and zlib.crc32(piece) == crc
        kinds.append(((payload[0] >> 1) & 3, head["length"]))
        at += isize
    assert at == len(data)
    assert sum(n for _, n in kinds) == len(stream)
    return kinds


@pytest.mark.parametrize("name", list(INPUTS))
def test_bgzf_compress(name):
    data = INPUTS[name]
    stream = formats.bgzf_compress(data)
    kinds = check_stream(stream, data)
    assert len(kinds) == (len(data) + BLOCK - 1) // BLOCK
    assert (stream == b"") == (data == b"")


def test_eof_block_is_an_empty_member():
    assert len(formats.BGZF_EOF) == 28 and gzip.decompress(formats.BGZF_EOF) == b""
    (head, payload, crc, isize), = formats.bgzf_members(formats.BGZF_EOF)
    assert head["length"] == 28 and payload == b"\x03\x00" and crc == 0 and isize == 0
    with pytest.raises(ValueError):
        list(formats.bgzf_members(gzip.compress(b"plain gzip has no BC subfield")))
    with pytest.raises(ValueError):
        list(formats.bgzf_members(formats.BGZF_EOF[:-1]))


@pytest.mark.parametrize("name", ["out_default.json", "out_b100.jsonl", "out_b100.tsv", "empty"])
def test_driver_bgzf_dump(name, tmp_path):
    exe = hipbuild.build_host()
    src = os.path.join(PAIRS_DIR, name)
    if name == "empty":
        src = str(tmp_path / "empty")
        open(src, "wb").close()
    data = open(src, "rb").read()
    out = str(tmp_path / "out.gz")
    r = subprocess.run([exe, "bgzf-dump", src, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    z = open(out, "rb").read()
    assert z.endswith(formats.BGZF_EOF)
    kinds = check_stream(z[:-28], data)
    assert len(kinds) == (len(data) + BLOCK - 1) // BLOCK
