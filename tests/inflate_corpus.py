"""The corpus of BGZF spans that tests/test_inflate_cpu.py and tests/test_gpu_inflate.py share: the smallest members at which
each part of an inflater can go wrong, all made here with Python's zlib (raw deflate, wbits = -15) in BGZF headers, and the
malformed members made by editing bytes of valid ones.  A case is (name, span, raw, status): raw = the text of a valid
span (status None), or status = (KASA_INFLATE_* code, member index) of a span that has to be rejected (raw None)."""
import functools
import gzip
import os
import struct
import subprocess
import zlib

from kasa_amd import build as hipbuild, formats
from tests.test_bgzf_cpu import INPUTS

BLOCK = formats.BGZF_BLOCK
# include/kasa_hip.h
HEADER, CUT, TRUNCATED, BTYPE, STORED_LEN, CODE_LENGTHS, SYMBOL, DISTANCE, OVERRUN, SHORT, TRAILING, CRC = range(1, 13)

MODES = {
    "stored": dict(level=0),
    "level1": dict(level=1),
    "level9": dict(level=9),
    "fixed": dict(level=6, strategy=zlib.Z_FIXED),
    "huffman": dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY),     # dynamic blocks without a distance code
    "rle": dict(level=6, strategy=zlib.Z_RLE),                  # distance 1, lengths to 258
}


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0, flush=zlib.Z_FULL_FLUSH):
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if not flush_every:
        return z.compress(raw) + z.flush()
    out = []
    for a in range(0, len(raw), flush_every):
        out.append(z.compress(raw[a:a + flush_every]) + z.flush(flush))
    return b"".join(out) + z.flush()


def member(raw, payload):
    assert 18 + len(payload) + 8 <= 65536 and len(raw) <= 65536
    return formats.BGZF_EOF[:16] + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload + struct.pack("<II", zlib.crc32(raw), len(raw))


def members(data, block=BLOCK, **kw):
    """data as a list of members of at most `block` bytes each (halved where the deflate data would not fit BSIZE)"""
    out, a = [], 0
    while a < len(data):
        n = min(block, len(data) - a)
        while True:
            payload = deflate(data[a:a + n], **kw)
            if 18 + len(payload) + 8 <= 65536:
                break
            n //= 2
        out.append(member(data[a:a + n], payload))
        a += n
    return out


def stream(data, block=BLOCK, **kw):
    return b"".join(members(data, block, **kw))


def edit_member(m, payload=None, crc=None, isize=None):
    """a member with parts replaced; BSIZE follows the payload"""
    p0, c0, i0 = m[18:-8], *struct.unpack("<II", m[-8:])
    payload = p0 if payload is None else payload
    return m[:16] + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload + struct.pack("<II", c0 if crc is None else crc, i0 if isize is None else isize)


def zlib_rejects_payload(payload):
    z = zlib.decompressobj(-15)
    try:
        z.decompress(payload)
    except zlib.error:
        return True
    return not z.eof or bool(z.unused_data)


def gzip_rejects(span):
    try:
        gzip.decompress(span)
    except (OSError, EOFError, zlib.error):
        return True
    return False


def _set_bits(buf, at, n, value):
    for i in range(n):
        byte, bit = (at + i) >> 3, (at + i) & 7
        buf[byte] = (buf[byte] & ~(1 << bit)) | (((value >> i) & 1) << bit)


@functools.lru_cache(maxsize=None)
def cases():
    text = INPUTS["text65280"]
    out = []
    for name, data in INPUTS.items():
        for mode, kw in MODES.items():
            out.append(("%s_%s" % (name, mode), stream(data, **kw), data, None))
    out.append(("zeros_level6", stream(INPUTS["zeros"], level=6), INPUTS["zeros"], None))                  # a block with ONE distance code
    out.append(("twice32768_level6", stream(INPUTS["twice32768"], level=6), INPUTS["twice32768"], None))   # a match at distance 32768
    t = text[:20000]
    flushed = member(t, deflate(t, level=6, flush_every=1000))
    assert flushed.count(b"\x00\x00\xff\xff") >= 19                                    # many blocks, and the empty stored block
    out.append(("fullflush", flushed, t, None))
    out.append(("syncflush", member(t, deflate(t, level=6, flush_every=777, flush=zlib.Z_SYNC_FLUSH)), t, None))
    # (a STORED member of ISIZE 65536 does not exist: 65536 + 10 + 26 bytes are more than BSIZE can say.  The two properties apart:)
    big = (text * 2)[:65536]
    out.append(("isize65536", member(big, deflate(big, level=6)), big, None))
    t = INPUTS["random70000"][:65000]
    two = member(t, deflate(t, level=0, flush_every=40000))
    out.append(("stored_two_blocks", two, t, None))
    out.append(("isize1", stream(b"k", level=6), b"k", None))
    out.append(("isize1_stored", stream(b"k", level=0), b"k", None))
    ms = members(text[:3000], block=1000, level=6)
    out.append(("eof_middle_and_end", ms[0] + formats.BGZF_EOF + ms[1] + ms[2] + formats.BGZF_EOF, text[:3000], None))
    out.append(("eof_only", formats.BGZF_EOF, b"", None))

    # ---- malformed: member 1 of three is edited, so the index that comes back says something
    good = members(text[:6000], block=2000, level=9)
    def bad(name, m1, status, at=1):
        out.append((name, good[0] + m1 + good[2], None, (status, at)))
    m = good[1]
    payload, (crc, isize) = m[18:-8], struct.unpack("<II", m[-8:])
    assert (payload[0] >> 1) & 3 == 2                                                  # a dynamic block
    cut = edit_member(m, payload=payload[:-1])
    assert zlib_rejects_payload(payload[:-1])
    bad("bad_payload_short", cut, TRUNCATED)
    for name, mm, status in (("bad_crc_bit", edit_member(m, crc=crc ^ 0x00010000), CRC), ("bad_isize_plus", edit_member(m, isize=isize + 1), SHORT),
                             ("bad_isize_minus", edit_member(m, isize=isize - 1), OVERRUN)):
        assert gzip_rejects(mm) and not zlib_rejects_payload(payload)
        bad(name, mm, status)
    p = bytearray(payload); p[0] |= 6
    assert zlib_rejects_payload(bytes(p))
    bad("bad_btype3", edit_member(m, payload=bytes(p)), BTYPE)
    p = bytearray(payload)
    hclen = ((p[1] >> 6) | (p[2] << 2)) & 15                                           # bits 13..16
    for i in range(hclen + 4):
        _set_bits(p, 17 + 3 * i, 3, 1)                                                 # every code-length code one bit long
    assert zlib_rejects_payload(bytes(p))
    bad("bad_oversubscribed", edit_member(m, payload=bytes(p)), CODE_LENGTHS)
    s = members(text[2000:4000], level=0)[0]
    p = bytearray(s[18:-8]); assert p[0] == 1
    p[3] ^= 0x10                                                                       # NLEN
    assert zlib_rejects_payload(bytes(p))
    bad("bad_stored_len", edit_member(s, payload=bytes(p)), STORED_LEN)
    f = members(text[2000:4000], level=6, strategy=zlib.Z_FIXED)[0]
    p = bytearray(f[18:-8]); assert p[0] & 7 == 3
    p[0], p[1] = 0x03, 0x02                                                            # fixed block; symbol 257 (length 3), distance code 0
    assert zlib_rejects_payload(bytes(p))
    bad("bad_first_is_match", edit_member(f, payload=bytes(p)), DISTANCE)
    p = bytearray(f[18:-8]) + b"\x00"
    assert zlib_rejects_payload(bytes(p))
    bad("bad_trailing_byte", edit_member(f, payload=bytes(p)), TRAILING)
    cutspan = good[0] + good[1][:10]
    assert gzip_rejects(cutspan)
    out.append(("bad_cut_in_header", cutspan, None, (CUT, 1)))
    out.append(("bad_cut_in_payload", good[0] + good[1][:-9], None, (CUT, 1)))
    plain = gzip.compress(text[:2000])
    with_plain = good[0] + plain
    out.append(("bad_not_bgzf", with_plain, None, (HEADER, 1)))
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def write_corpus(directory, only=None):
    for name, span, raw, status in cases():
        if only is not None and name not in only:
            continue
        with open(os.path.join(directory, name + ".bgzf"), "wb") as f:
            f.write(span)
        if raw is not None:
            with open(os.path.join(directory, name + ".raw"), "wb") as f:
                f.write(raw)
        else:
            with open(os.path.join(directory, name + ".status"), "w") as f:
                f.write("%d %d\n" % status)


_HOST = {}


def host_check(tmp_dir):
    """tools/inflate_host_check (AddressSanitizer + UBSan) over the whole corpus, once per session: name -> True / False by
    its report lines, and the run's exit code and output."""
    if not _HOST:
        exe = hipbuild.build_inflate_check()
        write_corpus(tmp_dir)
        r = subprocess.run([exe, tmp_dir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        ok = {}
        for line in r.stdout.splitlines():
            if ": status " in line and not line.startswith(" "):
                ok[line.split(":", 1)[0]] = "MISMATCH" not in line
        _HOST.update(ok=ok, returncode=r.returncode, output=r.stdout)
    return _HOST

