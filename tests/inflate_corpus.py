"""The corpus of BGZF spans that tests/test_inflate_cpu.py and tests/test_gpu_inflate.py share: the smallest members at which
each part of an inflater can go wrong, all made here with Python's zlib (raw deflate, wbits = -15) in BGZF headers, and the
malformed members made by editing bytes of valid ones.  A case is (name, span, raw, status): raw = the text of a valid
span (status None), or status = (KASA_INFLATE_* code, member index) of a span that has to be rejected (raw None).

cases() is what zlib's COMPRESSOR writes; built_cases() is what it never writes -- members made by construction with
tests/deflate_writer.py in groups A..H (listed at built_cases and in DESIGN.md 8f), each judged by zlib's INFLATER where it is
made.  All randomness is random.Random(seed) with the seeds written here; nothing is read from a fixture but the FASTQ text."""
import functools
import gzip
import os
import random
import struct
import subprocess
import zlib

from kasa_amd import build as hipbuild, formats
from tests import deflate_writer as W
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


# ---- members zlib's compressor never writes: made by tests/deflate_writer.py, judged by zlib's INFLATER ----------------------
GROUPS = "ABCDEFG"                                 # the valid groups; H is the malformed one
G_SEEDS = range(300)
HEADER_OFFSETS = range(236, 266)                   # where a dynamic header's first byte lies, around the window's reload mark (256)
HEADER316_OFFSETS = range(250, 257)
FASTQ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairs", "reads.fastq")


def zlib_inflates_to(payload, raw):
    z = zlib.decompressobj(-15)
    try:
        return z.decompress(payload) == raw and z.eof and not z.unused_data
    except zlib.error:
        return False


def _comb(symbols, size):
    """code lengths 1, 2, ..., n-1, n-1 on `symbols` in that order: complete, every length to n-1 in use"""
    lens = [0] * size
    for k, s in enumerate(symbols):
        lens[s] = min(k + 1, len(symbols) - 1)
    assert W.kraft(lens) == 32768
    return lens


def _header316(p, rng, tokens, final):
    """the longest dynamic header there is: 316 lengths of 7 bits each and no repeat (about 286 bytes)"""
    ll = [8] * 226 + [9] * 60
    dl = [4] * 2 + [5] * 28
    rng.shuffle(ll)
    rng.shuffle(dl)
    cl = [0] * 19
    for s, n in ((0, 1), (1, 2), (2, 3), (3, 4), (6, 5), (4, 7), (5, 7), (8, 7), (9, 7)):
        cl[s] = n
    p.dynamic(tokens, ll, dl, final, cl_lengths=cl, rle="none")
    b = p.blocks[-1]
    assert b["hclen"] == 18 and b["header_end_bit"] - b["bit"] == 17 + 18 * 3 + 316 * 7
    return p


def _g_member(rng, tokens=None):
    """group G's member: random complete codes to 15 bits on the symbols used, HLIT / HDIST minimal or maximal, 1-3 blocks,
    the header's run-length coding by chance.  tokens: a text's own (the parser test) instead of random ones"""
    if tokens is None:
        size = rng.choice([50, 300, 3000, 20000])
        literals = rng.sample(range(256), rng.randint(2, 40))
        len_syms = rng.sample(range(29), rng.randint(1, 29))
        dist_syms = rng.sample(range(30), rng.randint(1, 30))
        tokens = W.random_tokens(rng, size, literals, len_syms, dist_syms)
    maximal = rng.random() < 0.5
    parts = W.split_blocks(rng, tokens, rng.randint(1, 3))
    p = W.Payload()
    for k, part in enumerate(parts):
        W.random_dynamic(p, rng, part, k == len(parts) - 1, hlit=286 if maximal else None, hdist=30 if maximal else None)
    return p, tokens


def _lits(rng, n, alphabet=range(256)):
    alphabet = list(alphabet)
    return [rng.choice(alphabet) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _built():
    out, info = [], {}
    R = random.Random

    def valid(name, p, raw):
        """one member; zlib's inflater gives exactly `raw` from it and stops at its end"""
        raw = W.expand(raw) if isinstance(raw, list) else bytes(raw)
        payload = p.getvalue()
        assert len(payload) <= W.MAX_PAYLOAD and len(raw) <= 65536 and p.pos == len(raw), name
        assert zlib_inflates_to(payload, raw), name
        out.append((name, member(raw, payload), raw, None))
        info[name] = [p.blocks]

    # ---- A. alphabets
    for kind in ("fixed", "dynamic"):
        rng = R(1000 + (kind == "dynamic"))
        toks = _lits(rng, 33000, range(144) if kind == "fixed" else rng.sample(range(256), 16))
        for i in range(29):
            lo, hi = W.LEN_BASE[i], W.LEN_BASE[i] + (1 << W.LEN_EXTRA[i]) - 1
            toks.append((lo, rng.randint(1, 1000)))
            toks.append((258, rng.randint(1, 1000), W.AS_284) if i == 27 else (hi, rng.randint(1, 1000)))
        for i in range(30):
            toks.append((rng.randint(3, 12), W.DIST_BASE[i]))
            toks.append((rng.randint(3, 12), W.DIST_BASE[i] + (1 << W.DIST_EXTRA[i]) - 1))
        p = W.Payload()
        if kind == "fixed":
            p.fixed(toks, True)
        else:
            W.random_dynamic(p, rng, toks, True)
        valid("A_alphabet_" + kind, p, toks)
    for d in (1, 300):
        rng = R(1010 + d)
        toks = _lits(rng, 300) + [(n, d) for n in range(3, 259)]
        valid("A_lengths_d%d_fixed" % d, W.Payload().fixed(toks, True), toks)
        toks = _lits(rng, 300, rng.sample(range(256), 20)) + rng.sample([(n, d) for n in range(3, 259)], 256)
        valid("A_lengths_d%d_dynamic" % d, W.random_dynamic(W.Payload(), rng, toks, True), toks)
    toks = [7, 8, 9, 10, 11, (258, 1, W.AS_284), (258, 5, W.AS_284), 12, (258, 263, W.AS_284)]
    valid("A_258_as_284_31", W.Payload().fixed(toks, True), toks)
    toks = _lits(R(1020), 32768, range(144)) + [(258, 32768)]
    valid("A_distance32768_to_isize", W.Payload().fixed(toks, True), toks)

    # ---- B. code shapes
    rng = R(2000)
    lits15 = list(range(65, 80))
    for name, order in (("eob15", lits15 + [256]), ("eob1", [256] + lits15)):
        toks = _lits(rng, 400, lits15)
        valid("B_litlen_1_to_15_" + name, W.Payload().dynamic(toks, _comb(order, 257), [0], True), toks)
    order = list(range(16)); rng.shuffle(order)
    toks = _lits(rng, 400, range(97, 105)) + [(rng.randint(3, 20), W.DIST_BASE[d] + rng.randrange(1 << W.DIST_EXTRA[d])) for d in list(range(16)) * 3]
    ls, _ = W.used_symbols(toks)
    valid("B_distance_1_to_15", W.Payload().dynamic(toks, W.code_for(rng, ls, max(ls) + 1), _comb(order, 16), True), toks)
    # 48 bits in one match: a 15-bit code with 5 extra bits, a 15-bit code with 13
    head = rng.randbytes(33000)
    toks = _lits(rng, 30, lits15[:13])
    for _ in range(40):
        toks += [(227 + rng.randrange(31), 24577 + rng.randrange(8192)), rng.choice(lits15[:13]), (195 + rng.randrange(32), 16385 + rng.randrange(8192))]
    toks += [(258, 32768, W.AS_284), (257, 32768), (227, 24577)]
    p = W.Payload().stored(head, False).dynamic(toks, _comb(lits15[:13] + [256, 284, 283], 285), _comb(list(range(14)) + [29, 28], 30), True)
    valid("B_48_bit_match", p, head + W.expand(list(head) + toks)[len(head):])
    valid("B_only_end_of_block_final", W.Payload().dynamic([], [0] * 256 + [1], [0], True), b"")
    toks = _lits(rng, 50)
    valid("B_only_end_of_block_then_data", W.Payload().dynamic([], [0] * 256 + [1], [0], False).fixed(toks, True), toks)
    toks = _lits(rng, 300, range(48, 58))
    valid("B_hdist1_no_distance_code", W.Payload().dynamic(toks, W.code_for(rng, W.used_symbols(toks)[0], 257), [0], True), toks)
    toks = [33] + [(n, 1) for n in (3, 4, 17, 258, 100)] + [34, (9, 1)]
    valid("B_hdist1_one_bit_code", W.Payload().dynamic(toks, W.code_for(rng, W.used_symbols(toks)[0], 286), [1], True), toks)
    toks = _lits(rng, 200, range(100, 130))
    valid("B_hlit257", W.Payload().dynamic(toks, W.code_for(rng, W.used_symbols(toks)[0], 257), [0], True), toks)
    toks = _lits(rng, 300, range(100, 130)) + [(258, 7), (258, 300), (3, 2)]
    ls, ds = W.used_symbols(toks)
    assert 285 in ls
    valid("B_hlit286", W.Payload().dynamic(toks, W.code_for(rng, ls, 286), W.code_for(rng, ds, max(ds) + 1), True), toks)
    head = rng.randbytes(25000)
    toks = _lits(rng, 20, range(100, 130)) + [(10, 24577), (20, 25000), (5, 3)]
    ls, ds = W.used_symbols(toks)
    assert 29 in ds
    p = W.Payload().stored(head, False).dynamic(toks, W.code_for(rng, ls, max(ls) + 1), W.code_for(rng, ds, 30), True)
    valid("B_hdist30", p, head + W.expand(list(head) + toks)[len(head):])

    # ---- C. dynamic headers
    rng = R(3000)
    toks = _lits(rng, 200, lits15[:13]) + [(5, 9), (40, 100)]
    ls, ds = W.used_symbols(toks)
    order = sorted(ls); rng.shuffle(order)
    cl = W.flat_code(19); rng.shuffle(cl)
    p = W.Payload().dynamic(toks, _comb(order, max(ls) + 1), W.code_for(rng, ds, max(ds) + 1), True, cl_lengths=cl, hclen=19)
    assert {s for s, _, _ in p.blocks[0]["items"]} >= set(range(1, 16)) and len(order) >= 16
    valid("C_hclen19", p, toks)
    toks = _lits(rng, 300, range(255))
    cl = [0] * 19; cl[0] = cl[8] = 1
    p = W.Payload().dynamic(toks, [8] * 255 + [0, 8], [0], True, cl_lengths=cl, rle="none")
    assert p.blocks[0]["hclen"] == 5
    valid("C_hclen5_smallest", p, toks)
    five = [97, 98, 99, 100, 101]
    toks = _lits(rng, 100, five) + [(3, 1), (4, 2)]
    ll, dl = _comb(five + [256] + [257, 258], 259), [1, 1]
    used = sorted(set(ll + dl))
    assert len(used) == 8 and used[0] == 0
    cl = [0] * 19
    for k, s in enumerate(used):
        cl[s] = min(k + 1, 7)
    p = W.Payload().dynamic(toks, ll, dl, True, cl_lengths=cl, rle="none")
    valid("C_code_length_code_7_bits", p, toks)
    ll = [0] * 257
    for s in [138, 150, 161] + list(range(165, 172)) + list(range(173, 177)):
        ll[s] = 4
    ll[256] = 3
    items = [(18, 138), (4, 1), (18, 11), (4, 1), (17, 10), (4, 1), (17, 3), (4, 1), (16, 6), (0, 1), (4, 1), (16, 3), (18, 79), (3, 1), (0, 1)]
    toks = _lits(rng, 100, [s for s in range(256) if ll[s]])
    valid("C_repeats_at_both_ends", W.Payload().dynamic(toks, ll, [0], True, rle=items), toks)
    ll = [0] * 258
    ll[65] = ll[66] = 2
    ll[254] = ll[255] = ll[256] = ll[257] = 3
    toks = [65, 66, 254, 255, (3, 1), (3, 2), (3, 3), (3, 4), (3, 5), 65, (3, 6)]
    p = W.Payload().dynamic(toks, ll, [3, 3, 3, 3, 1], True, rle=W.rle_items(ll[:255], "greedy") + [(16, 6), (3, 1), (1, 1)])
    valid("C_16_across_hlit", p, toks)
    ll = [0] * 272
    ll[65], ll[256], ll[257], ll[258] = 1, 2, 3, 3
    toks = [65] * 64 + [(3, 33), (4, 48), (3, 49), (4, 64)]
    p = W.Payload().dynamic(toks, ll, [0] * 10 + [1, 1], True, rle=W.rle_items(ll[:259], "greedy") + [(18, 23), (1, 1), (1, 1)])
    valid("C_18_across_hlit", p, toks)
    toks = W.random_tokens(rng, 2000, list(range(256)), list(range(29)), list(range(30)))
    valid("C_header316", _header316(W.Payload(), rng, toks, True), toks)

    # ---- D. where things start
    for off in HEADER_OFFSETS:
        rng = R(4000 + off)
        head = rng.randbytes(off - 5)
        toks = W.random_tokens(rng, 300, rng.sample(range(256), 12), rng.sample(range(29), 10), rng.sample(range(30), 12), start=len(head))
        p = W.random_dynamic(W.Payload().stored(head, False), rng, toks, True)
        assert p.blocks[1]["bit"] == 8 * off
        valid("D_stored_then_dynamic_at_%d" % off, p, head + W.expand(list(head) + toks)[len(head):])
    for off in HEADER316_OFFSETS:
        rng = R(4300 + off)
        head = rng.randbytes(off - 5)
        toks = W.random_tokens(rng, 600, list(range(256)), list(range(29)), list(range(30)), start=len(head))
        p = _header316(W.Payload().stored(head, False), rng, toks, True)
        assert p.blocks[1]["bit"] == 8 * off
        valid("D_stored_then_header316_at_%d" % off, p, head + W.expand(list(head) + toks)[len(head):])
    # (behind a stored block the window is loaded anew; behind a CODED block it is not, and the header lies across the reload mark)
    for off in HEADER_OFFSETS:
        rng = R(4400 + off)
        first = _lits(rng, off - 1, range(144))                      # 3 + 8 n + 7 bits: the next block begins in byte n + 1
        toks = W.random_tokens(rng, 600, list(range(256)), list(range(29)), list(range(30)), start=len(first))
        p = _header316(W.Payload().fixed(first, False), rng, toks, True)
        assert p.blocks[1]["bit"] // 8 == off
        valid("D_fixed_then_header316_at_%d" % off, p, first + toks)
    rng = R(4500)

    def block(p, kind, toks, final):
        if kind == "stored":
            return p.stored(W.expand(toks), final)
        return p.fixed(toks, final) if kind == "fixed" else W.random_dynamic(p, rng, toks, final)

    for a in ("stored", "fixed", "dynamic"):
        for b in ("stored", "fixed", "dynamic"):
            one = _lits(rng, 120, range(60, 90))
            two = _lits(rng, 40, range(60, 90)) + ([] if b == "stored" else [(30, 150), (12, 12), (100, 1)]) + _lits(rng, 9, range(60, 90))
            text = W.expand(one + two)
            p = block(W.Payload(), a, one, False)
            p = p.stored(text[len(one):], True) if b == "stored" else block(p, b, two, True)
            valid("D_%s_then_%s" % (a, b), p, text)
    for kind in ("stored", "fixed", "dynamic"):
        p, toks = W.Payload(), _lits(rng, 70) + [(20, 33)]
        for _ in range(3):
            if kind == "dynamic":
                p.dynamic([], [0] * 256 + [1], [0], False)
            else:
                block(p, kind, [], False)
        valid("D_three_empty_%s_then_data" % kind, p.fixed(toks, True), toks)
    phases = set()
    for k in range(8):
        first = [200] * k + [65, 66]                                 # 3 + 9 k + 16 + 7 bits
        p = W.Payload().fixed(first, False)
        phases.add(p.w.bitpos % 8)
        data = rng.randbytes(33)
        valid("D_stored_after_%d_bits" % (p.w.bitpos % 8), p.stored(data, True), bytes(first) + data)
    assert phases == set(range(8))
    head = rng.randbytes(100)
    for name, toks in (("wholly_in", _lits(rng, 10) + [(20, 60), (20, 110)]), ("straddles", _lits(rng, 10) + [(20, 20), (64, 105)]),
                       ("overlaps_from", [(30, 5), (258, 100)])):
        valid("D_match_%s_stored" % name, W.Payload().stored(head, False).fixed(toks, True), head + W.expand(list(head) + toks)[100:])
    data = R(4600).randbytes(65505)
    p = W.Payload().stored(data, True)
    assert len(p.getvalue()) == W.MAX_PAYLOAD
    valid("D_largest_stored", p, data)
    rng = R(4601)
    toks = _lits(rng, 32742, range(144)) + _lits(rng, 29126, range(144, 256))      # 3 + 8 a + 9 b + 7 bits = 8 x 65510
    rng.shuffle(toks)
    p = W.Payload().fixed(toks, True)
    assert len(p.getvalue()) == W.MAX_PAYLOAD and p.w.n == 0
    valid("D_largest_fixed", p, toks)

    # ---- E. the copy rule and the queue
    for d in range(1, 67):
        rng = R(5000 + d)
        toks = _lits(rng, d) + [(258, d), rng.randrange(256), (258, d)]
        valid("E_overlap_258_at_%d" % d, W.Payload().fixed(toks, True), toks)
    rng = R(5100)
    toks, prev = _lits(rng, 40), 40
    for _ in range(200):
        n = rng.randint(3, 258)
        toks.append((n, prev))
        prev = n
    valid("E_chain_of_200", W.Payload().fixed(toks, True), toks)
    for n in (3, 258):
        valid("E_literal_then_distance1_len%d" % n, W.Payload().fixed([90, (n, 1)], True), [90, (n, 1)])
    for lead in (126, 127, 128):
        # tokens `lead` and `lead + 1` (counted from 0) are a match and a match of its output; a queue holds tokens 0..127
        toks = _lits(rng, lead, range(144)) + [(10, 50), (10, 10), 66, (4, 1)]
        p = W.Payload().fixed(toks, True)
        assert p.blocks[0]["end_bit"] < 8 * 240                       # (one window: nothing but the token count ends a queue)
        valid("E_dependent_pair_after_%d" % lead, p, toks)
        toks = _lits(rng, lead + 1, range(144)) + [(9, 1), 67, (9, 10)]
        valid("E_literal_then_match_after_%d" % lead, W.Payload().fixed(toks, True), toks)
    for delta in (-1, 0, 1):
        # M1 = (20, 30) at p1 = 40; M2 follows with distance >= length and its source ending at p1 + delta
        toks = _lits(rng, 40) + [(20, 30), (8, 28 - delta), 1, 2, (8, 3)]
        p = W.Payload().fixed(toks, True)
        (_, _, p1, _, _), (_, _, p2, l2, d2) = p.blocks[0]["matches"][:2]
        assert d2 >= l2 and p2 - d2 + l2 == p1 + delta
        valid("E_source_ends_%+d_of_previous_match" % delta, p, toks)

    # ---- F. ISIZE and the CRC's slices
    rng = R(6000)
    span, text, blocks = [], [], []
    for n in range(201):
        toks = W.random_tokens(rng, n, rng.sample(range(256), 5), [0, 1, 2, 5, 9], [0, 1, 3, 6, 8])
        raw = W.expand(toks)
        p = W.Payload()
        p = p.stored(raw, True) if n % 3 == 0 else p.fixed(toks, True) if n % 3 == 1 else W.random_dynamic(p, rng, toks, True)
        assert zlib_inflates_to(p.getvalue(), raw) and len(raw) == n
        span.append(member(raw, p.getvalue())); text.append(raw); blocks.append(p.blocks)
    out.append(("F_isize_0_to_200", b"".join(span), b"".join(text), None))
    info["F_isize_0_to_200"] = blocks
    for n in (4095, 4096, 4097, 65535, 65536):
        rng = R(6000 + n)
        toks = W.random_tokens(rng, n, rng.sample(range(256), 30), list(range(29)), list(range(30)))
        valid("F_isize_%d" % n, W.Payload().fixed(toks, True), toks)

    # ---- G. random valid members
    for seed in G_SEEDS:
        p, toks = _g_member(R(7000 + seed))
        if len(p.getvalue()) > W.MAX_PAYLOAD:                          # (more than BSIZE can state)
            continue
        valid("G_seed_%03d" % seed, p, toks)

    # G's members once more, over a text the parser reads: a FASTQ file in pieces, each as literals and random back-references
    text, span, blocks, at = open(FASTQ, "rb").read(), [], [], 0
    sizes = R(7900)
    while at < len(text):
        chunk = text[at:at + sizes.choice([50, 300, 3000])]
        rng = R(7000 + len(span))
        p, _ = _g_member(rng, W.tokens_of_text(rng, chunk))
        assert zlib_inflates_to(p.getvalue(), chunk) and len(p.getvalue()) <= W.MAX_PAYLOAD
        span.append(member(chunk, p.getvalue())); blocks.append(p.blocks)
        at += len(chunk)
    out.append(("G_over_fastq", b"".join(span), text, None))
    info["G_over_fastq"] = blocks

    # ---- H. malformed by construction: member 1 of three
    rng = R(8000)
    good = [c[1] for c in out if c[0] in ("E_overlap_258_at_7", "C_16_across_hlit", "D_fixed_then_dynamic")]
    assert len(good) == 3

    def bad(name, p, raw, status, isize=None, crc=None, judge="zlib"):
        """raw: the text up to where the member goes wrong (what ISIZE and CRC state unless given)"""
        raw = W.expand(raw) if isinstance(raw, list) else bytes(raw)
        payload = p if isinstance(p, bytes) else p.getvalue()
        assert len(payload) <= W.MAX_PAYLOAD, name
        m = member(raw, payload)
        if isize is not None:
            m = edit_member(m, isize=isize)
        assert zlib_rejects_payload(payload) if judge == "zlib" else (gzip_rejects(m) and not zlib_rejects_payload(payload)), name
        out.append((name, good[0] + m + good[2], None, (status, 1)))
        return m

    ten = _lits(rng, 10)
    for s in (286, 287):
        bad("H_fixed_litlen_symbol_%d" % s, W.Payload().fixed(ten + [("L", s)] + ten, True), ten, SYMBOL)
    for s in (30, 31):
        bad("H_fixed_distance_symbol_%d" % s, W.Payload().fixed(ten + [("L", 257), ("D", s)] + ten, True), ten, SYMBOL)
    ll = W.code_for(rng, set(ten) | {256, 257}, 258)
    bad("H_match_without_distance_code", W.Payload().dynamic(ten + [("L", 257)] + ten, ll, [0], True), ten, SYMBOL)
    bad("H_unused_code_of_one_distance_code", W.Payload().dynamic(ten + [("L", 257), ("B", 1, 1)] + ten, ll, [1], True), ten, SYMBOL)
    tail = bytes(40)                                                   # (something behind a header that is refused)
    for n in (287, 288):
        p = W.Payload().dynamic([], W.code_for(rng, set(ten) | {256}, 257) + [0] * (n - 257), [1, 1], True, body=False, check=False)
        bad("H_hlit_%d" % n, p.getvalue() + tail, b"", CODE_LENGTHS)
    for n in (31, 32):
        p = W.Payload().dynamic([], W.code_for(rng, set(ten) | {256}, 257), [1, 1] + [0] * (n - 2), True, body=False, check=False)
        bad("H_hdist_%d" % n, p.getvalue() + tail, b"", CODE_LENGTHS)
    ll = [0] * 257
    ll[0] = ll[1] = ll[2] = ll[256] = 2
    seq = W.rle_items(ll + [1, 1], "greedy")
    assert seq[0] == (2, 1) and seq[-3:] == [(2, 1), (1, 1), (1, 1)]
    cl = [0] * 19
    for s, n in ((0, 2), (1, 2), (2, 3), (16, 3), (17, 3), (18, 3)):
        cl[s] = n
    assert W.kraft(cl) == 32768

    def header(items, cl_lengths=cl, ll_=ll, dl=(1, 1)):
        return W.Payload().dynamic([], ll_, list(dl), True, cl_lengths=cl_lengths, rle=items, body=False, check=False).getvalue() + tail

    assert not zlib_rejects_payload(W.Payload().dynamic([0, 1, 2], ll, [1, 1], True, cl_lengths=cl, rle=seq).getvalue())
    bad("H_first_length_is_16", header([(16, 3)] + seq[1:]), b"", CODE_LENGTHS)
    bad("H_16_past_the_end", header(seq[:-1] + [(16, 4)]), b"", CODE_LENGTHS)
    bad("H_17_past_the_end", header(seq[:-2] + [(17, 3)]), b"", CODE_LENGTHS)
    bad("H_18_past_the_end", header(seq[:-3] + [(0, 1), (18, 11)]), b"", CODE_LENGTHS)
    no256 = [2, 2, 2, 2] + [0] * 253
    bad("H_no_code_for_256", header(W.rle_items(no256 + [1, 1], "greedy"), ll_=no256), b"", CODE_LENGTHS)
    cl4 = [0] * 19
    cl4[0] = cl4[18] = 1
    p = W.Payload().dynamic([], [0] * 257, [0], True, cl_lengths=cl4, hclen=4, rle="greedy", body=False, check=False)
    assert p.blocks[0]["hclen"] == 4
    bad("H_hclen4_has_no_code_for_256", p.getvalue() + tail, b"", CODE_LENGTHS)
    over = [1, 1, 1] + [0] * 253 + [2]
    bad("H_litlen_oversubscribed", header(W.rle_items(over + [1, 1], "greedy"), ll_=over), b"", CODE_LENGTHS)
    bad("H_distance_oversubscribed", header(W.rle_items(ll + [1, 1, 1], "greedy"), dl=(1, 1, 1)), b"", CODE_LENGTHS)
    two = [2] + [0] * 255 + [2]
    bad("H_litlen_incomplete_two_codes", header(W.rle_items(two + [1, 1], "greedy"), ll_=two), b"", CODE_LENGTHS)
    bad("H_distance_incomplete_two_codes", header(W.rle_items(ll + [2, 2], "greedy"), dl=(2, 2)), b"", CODE_LENGTHS)
    cli = list(cl); cli[18] = 0; cli[17] = 4
    bad("H_code_length_code_incomplete", header(W.rle_items(ll + [1, 1], "none"), cl_lengths=cli), b"", CODE_LENGTHS)
    w = W.BitWriter(); w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(15, 4); w.bits(0, 57)
    bad("H_code_length_code_all_zero", w.getvalue() + tail, b"", CODE_LENGTHS)
    # a distance one beyond the member's first byte, in the second block.  (RFC 1951 has no distance above 32768, so the
    # deepest place is 32767 bytes in, not the issue's 40 000: a distance of 40 001 cannot be written)
    for n in (1, 100, 32767):
        first = rng.randbytes(n)
        di, de = W.distance_symbol(n + 1)
        p = W.Payload().stored(first, False).fixed([("L", 257), ("D", di, de)] + ten, True)
        bad("H_distance_%d_bytes_in" % n, p, first, DISTANCE)
    toks = _lits(rng, 30)
    bad("H_literal_at_isize", W.Payload().fixed(toks, True), toks[:29], OVERRUN, judge="gzip")
    toks = _lits(rng, 30) + [(40, 7)]
    bad("H_match_crosses_isize", W.Payload().fixed(toks, True), W.expand(toks)[:69], OVERRUN, judge="gzip")
    data = rng.randbytes(50)
    bad("H_stored_crosses_isize", W.Payload().fixed(ten, False).stored(data, True), (bytes(ten) + data)[:59], OVERRUN, judge="gzip")
    bad("H_stored_len_beyond_payload", W.Payload().stored(data, True, length=51), data, TRUNCATED)
    bad("H_ends_after_non_final_block", W.Payload().fixed(toks, False), toks, TRUNCATED)
    bad("H_text_short_of_isize", W.Payload().fixed(toks, True), toks, SHORT, isize=W.text_len(toks) + 1, judge="gzip")
    bad("H_trailing_1", W.Payload().fixed(toks, True).getvalue() + b"\x00", toks, TRAILING)
    bad("H_trailing_300", W.Payload().fixed(toks, True).getvalue() + rng.randbytes(300), toks, TRAILING)
    # every proper prefix of a dynamic and of a fixed member's payload
    toks = W.random_tokens(rng, 420, rng.sample(range(256), 14), [0, 3, 9, 14, 20], [0, 2, 5, 9, 12])
    cut_info = {}
    for kind, p in (("dynamic", W.random_dynamic(W.Payload(), rng, toks, True)), ("fixed", W.Payload().fixed(toks, True))):
        payload, raw = p.getvalue(), W.expand(toks)
        assert 60 <= len(payload) <= 200 and zlib_inflates_to(payload, raw), (kind, len(payload))
        cut_info[kind] = (len(payload), p.blocks)
        for n in range(len(payload)):
            bad("H_%s_cut_at_%03d" % (kind, n), payload[:n], raw, TRUNCATED)
    info["H_cuts"] = cut_info
    # two bad members in a span of eight: the EARLIER one is reported, though the later one's code is the smaller
    eight = [c[1] for c in out if c[0].startswith("E_overlap_258_at_")][:8]
    toks = _lits(rng, 30)
    trailing = member(W.expand(toks), W.Payload().fixed(toks, True).getvalue() + b"\x00")
    symbol = member(bytes(ten), W.Payload().fixed(ten + [("L", 286)], True).getvalue())
    overrun = edit_member(member(W.expand(toks), W.Payload().fixed(toks, True).getvalue()), isize=29)
    truncated = member(W.expand(toks), W.Payload().fixed(toks, False).getvalue())
    for name, (m2, c2), (m5, c5) in (("H_two_bad_trailing_then_symbol", (trailing, TRAILING), (symbol, SYMBOL)),
                                     ("H_two_bad_overrun_then_truncated", (overrun, OVERRUN), (truncated, TRUNCATED))):
        assert c5 < c2 and gzip_rejects(m2) and gzip_rejects(m5)
        out.append((name, b"".join(eight[:2] + [m2] + eight[3:5] + [m5] + eight[6:]), None, (c2, 2)))

    names = [c[0] for c in out]
    assert len(set(names)) == len(names) and not set(names) & {c[0] for c in cases()}
    return tuple(out), info


def built_cases():
    """as cases(), of members made by construction (tests/deflate_writer.py): groups A..G valid, a member per span but
    F_isize_0_to_200; group H malformed.  The group is the name's first letter."""
    return _built()[0]


def built_info():
    """name -> per member, the writer's record of the blocks it wrote (what test_built_corpus_covers_what_it_claims walks)"""
    return _built()[1]


def all_cases():
    return cases() + built_cases()


def write_corpus(directory, only=None):
    for name, span, raw, status in all_cases():
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

