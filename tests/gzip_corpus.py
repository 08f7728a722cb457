"""The corpus of PLAIN gzip files (one long deflate stream per member, no BC subfield) that tests/test_gzip_corpus_cpu.py and
tests/test_gpu_gunzip.py share: the smallest streams at which each part of the chunked inflater of csrc/kasa_gunzip.h can go
wrong.  Two sources: zlib streams (cut by Z_FULL_FLUSH / Z_SYNC_FLUSH every few hundred bytes, or as gzip.compress writes
them), whose block starts a small inflater written here (block_starts) lists, and streams built block by block with
tests/deflate_writer.py, whose block starts are known by construction.  All randomness is random.Random(seed) with the seeds
written here; nothing is read from a fixture but the golden inputs.

A case is a Case: name, group ("a".."h" of the list below), gz (the file), raw (its text) or status = (KASA_INFLATE_* code,
member index) of a file that has to be rejected, and for a single-member valid file data_at (where the deflate data begin)
and starts = [(bit in the file, block kind, text bytes before it)] of EVERY block.

  a  many dynamic blocks; a chunk's block start at each of the 8 bit alignments, on the first and on the last bit of a chunk
  b  back-references across a chunk start: distance 1 x 258, distance 32768, a match of markers, > 64 KiB through two windows
  c  only fixed and stored blocks: no candidate
  d  a stored block that holds a valid dynamic block: a false candidate that a chunk finds first
  e  200 000 bytes of one byte value: far above any capacity guess
  f  several members: an empty one, a header with FEXTRA / FNAME / FCOMMENT / FHCRC
  g  malformed files, each an edit of a valid one
  h  the golden inputs through gzip.compress at levels 1, 6 and 9"""
import collections
import functools
import gzip
import os
import random
import re
import struct
import subprocess
import zlib

from kasa_amd import build as hipbuild
from tests import deflate_writer as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pairs")
# include/kasa_hip.h
HEADER, CUT, TRUNCATED, BTYPE, STORED_LEN, CODE_LENGTHS, SYMBOL, DISTANCE, OVERRUN, SHORT, TRAILING, CRC, GZIP_HEADER, SPAN = range(1, 15)
CHUNKS = (64, 256, 1024, 0)                       # kasa_gzip_inflate's chunkBytes in the tests; 0: the default
DEFAULT_CHUNK = 65536
STATS = ("chunks", "started", "confirmed", "rejected", "rounds", "markers", "reruns", "members")
PLAIN_HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"

Case = collections.namedtuple("Case", "name group gz raw status data_at starts")


def golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def member(raw, payload, header=PLAIN_HEADER):
    return header + payload + struct.pack("<II", zlib.crc32(raw), len(raw) & 0xFFFFFFFF)


def gzip_rejects(data):
    try:
        gzip.decompress(data)
    except (OSError, EOFError, zlib.error):
        return True
    return False


# ---- a small inflater that says where every block begins -------------------------------------------------------------------------
def _decoder(lengths):
    """{(code length, code): symbol} of a canonical code"""
    return {(n, c): s for s, (n, c) in enumerate(zip(lengths, W.canonical(lengths))) if n}


def block_starts(payload):
    """([(bit, kind, text bytes before the block)] of every block of a raw deflate stream, (end bit, text length))"""
    bits = int.from_bytes(payload, "little")
    at, n, out = 0, 0, []

    def take(k):
        nonlocal at
        v = (bits >> at) & ((1 << k) - 1)
        at += k
        return v

    def sym(table):
        code, k = 0, 0
        while True:
            code = code << 1 | take(1)
            k += 1
            if (k, code) in table:
                return table[(k, code)]
            assert k < 16

    while True:
        start = at
        final, kind = take(1), take(2)
        out.append((start, ("stored", "fixed", "dynamic")[kind], n))
        if kind == 0:
            at = (at + 7) & ~7
            length = take(16)
            assert take(16) == length ^ 0xFFFF
            at += 8 * length
            n += length
        else:
            if kind == 1:
                lt, dt = _decoder(W.FIXED_L), _decoder(W.FIXED_D)
            else:
                hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
                cl = [0] * 19
                for s in W.CL_ORDER[:hclen]:
                    cl[s] = take(3)
                ct, lens = _decoder(cl), []
                while len(lens) < hlit + hdist:
                    s = sym(ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + take(2))
                    elif s == 17:
                        lens += [0] * (3 + take(3))
                    else:
                        lens += [0] * (11 + take(7))
                lt, dt = _decoder(lens[:hlit]), _decoder(lens[hlit:hlit + hdist])
            while True:
                s = sym(lt)
                if s < 256:
                    n += 1
                elif s == 256:
                    break
                else:
                    n += W.LEN_BASE[s - 257] + take(W.LEN_EXTRA[s - 257])
                    d = sym(dt)
                    take(W.DIST_EXTRA[d])
        if final:
            return out, (at, n)


def _case(name, group, raw, payload, starts=None):
    """a single-member valid file with its block table: the writer's records (starts), or what block_starts reads"""
    assert zlib.decompress(payload, -15) == raw, name
    if starts is None:
        starts, (end, n) = block_starts(payload)
        assert n == len(raw) and (end + 7) // 8 == len(payload), name
    data_at = len(PLAIN_HEADER)
    return Case(name, group, member(raw, payload), raw, None, data_at, [(8 * data_at + bit, kind, before) for bit, kind, before in starts])


def _built(name, group, p, raw=None):
    payload = p.getvalue()
    return _case(name, group, zlib.decompress(payload, -15) if raw is None else raw, payload, [(b["bit"], b["kind"], b["text_at"]) for b in p.blocks])


def flushed(raw, every, flush, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    """(payload, the byte at which every piece begins): the block behind a flush begins on the first bit of that byte"""
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    parts = [z.compress(raw[a:a + every]) + z.flush(flush) for a in range(0, len(raw), every)]
    parts.append(z.flush())
    return b"".join(parts), [sum(map(len, parts[:k])) for k in range(len(parts))]


def expected_confirmed(case, chunk):
    """the chunks (of `chunk` compressed bytes from the deflate data's first) that hold a dynamic block's start, and the first
    chunk, whose start is known: what the chain has to confirm when no chunk finds a chance candidate first"""
    chunk = chunk or DEFAULT_CHUNK
    return len({0} | {(bit // 8 - case.data_at) // chunk for bit, kind, _ in case.starts if kind == "dynamic"})


def check_stats(case, chunk, st):
    """what the chunk statistics of a run over a valid case have to say: st is the host check's line or kasa_gzip_inflate's
    stats8, by the names of STATS.  The condition on `confirmed` keeps a run from passing with everything decoded serially."""
    if case.raw is None:
        return
    size = chunk or DEFAULT_CHUNK
    assert st["confirmed"] <= st["started"] <= st["chunks"] and st["rounds"] >= 1, st
    if case.starts:
        assert st["members"] == 1 and st["chunks"] == max(1, -(-(len(case.gz) - case.data_at) // size)), st
    if case.group in "abh":
        assert st["confirmed"] == expected_confirmed(case, chunk) and st["rejected"] == 0 and st["rounds"] == 1, (st, expected_confirmed(case, chunk))
    if case.group == "b" and chunk:
        assert st["markers"] > 0, st
    if case.group == "c":
        assert st["confirmed"] == 1 and st["started"] == 1, st
    if case.group == "d":
        assert st["rejected"] >= 1 and st["rounds"] >= 2, st
    if case.group == "e":
        assert st["confirmed"] == 1 and st["reruns"] >= 1, st
    if case.name == "f_members":
        assert st["members"] == 5 and st["confirmed"] == 5, st


# ---- the writer's helpers ----------------------------------------------------------------------------------------------------------
def pad_to(p, target):
    """a stored block of zeros and a fixed block of literals, so that the NEXT block begins at bit `target` of the payload"""
    e = (target - 10 - 56) // 8                                      # the byte behind the stored block
    r = target - 10 - 8 * e                                          # 56..63 bits of literals: (7 - b) of 8 bits and b of 9
    room = e - ((p.w.bitpos + 3 + 7) // 8 + 4)
    assert room >= 0, "the target lies too close"
    p.stored(bytes(room), 0)
    assert p.w.bitpos == 8 * e
    b = r - 56
    p.fixed([65] * (7 - b) + [200] * b, 0)
    assert p.w.bitpos == target, (p.w.bitpos, target)


def literals(rng, n):
    return [rng.randrange(256) for _ in range(n)]


def flat_literal_block(p, data, final):
    """a dynamic block of literals in a flat code: 8 bits each for the bytes 0..254 (and 9 for 255 and the end of the block)"""
    assert 255 not in data
    p.dynamic(list(data), W.flat_code(257), [1], final)


# ---- the groups --------------------------------------------------------------------------------------------------------------------
A_SEED, B_SEED, C_SEED, D_SEED, F_SEED, G_SEED = 20, 31, 37, 41, 53, 61
# where (a)'s built blocks begin, in bits behind the stream's first: every alignment, the first and the last bit of chunks of
# 64, 256 and 1024 bytes, and two starts in one chunk
A_OFFSETS = (512 * 3, 512 * 6 + 511, 512 * 10 + 1, 512 * 13 + 2, 512 * 16 + 3, 512 * 19 + 4, 512 * 22 + 5, 512 * 25 + 6, 512 * 28 + 7,
             2048 * 8, 2048 * 9 + 2047, 8192 * 3, 8192 * 4 + 8191, 8192 * 6 + 600, 8192 * 6 + 1900)


def group_a():
    text = golden("reads.fastq")
    out = []
    # (behind a sync flush the history stays: blocks of 300 bytes would mostly take the fixed code)
    for name, flush, every in (("full", zlib.Z_FULL_FLUSH, 300), ("sync", zlib.Z_SYNC_FLUSH, 1000)):
        payload, pieces = flushed(text, every, flush)
        c = _case("a_flush_%s_%d" % (name, every), "a", text, payload)
        assert {8 * (c.data_at + b) for b in pieces[:-1]} <= {s[0] for s in c.starts}          # the pieces' sizes say the same
        out.append(c)
    rng = random.Random(A_SEED)
    p = W.Payload()
    for k, target in enumerate((0,) + A_OFFSETS):
        if k:
            pad_to(p, target)
        piece = text[60 * k:60 * k + 60]                              # some 60 bytes of deflate data a block
        W.random_dynamic(p, rng, W.tokens_of_text(rng, piece, 0.6), k == len(A_OFFSETS))
    c = _built("a_alignments", "a", p)
    assert [s[0] - 8 * c.data_at for s in c.starts if s[1] == "dynamic"] == [0] + list(A_OFFSETS)
    out.append(c)
    return out


def group_b():
    out = []
    rng = random.Random(B_SEED)
    # 1: distance 1, length 258, the first token of a block in a later chunk (the run goes on from the block before)
    p = W.Payload()
    blocks = [literals(rng, 1300) + [(258, 1)], [(258, 1), (258, 1)] + literals(rng, 1300) + [(258, 1)], [(258, 1)] + literals(rng, 100)]
    for k, b in enumerate(blocks):
        W.random_dynamic(p, rng, b, k == len(blocks) - 1)
    out.append(_built("b_distance1_x258", "b", p, W.expand(sum(blocks, []))))
    # 2: distance 32768 exactly: the first byte of the window
    p = W.Payload()
    first = literals(rng, 1200)
    first += [(258, 1200)] * ((32768 - 1200) // 258)
    first += literals(rng, 32768 - W.text_len(first))
    blocks = [first, [(258, 32768), (3, 32768)] + literals(rng, 1200) + [(100, 32768)], [(258, 32768)] + literals(rng, 50)]
    for k, b in enumerate(blocks):
        W.random_dynamic(p, rng, b, k == len(blocks) - 1)
    out.append(_built("b_distance32768", "b", p, W.expand(sum(blocks, []))))
    # 3: a match whose source is a match into the chunk before: markers copied by a match, overlapping and not
    p = W.Payload()
    blocks = [literals(rng, 1300), [(10, 500), (10, 10), (30, 5), (258, 1)] + literals(rng, 1300) + [(200, 1400)], [(50, 258), (258, 50)] + literals(rng, 40)]
    for k, b in enumerate(blocks):
        W.random_dynamic(p, rng, b, k == len(blocks) - 1)
    out.append(_built("b_match_of_markers", "b", p, W.expand(sum(blocks, []))))
    # 4: more than 64 KiB of text: a chunk of less than 32 KiB of output passes part of its predecessor's window on, and a
    # marker is resolved through two windows (a match into a match into the chunk before that)
    p = W.Payload()
    one = literals(rng, 1300)
    one += [(258, 1300), (258, 999)] * ((40000 - 1300) // 516)
    two = [(100, 30000), (100, 100)] + literals(rng, 1300)           # 1500 bytes of output
    three = [(258, 1500 + 20000), (200, 258 + 1500), (258, 458 + 1500 + 30000)] + literals(rng, 1300)
    three += [(258, 1300), (258, 32768)] * ((36000 - W.text_len(three)) // 516)
    four = [(258, 32768), (258, 30000), (258, 258)] + literals(rng, 1300)
    blocks = [one, two, three, four]
    for k, b in enumerate(blocks):
        W.random_dynamic(p, rng, b, k == len(blocks) - 1)
    raw = W.expand(sum(blocks, []))
    assert len(raw) > 65536 + 4096
    out.append(_built("b_two_windows", "b", p, raw))
    return out


def group_c():
    text = golden("reads.fastq")[:6000]
    payload, _ = flushed(text, 500, zlib.Z_FULL_FLUSH, strategy=zlib.Z_FIXED)
    c = _case("c_fixed_and_stored", "c", text, payload)
    assert {s[1] for s in c.starts} == {"fixed", "stored"}
    rnd = bytes(random.Random(C_SEED).randrange(256) for _ in range(3000))
    payload = zlib.compressobj(0, zlib.DEFLATED, -15)
    payload = payload.compress(rnd) + payload.flush()
    return [c, _case("c_stored", "c", rnd, payload)]


D_FALSE_AT = 65536 + 8                            # the byte of the deflate data at which the false block header stands


def group_d():
    """[one dynamic block that ends just behind byte 65536][stored: a whole dynamic block as DATA][fixed][dynamic][dynamic].
    For chunks of 64, 256, 1024 and 65536 bytes alike, the chunk that begins at byte 65536 finds the stored block's data
    first: its predecessor passes over that candidate, ends behind the stored block where no candidate stands (the fixed
    block), and decodes on in a second round."""
    rng = random.Random(D_SEED)
    inner = W.Payload()
    W.random_dynamic(inner, rng, W.tokens_of_text(rng, golden("reads.fastq")[:400], 0.6), 0)
    false_block = inner.getvalue()
    n = 65000
    for _ in range(3):
        p = W.Payload()
        flat_literal_block(p, [rng.randrange(255) for _ in range(n)], 0)
        # the stored block's data begin 3 bits, the padding and 4 bytes behind the block's end
        at = (p.w.bitpos + 3 + 7) // 8 + 4
        if at == D_FALSE_AT:
            break
        n += D_FALSE_AT - at
    assert at == D_FALSE_AT
    p.stored(false_block, 0)
    p.fixed(list(b"a fixed block: no candidate stands here") * 3, 0)
    W.random_dynamic(p, rng, W.tokens_of_text(rng, golden("reads.fastq")[400:2400], 0.6), 0)
    W.random_dynamic(p, rng, literals(rng, 300) + [(258, 66000 % 32768)], 1)
    c = _built("d_false_candidate", "d", p)
    assert c.gz[c.data_at + D_FALSE_AT:][:len(false_block)] == false_block
    return [c]


def group_e():
    raw = b"A" * 200000
    z = zlib.compressobj(9, zlib.DEFLATED, -15)
    payload = z.compress(raw) + z.flush()
    assert len(payload) < 300
    return [_case("e_one_byte_200000", "e", raw, payload)]


def rich_header(extra=b"KA\x03\x00abc", name=b"reads.fastq", comment=b"a comment"):
    """FEXTRA (a subfield that is not BC), FNAME, FCOMMENT and FHCRC"""
    h = b"\x1f\x8b\x08" + bytes([2 | 4 | 8 | 16]) + b"\x00\x00\x00\x00\x00\x03" + struct.pack("<H", len(extra)) + extra + name + b"\x00" + comment + b"\x00"
    return h + struct.pack("<H", zlib.crc32(h) & 0xFFFF)


def group_f():
    text = golden("reads.fastq")
    t1, t2, t3 = text[:5000], text[5000:9000], text[9000:12000]
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    m2 = member(t2, z.compress(t2) + z.flush(), rich_header())
    gz = gzip.compress(t1, 6) + gzip.compress(b"") + m2 + gzip.compress(t3, 1) + gzip.compress(b"")
    assert gzip.decompress(gz) == t1 + t2 + t3
    out = [Case("f_members", "f", gz, t1 + t2 + t3, None, None, None),
           Case("f_empty_member_alone", "f", gzip.compress(b""), b"", None, None, None)]
    # a back-reference that would reach into the member before: a status, in the member's first chunk and in a later one
    rng = random.Random(F_SEED)
    p = W.Payload()
    p.fixed([65, 66, ("L", 257), ("D", 2)], 1)                        # length 3 at distance 3, two bytes in
    bad = PLAIN_HEADER + p.getvalue() + struct.pack("<II", 0, 5)
    out.append(Case("f_distance_into_member_before", "f", gzip.compress(t1, 6) + bad, None, (DISTANCE, 1), None, None))
    p = W.Payload()
    W.random_dynamic(p, rng, literals(rng, 1300), 0)
    W.random_dynamic(p, rng, [("L", 257), ("D", 21, 500)] + literals(rng, 30), 1)          # distance 1537 + 500 at 1300 bytes
    bad = PLAIN_HEADER + p.getvalue() + struct.pack("<II", 0, 1333)
    out.append(Case("f_distance_into_member_before_later_chunk", "f", gzip.compress(t1, 6) + bad, None, (DISTANCE, 1), None, None))
    return out


def _set_bits(buf, at, n, value):
    for i in range(n):
        byte, bit = (at + i) >> 3, (at + i) & 7
        buf[byte] = (buf[byte] & ~(1 << bit)) | (((value >> i) & 1) << bit)


def group_g():
    text = golden("reads.fastq")[:9000]
    payload, pieces = flushed(text, 1500, zlib.Z_SYNC_FLUSH)
    good = member(text, payload)
    assert gzip.decompress(good) == text
    crc, isize = struct.unpack("<II", good[-8:])
    out = []

    def bad(name, data, code, at=0):
        assert gzip_rejects(data), name
        out.append(Case("g_" + name, "g", data, None, (code, at), None, None))

    bad("crc", good[:-8] + struct.pack("<II", crc ^ 0x10000, isize), CRC)
    bad("isize_larger", good[:-4] + struct.pack("<I", isize + 1), SHORT)
    bad("isize_smaller", good[:-4] + struct.pack("<I", isize - 1), OVERRUN)
    bad("cut_in_first_block", good[:10 + pieces[1] // 2], TRUNCATED)
    bad("cut_in_later_block", good[:10 + (pieces[3] + pieces[4]) // 2], TRUNCATED)
    bad("cut_behind_a_block", good[:10 + pieces[3]], TRUNCATED)
    bad("cut_in_trailer", good[:-3], CUT)
    bad("cut_before_trailer", good[:-8], CUT)
    for k in (0, 3):
        b = bytearray(good)
        _set_bits(b, 8 * (10 + pieces[k]) + 1, 2, 3)
        bad("btype3_block%d" % k, bytes(b), BTYPE)
    p = W.Payload()
    p.fixed([65, ("L", 257), ("D", 1)], 1)                            # distance 2, one byte in
    bad("distance_before_first_byte", PLAIN_HEADER + p.getvalue() + struct.pack("<II", 0, 4), DISTANCE)
    bad("trailing_garbage", good + b"garbage that is no member header", GZIP_HEADER, 1)
    bad("trailing_one_byte", good + b"\x1f", CUT, 1)
    bad("no_gzip_at_all", text[:200], GZIP_HEADER)
    bad("header_cut", good[:7], CUT)
    return out


def group_h():
    out = []
    for name in ("reads.fastq", "edge_crlf.fasta", "edge_noeol.fasta", "reads.fasta"):
        raw = golden(name)
        for level in (1, 6, 9):
            gz = gzip.compress(raw, level)
            c = _case("h_%s_level%d" % (name.replace(".", "_"), level), "h", raw, gz[10:-8])
            out.append(c._replace(gz=gz))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = group_a() + group_b() + group_c() + group_d() + group_e() + group_f() + group_g() + group_h()
    assert len({c.name for c in out}) == len(out)
    return out


def write_corpus(path):
    os.makedirs(path, exist_ok=True)
    for c in cases():
        with open(os.path.join(path, c.name + ".gz"), "wb") as f:
            f.write(c.gz)
        if c.raw is not None:
            with open(os.path.join(path, c.name + ".raw"), "wb") as f:
                f.write(c.raw)
        else:
            with open(os.path.join(path, c.name + ".status"), "w") as f:
                f.write("%d %d\n" % c.status)


_HOST = {}
_LINE = re.compile(r"^(\S+) @(\d+): status (\d+), (\d+) bytes; " + " ".join(r"%s (\d+)" % s for s in STATS) + r"(  MISMATCH)?$")


def host_check(tmp_dir):
    """tools/gunzip_host_check (AddressSanitizer + UBSan) over the whole corpus at every chunk size of CHUNKS, once per
    session: runs[(name, chunk)] = dict(status, bytes, ok and the chunk statistics), and the program's exit code and output."""
    if not _HOST:
        exe = hipbuild.build_gunzip_check()
        write_corpus(tmp_dir)
        r = subprocess.run([exe, tmp_dir] + [str(c) for c in CHUNKS], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        runs = {}
        for line in r.stdout.splitlines():
            m = _LINE.match(line)
            if m:
                v = dict(zip(("status", "bytes") + STATS, map(int, m.groups()[2:12])))
                v["ok"] = m.group(13) is None
                runs[(m.group(1), int(m.group(2)))] = v
        _HOST.update(runs=runs, returncode=r.returncode, output=r.stdout)
    return _HOST
