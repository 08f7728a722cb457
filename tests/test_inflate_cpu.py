"""The device inflater without a device: formats.bgzf_member_table / record_cut (the member walk and the two cut rules of
kasa_bgzf_parse_append, stated in Python) on hand-made input, and the decoder body of csrc/kasa_inflate.h -- the very
functions inflate_kernel runs -- compiled for the CPU under AddressSanitizer + UBSan (tools/inflate_host_check, a stand-alone
program) over the corpus of tests/inflate_corpus.py: every span gives its bytes or its status, and the run ends clean.

One case of the issue's list cannot exist: a STORED member of ISIZE 65536 needs 65536 + 10 + 26 bytes, more than BSIZE can
state.  The corpus has its two properties apart: `isize65536` (a coded member of the largest ISIZE) and `stored_two_blocks`."""
import gzip
import re
import zlib

import pytest

from kasa_amd import build as hipbuild, capi, formats
from tests import inflate_corpus as corpus


# ---- (a) the member walk and the cut rules ------------------------------------------------------------------------------------
def test_member_table_walks_by_bsize():
    data = bytes(range(256)) * 20
    ms = corpus.members(data, block=1000, level=6)
    stream = b"".join(ms[:3]) + formats.BGZF_EOF + b"".join(ms[3:])
    rows, consumed, status = formats.bgzf_member_table(stream)
    assert (consumed, status) == (len(stream), 0) and len(rows) == len(ms) + 1
    at = text = 0
    for (off, length, poff, plen, crc, isize, toff), (head, payload, c, n) in zip(rows, formats.bgzf_members(stream)):
        assert (off, length) == (at, head["length"]) and stream[poff:poff + plen] == payload and (crc, isize) == (c, n) and toff == text
        piece = zlib.decompress(payload, -15)
        assert len(piece) == isize and zlib.crc32(piece) == crc and data[toff:toff + isize] == piece
        at += length
        text += isize
    assert rows[3][5] == 0 and rows[3][3] == 2                      # the EOF member in the middle: no text, two bytes of deflate
    assert text == len(data)


@pytest.mark.parametrize("cut", [1, 4, 10, 11, 16, 17, 18, 25, 40, 1000])
def test_member_table_span_that_ends_inside_a_member(cut):
    ms = corpus.members(corpus.INPUTS["random70000"][:2000], block=1000, level=6)
    assert len(ms[1]) > 1000
    rows, consumed, status = formats.bgzf_member_table(ms[0] + ms[1][:cut])
    assert status == 0 and consumed == len(ms[0]) and len(rows) == 1


def test_member_table_refuses_what_is_not_bgzf():
    ms = corpus.members(b"kasa" * 500, block=1000, level=6)
    plain = gzip.compress(b"one long stream has no BC subfield")
    assert formats.bgzf_member_table(plain)[1:] == (0, 1)
    assert formats.bgzf_member_table(ms[0] + plain)[1:] == (len(ms[0]), 1)
    assert formats.bgzf_member_table(ms[0] + b"\x1f\x8b\x08")[1:] == (len(ms[0]), 0)          # may still become a header
    assert formats.bgzf_member_table(ms[0] + b"\x1f\x8b\x09")[1:] == (len(ms[0]), 1)
    too_big = corpus.edit_member(ms[1], isize=65537)
    assert formats.bgzf_member_table(ms[0] + too_big)[1:] == (len(ms[0]), 1)
    short = bytearray(ms[1]); short[16:18] = (24).to_bytes(2, "little")                        # BSIZE 24: 25 bytes cannot hold header and trailer
    assert formats.bgzf_member_table(ms[0] + bytes(short))[1:] == (len(ms[0]), 1)


def test_cut_fastq_quality_line_that_starts_with_at():
    rec = b"@r0\nACGT\n+\n@III\n"
    text = rec + b"@r1\nAC\n+\n@@\n@r2\nAC"
    assert formats.record_cut(text, False) == len(rec) + 12          # behind r1; '@@' and '@III' begin no record
    assert formats.record_cut(rec + b"@r1\nAC\n+\n@@", False) == len(rec)          # the fourth line has no line feed yet
    assert formats.record_cut(rec[:-1], False) == 0
    assert formats.record_cut(rec, False) == len(rec)
    assert formats.record_cut(b"", False) == 0


def test_cut_crlf():
    rec = b"@r0\r\nACGT\r\n+\r\nIIII\r\n"
    assert formats.record_cut(rec + b"@r1\r\nAC\r", False) == len(rec)
    assert formats.record_cut(rec + rec[:-1], False) == len(rec)     # ...\r without its \n: not whole
    fa = b">a\r\nACGT\r\n>b\r\nAC\r\n"
    assert formats.record_cut(fa, True) == fa.index(b">b")


def test_cut_no_final_line_feed_with_final():
    text = b"@r0\nACGT\n+\nIIII\n@r1\nAC\n+\nII"
    assert formats.record_cut(text, False) == 16
    assert formats.record_cut(text, False, final=True) == len(text)
    assert formats.record_cut(b">a\nACGT\n>b\nAC", True, final=True) == 13 and formats.record_cut(b">a\nACGT\n>b\nAC", True) == 8


def test_cut_fasta_single_header_cuts_nothing():
    assert formats.record_cut(b">only one\nACGT\nACGT\nAC", True) == 0
    assert formats.record_cut(b">a\nAC>GT\n", True) == 0             # '>' inside a line begins none
    assert formats.record_cut(b">a\nAC\n\n>b\n", True) == 7
    assert formats.record_cut(b">a\nAC\n>b\nGG\n>", True) == 12      # a header of which only '>' is there yet


# ---- (b) the decoder body under the sanitizers ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return corpus.host_check(str(tmp_path_factory.mktemp("inflate_corpus")))


def test_corpus_is_what_it_says():
    """every valid span is gzip's to read; every malformed one was asserted against zlib / gzip where it was made"""
    cases = corpus.cases()
    for name, span, raw, status in cases:
        if raw is not None:
            assert gzip.decompress(span + formats.BGZF_EOF) == raw, name
        elif status[0] == corpus.HEADER:                                # (gzip takes a plain member among BGZF ones; the BGZF walk does not)
            with pytest.raises(ValueError):
                list(formats.bgzf_members(span))
        else:
            assert corpus.gzip_rejects(span), name
    kinds = {(m[18] >> 1) & 3 for name, span, raw, _ in cases if raw for m in [span]}
    assert kinds == {0, 1, 2}
    assert {s[0] for *_, s in cases if s} >= {corpus.CUT, corpus.TRUNCATED, corpus.BTYPE, corpus.STORED_LEN, corpus.CODE_LENGTHS, corpus.DISTANCE,
                                              corpus.OVERRUN, corpus.SHORT, corpus.CRC, corpus.HEADER}


def test_host_check_runs_clean(host):
    assert host["returncode"] == 0, host["output"][-4000:]
    assert not re.search(r"runtime error|AddressSanitizer|MISMATCH", host["output"])
    assert len(host["ok"]) == len(corpus.cases())
    assert host["output"].rstrip().endswith("%d spans, 0 wrong" % len(corpus.cases()))


@pytest.mark.parametrize("name", [c[0] for c in corpus.cases()])
def test_host_check_span(host, name):
    assert host["ok"].get(name) is True, [line for line in host["output"].splitlines() if line.startswith(name + ":")]


def test_status_codes_are_the_header_s():
    text = open(hipbuild.HEADER).read()
    for name in ("HEADER", "CUT", "TRUNCATED", "BTYPE", "STORED_LEN", "CODE_LENGTHS", "SYMBOL", "DISTANCE", "OVERRUN", "SHORT", "TRAILING", "CRC"):
        m = re.search(r"KASA_INFLATE_%s = (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(corpus, name)
    assert "KASA_PARSE_INFLATE = 11" in text
    for s in ("kasa_bgzf_inflate", "kasa_inflate_status_text", "kasa_bgzf_parse_append", "kasa_bgzf_parse_status", "kasa_bgzf_parse_ms"):
        assert s in capi.EXPORTS and re.search(r"\b%s\(" % s, text)
