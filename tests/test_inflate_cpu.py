"""The device inflater without a device: formats.bgzf_member_table / record_cut (the member walk and the two cut rules of
kasa_bgzf_parse_append, stated in Python) on hand-made input, and the decoder body of csrc/kasa_inflate.h -- the very
functions inflate_kernel runs -- compiled for the CPU under AddressSanitizer + UBSan (tools/inflate_host_check, a stand-alone
program) over the corpus of tests/inflate_corpus.py: every span gives its bytes or its status, and the run ends clean.
One run of the program takes cases() and built_cases() -- the members made by construction, which zlib's compressor never
writes -- and test_built_corpus_covers_what_it_claims checks the generator itself: that what it wrote holds what it is for.

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
    assert len(host["ok"]) == len(corpus.all_cases())
    assert host["output"].rstrip().endswith("%d spans, 0 wrong" % len(corpus.all_cases()))


@pytest.mark.parametrize("name", [c[0] for c in corpus.cases()])
def test_host_check_span(host, name):
    assert host["ok"].get(name) is True, [line for line in host["output"].splitlines() if line.startswith(name + ":")]


# ---- (c) members zlib's compressor never writes (corpus.built_cases, made by tests/deflate_writer.py) ------------------------
BUILT = corpus.built_cases()


def test_built_corpus_is_what_it_says():
    """zlib's inflater judged every member where it was made; here gzip reads the spans as files"""
    assert not {c[0] for c in BUILT} & {c[0] for c in corpus.cases()}
    for name, span, raw, status in BUILT:
        assert name[0] in corpus.GROUPS + "H"
        if raw is not None:
            assert status is None and name[0] in corpus.GROUPS and gzip.decompress(span + formats.BGZF_EOF) == raw, name
        else:
            assert name[0] == "H" and corpus.gzip_rejects(span), name
            rows, consumed, st = formats.bgzf_member_table(span)
            assert st == 0 and consumed == len(span) and status[1] < len(rows), name       # the header walk takes all of it: the payload is what is wrong
    assert {s[0] for *_, s in BUILT if s} == {corpus.TRUNCATED, corpus.CODE_LENGTHS, corpus.SYMBOL, corpus.DISTANCE, corpus.OVERRUN, corpus.SHORT,
                                              corpus.TRAILING}
    assert len([c for c in BUILT if c[0].startswith("G_seed_")]) == len(corpus.G_SEEDS)     # none was larger than BSIZE can state
    assert all(sum(c[0].startswith("G_seed_%d" % h) for c in BUILT) == 100 for h in range(3))


def test_host_check_built_runs_clean(host):
    """the sanitizer run gave every built span a report line, and none of them a wrong one"""
    lines = {line.split(":", 1)[0]: line for line in host["output"].splitlines() if ": status " in line and not line.startswith(" ")}
    for name, _, raw, status in BUILT:
        assert name in lines and "MISMATCH" not in lines[name], lines.get(name)
        assert ("status 0, %d bytes" % len(raw) if raw is not None else "status %d (rejected) in member %d" % status) in lines[name], lines[name]


@pytest.mark.parametrize("name", [c[0] for c in BUILT])
def test_host_check_built_span(host, name):
    assert host["ok"].get(name) is True, [line for line in host["output"].splitlines() if line.startswith(name + ":")]


def _blocks(prefix, kind=None):
    """the writer's records of the blocks of every member whose case name begins with prefix"""
    return [b for name, ms in corpus.built_info().items() if name.startswith(prefix) and name != "H_cuts"
            for m in ms for b in m if kind is None or b["kind"] == kind]


def test_built_corpus_covers_what_it_claims():
    """conditions on the GENERATOR: what the writer recorded while it wrote, block by block, holds every item the corpus is
    there for.  No case is left out to make one of them true."""
    W = corpus.W
    every_l, every_d = set(range(257, 286)), set(range(30))
    for kind in ("fixed", "dynamic"):
        (b,) = _blocks("A_alphabet_" + kind)
        assert b["kind"] == kind and b["lsyms"] >= every_l and b["dsyms"] >= every_d
        assert b["lext"] >= {(s, e) for s in every_l for e in ("min", "max")} and b["dext"] >= {(s, e) for s in every_d for e in ("min", "max")}
    for d in (1, 300):
        for kind in ("fixed", "dynamic"):
            (b,) = _blocks("A_lengths_d%d_%s" % (d, kind))
            assert sorted(m[3] for m in b["matches"]) == list(range(3, 259)) and {m[4] for m in b["matches"]} == {d}
    (b,) = _blocks("A_258_as_284")
    assert 284 in b["lsyms"] and 285 not in b["lsyms"] and {m[3] for m in b["matches"]} == {258} and (284, "max") in b["lext"]
    (b,) = _blocks("A_distance32768")
    assert b["matches"] == [(32768, b["matches"][0][1], 32768, 258, 32768)] and (29, "max") in b["dext"]
    # code lengths either side of the fast tables (10 / 8 bits) and up to 15, on symbols that were written
    dyn = _blocks("", "dynamic")
    assert set().union(*(b["llens"] for b in dyn)) >= set(range(1, 16)) and set().union(*(b["dlens"] for b in dyn)) >= set(range(1, 16))
    assert set().union(*(b["llens"] for b in _blocks("B_litlen_1_to_15"))) == set(range(1, 16))
    assert set().union(*(b["dlens"] for b in _blocks("B_distance_1_to_15"))) == set(range(1, 16))
    (_, b) = _blocks("B_48_bit")
    assert b["cl_lengths"] and any(m[3] in range(227, 259) and m[4] >= 24577 for m in b["matches"]) and {15} <= b["llens"] and {15} <= b["dlens"]
    assert [(b["lsyms"], b["ntok"], b["hdist"]) for b in _blocks("B_only_end_of_block_final")] == [({256}, 0, 1)]
    assert [b["hlit"] for b in _blocks("B_hlit257")] == [257] and [b["hlit"] for b in _blocks("B_hlit286")] == [286] and 285 in _blocks("B_hlit286")[0]["lsyms"]
    assert _blocks("B_hdist30")[1]["hdist"] == 30 and 29 in _blocks("B_hdist30")[1]["dsyms"]
    # the header's sequence
    assert _blocks("C_hclen19")[0]["hclen"] == 19 and _blocks("C_hclen5")[0]["hclen"] == 5
    (b,) = _blocks("C_code_length_code_7")
    assert {s for s, _, _ in b["items"] if b["cl_lengths"][s] == 7}
    items = {(s, r) for b in dyn for s, r, _ in b["items"]}
    assert items >= {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)}
    assert {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)} <= {(s, r) for s, r, _ in _blocks("C_repeats")[0]["items"]}
    across = {s for b in dyn for s, r, at in b["items"] if s >= 16 and at < b["hlit"] < at + r}
    assert across >= {16, 18}
    assert [s for s, r, at in _blocks("C_16_across")[0]["items"] if at < 258 < at + r] == [16]
    assert [s for s, r, at in _blocks("C_18_across")[0]["items"] if at < 272 < at + r] == [18]
    (b,) = _blocks("C_header316")
    assert len(b["items"]) == 316 and all(b["cl_lengths"][s] == 7 for s, _, _ in b["items"]) and (b["header_end_bit"] - b["bit"]) // 8 == 285
    # where a dynamic header begins
    for prefix, first, offsets in (("D_stored_then_dynamic_at_", "stored", corpus.HEADER_OFFSETS), ("D_stored_then_header316_at_", "stored", corpus.HEADER316_OFFSETS),
                                   ("D_fixed_then_header316_at_", "fixed", corpus.HEADER_OFFSETS)):
        got = set()
        for name, ms in corpus.built_info().items():
            if name.startswith(prefix):
                (one, two), = ms
                assert one["kind"] == first and two["kind"] == "dynamic" and two["final"] and not one["final"]
                got.add(two["bit"] // 8)
        assert got == set(offsets), prefix
    assert {tuple(b["kind"] for b in ms[0]) for name, ms in corpus.built_info().items() if name.startswith("D_") and name.count("_then_") == 1
            and "_at_" not in name and "_three_" not in name} == {(a, b) for a in ("stored", "fixed", "dynamic") for b in ("stored", "fixed", "dynamic")}
    assert {b[1]["bit"] % 8 for name, ms in corpus.built_info().items() if name.startswith("D_stored_after_") for b in [ms[0]]} == set(range(8))
    assert _blocks("D_largest_stored")[0]["end_bit"] == 8 * W.MAX_PAYLOAD and _blocks("D_largest_fixed")[0]["end_bit"] == 8 * W.MAX_PAYLOAD
    # the copy rule and the queue: a queue is tokens 0..127 of a block that lies in one window
    assert {(m[3], m[4]) for b in _blocks("E_overlap_258_at_") for m in b["matches"]} == {(258, d) for d in range(1, 67)}
    (b,) = _blocks("E_chain_of_200")
    assert len(b["matches"]) == 200 and all(m[4] == prev[3] for prev, m in zip(b["matches"], b["matches"][1:]))
    slots = set()
    for lead in (126, 127, 128):
        (b,) = _blocks("E_dependent_pair_after_%d" % lead)
        (k1, _, p1, l1, _), (k2, _, p2, l2, d2) = b["matches"][:2]
        assert b["bit"] == 0 and b["end_bit"] < 8 * 240 and (k1, k2) == (lead, lead + 1) and p2 - d2 == p1 and l2 <= l1      # token k2 reads what token k1 wrote
        slots.add((k1 // 128, k1 % 128, k2 // 128, k2 % 128))
        (b,) = _blocks("E_literal_then_match_after_%d" % lead)
        assert b["matches"][0][0] == lead + 1 and b["matches"][0][4] == 1
    assert slots == {(0, 126, 0, 127), (0, 127, 1, 0), (1, 0, 1, 1)}
    ends = set()
    for delta in (-1, 0, 1):
        (b,) = _blocks("E_source_ends_%+d" % delta)
        (_, _, p1, _, _), (_, _, p2, l2, d2) = b["matches"][:2]
        assert d2 >= l2 and b["ntok"] < 128
        ends.add(p2 - d2 + l2 - p1)
    assert ends == {-1, 0, 1}
    # ISIZE 0..200 in one span; G: 1, 2 and 3 blocks, both ways of stating HLIT / HDIST, every text size
    cases = {c[0]: c for c in BUILT}
    rows = formats.bgzf_member_table(cases["F_isize_0_to_200"][1])[0]
    assert [r[5] for r in rows] == list(range(201))
    assert {len(c[2]) for c in BUILT if c[0].startswith("F_isize_")} >= {4095, 4096, 4097, 65535, 65536}
    g = [ms[0] for name, ms in corpus.built_info().items() if name.startswith("G_seed_")]
    assert {len(m) for m in g} == {1, 2, 3} and {(b["hlit"] == 286, b["hdist"] == 30) for m in g for b in m} >= {(True, True), (False, False)}
    assert {len(c[2]) for c in BUILT if c[0].startswith("G_seed_")} == {50, 300, 3000, 20000}
    # (random splits seldom reach 15 bits -- group B holds those -- but G's codes do pass both fast tables)
    assert max(max(b["llens"]) for m in g for b in m) > 10 and max(max(b["dlens"] or {0}) for m in g for b in m) > 8
    # the cuts: every proper prefix of both members
    for kind in ("dynamic", "fixed"):
        n, blocks = corpus.built_info()["H_cuts"][kind]
        assert 60 <= n <= 200 and blocks[0]["kind"] == kind
        assert [c[0] for c in BUILT if c[0].startswith("H_%s_cut_at_" % kind)] == ["H_%s_cut_at_%03d" % (kind, k) for k in range(n)]


def test_status_codes_are_the_header_s():
    text = open(hipbuild.HEADER).read()
    for name in ("HEADER", "CUT", "TRUNCATED", "BTYPE", "STORED_LEN", "CODE_LENGTHS", "SYMBOL", "DISTANCE", "OVERRUN", "SHORT", "TRAILING", "CRC"):
        m = re.search(r"KASA_INFLATE_%s = (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(corpus, name)
    assert "KASA_PARSE_INFLATE = 11" in text
    for s in ("kasa_bgzf_inflate", "kasa_inflate_status_text", "kasa_bgzf_parse_append", "kasa_bgzf_parse_status", "kasa_bgzf_parse_ms"):
        assert s in capi.EXPORTS and re.search(r"\b%s\(" % s, text)
