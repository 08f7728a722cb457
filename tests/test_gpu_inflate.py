"""BGZF inflated on the device (kasa_bgzf_inflate, kasa_bgzf_parse_append; csrc/kasa_inflate.h) against Python's zlib and
against the parser fed with plain text: the corpus of tests/inflate_corpus.py gives zlib's bytes or its status and member,
what the device's own deflater wrote comes back, members land at the running sum of ISIZE, and a file cut into members of
997 bytes -- they end inside headers, sequences and quality lines -- pools the reads one append of the whole text pools.
The second half takes corpus.built_cases(), the members tests/deflate_writer.py makes by construction (what zlib's compressor
never writes), as spans of many members: the kernel's own sequencing, copies, token queue and CRC slices have no CPU build."""
import ctypes as C
import os

import numpy as np
import pytest

from kasa_amd import capi, formats
from tests import helpers, inflate_corpus as corpus
from tests.test_bgzf_cpu import INPUTS, golden_texts

pytestmark = pytest.mark.gpu

KASA_E_LIMIT = 5                        # include/kasa_hip.h
KASA_PARSE_BLANK, KASA_PARSE_FASTA_HEADER, KASA_PARSE_INFLATE = 6, 8, 11

PAIRS_DIR = os.path.join(helpers.GOLDEN, "pairs")
CASES = {c[0]: c for c in corpus.cases()}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the CPU check of the same spans, first (once per session)"""
    return corpus.host_check(str(tmp_path_factory.mktemp("inflate_corpus")))


@pytest.mark.parametrize("name", list(CASES))
def test_corpus(name, host):
    assert capi.device_count() > 0, "no HIP device visible: the inflater needs a real MI355X"
    _, span, raw, status = CASES[name]
    # a span the decoder body got wrong under the sanitizers does not go to the device
    assert host["ok"].get(name) is True, "the host check of this span failed: not run on the device"
    text, st, member = capi.bgzf_inflate(0, span)
    if raw is not None:
        assert (st, member) == (0, 0), capi.inflate_status_text(st)
        assert text == raw
    else:
        assert text is None and (st, member) == status, (capi.inflate_status_text(st), member)


@pytest.mark.parametrize("name", list(INPUTS))
def test_what_the_device_deflated_comes_back(name):
    data = INPUTS[name]
    text, st, _ = capi.bgzf_inflate(0, capi.bgzf_deflate(0, data))
    assert st == 0 and text == data


def test_golden_per_read_files_round_trip():
    files = golden_texts()
    assert len(files) > 20
    for f in files:
        data = open(f, "rb").read()
        text, st, _ = capi.bgzf_inflate(0, capi.bgzf_deflate(0, data))
        assert st == 0 and text == data, f


def _members_of(data, size=997, level=6):
    return corpus.members(data, block=size, level=level)


def test_three_hundred_members_land_at_the_prefix_sum():
    raw = open(os.path.join(PAIRS_DIR, "reads.fastq"), "rb").read()
    data = (raw * (300 * 997 // len(raw) + 1))[:300 * 997]
    ms = _members_of(data)
    assert len(ms) == 300
    rows, consumed, status = formats.bgzf_member_table(b"".join(ms))
    assert status == 0 and [r[6] for r in rows] == [997 * i for i in range(300)]
    text, st, _ = capi.bgzf_inflate(0, b"".join(ms))
    assert st == 0 and text == data
    # members of unequal ISIZE, EOF members among them
    mixed = []
    for i in range(0, 40):
        mixed += _members_of(data[1000 * i:1000 * i + 1 + 37 * i], size=70000) + ([formats.BGZF_EOF] if i % 7 == 0 else [])
    want = b"".join(data[1000 * i:1000 * i + 1 + 37 * i] for i in range(40))
    text, st, _ = capi.bgzf_inflate(0, b"".join(mixed))
    assert st == 0 and text == want


def test_tap_edges():
    lib = capi.lib()
    got, st, member = C.c_uint64(7), C.c_int(7), C.c_uint64(7)
    assert lib.kasa_bgzf_inflate(C.c_int(0), None, C.c_uint64(0), None, C.c_uint64(0), C.byref(got), C.byref(st), C.byref(member)) == 0
    assert (got.value, st.value, member.value) == (0, 0, 0)                # an empty stream: no member
    span = np.frombuffer(CASES["runs_level9"][1], dtype=np.uint8)
    small = np.zeros(64, dtype=np.uint8)
    rc = lib.kasa_bgzf_inflate(C.c_int(0), C.c_void_p(span.ctypes.data), C.c_uint64(span.shape[0]), C.c_void_p(small.ctypes.data), C.c_uint64(8),
                               C.byref(got), C.byref(st), C.byref(member))
    assert rc == KASA_E_LIMIT and got.value == len(INPUTS["runs"]) and not small.any()      # says what it needs, writes nothing
    assert capi.inflate_status_text(0) == "inflated" and "CRC" in capi.inflate_status_text(corpus.CRC) and capi.inflate_status_text(99) == "unknown"


# ---- the parser fed with members ----------------------------------------------------------------------------------------------
PARSER_INPUTS = ["reads.fastq", "reads.fasta", "edge_crlf.fasta", "edge_multi.fastq", "edge_noeol.fasta"]


def _plain_pool(text, fasta, long_sequence=1_000_000):
    ps = capi.Parser(0, long_sequence)
    try:
        n, ok = ps.append(text, fasta)
        assert ok, ps.status()
        return n, ps.sizes(), ps.fetch()
    finally:
        ps.close()


_PLAIN = {}


def _plain(name):
    if name not in _PLAIN:
        text = open(os.path.join(PAIRS_DIR, name), "rb").read()
        _PLAIN[name] = (text,) + _plain_pool(text, name.endswith(".fasta"))
    return _PLAIN[name]


def _feed(ps, ms, per_span, fasta):
    """members in spans of `per_span`, final on the last: [(reads, text bytes, carry)] per call"""
    calls = []
    spans = [ms[i:i + per_span] for i in range(0, len(ms), per_span)]
    for k, span in enumerate(spans):
        n, ok, nt, carry = ps.append_bgzf(b"".join(span), fasta, final=k == len(spans) - 1)
        assert ok, (ps.status(), ps.inflate_status())
        calls.append((n, nt, carry))
    return calls


@pytest.mark.parametrize("per_span", [1, 3, 50])
@pytest.mark.parametrize("name", PARSER_INPUTS)
def test_append_bgzf_equals_append(name, per_span):
    assert capi.device_count() > 0
    text, n, sizes, pool = _plain(name)
    fasta = name.endswith(".fasta")
    ms = _members_of(text)
    assert len(ms) == (len(text) + 996) // 997
    ps = capi.Parser(0)
    try:
        calls = _feed(ps, ms, per_span, fasta)
        assert sum(c[0] for c in calls) == n and ps.sizes() == sizes
        assert sum(c[1] for c in calls) == len(text) and calls[-1][2] == 0
        # every call but the last cut where the rule says: the text up to the cut is what record_cut gives on what was there
        at = 0
        for k, (_, nt, carry) in enumerate(calls[:-1]):
            there = text[at:997 * per_span * (k + 1)]
            assert nt == formats.record_cut(there, fasta) and carry == len(there) - nt
            at += nt
        for x, y in zip(ps.fetch(), pool):
            assert np.array_equal(x, y)
        assert ps.inflate_ms() > 0 and ps.stage_ms()[0] > 0
    finally:
        ps.close()


def test_a_fasta_record_longer_than_three_spans():
    """calls that add no read and carry everything, then all of them"""
    rng = np.random.default_rng(5)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 9000)].tobytes()
    text = b">short\nACGTACGT\n>contig one\n" + b"\n".join(seq[i:i + 70] for i in range(0, 9000, 70)) + b"\n>last\nGGCC\n"
    n, sizes, pool = _plain_pool(text, True)
    assert n == 3
    ms = _members_of(text)
    ps = capi.Parser(0)
    try:
        calls = _feed(ps, ms, 2, True)
        assert calls[0][0] == 1 and calls[0][1] == text.index(b">contig")
        idle = [c for c in calls[1:-1] if c[0] == 0]
        assert len(idle) >= 3 and all(c[1] == 0 for c in idle)                 # nothing parsed, everything carried
        assert [c[2] for c in calls[1:len(idle) + 1]] == [min(len(text), 1994 * (k + 2)) - calls[0][1] for k in range(len(idle))]
        assert sum(c[0] for c in calls) == 3 and sum(c[1] for c in calls) == len(text) and calls[-1][2] == 0
        assert ps.sizes() == sizes
        for x, y in zip(ps.fetch(), pool):
            assert np.array_equal(x, y)
    finally:
        ps.close()


def test_refusals_leave_pool_and_carry():
    text = open(os.path.join(PAIRS_DIR, "reads.fastq"), "rb").read()
    ms = _members_of(text)
    ps = capi.Parser(0)
    try:
        n0, ok, nt0, carry0 = ps.append_bgzf(b"".join(ms[:5]), False)
        assert ok and n0 > 0 and carry0 > 0 and nt0 + carry0 == 5 * 997
        before, kept = ps.sizes(), ps.fetch()
        # a member whose CRC is wrong: KASA_PARSE_INFLATE, the member's index in the span
        crc_bad = corpus.edit_member(ms[6], crc=int.from_bytes(ms[6][-8:-4], "little") ^ 1)
        assert ps.append_bgzf(ms[5] + crc_bad + ms[7], False) == (0, False, 0, carry0)
        assert ps.status()[0] == KASA_PARSE_INFLATE and ps.status()[2] == 1
        assert ps.inflate_status()[0] == corpus.CRC and ps.inflate_status()[2] == 1
        # a span that is cut
        assert ps.append_bgzf(ms[5] + ms[6][:-3], False) == (0, False, 0, carry0)
        assert ps.status()[0] == KASA_PARSE_INFLATE and ps.inflate_status()[0] == corpus.CUT and ps.inflate_status()[2] == 1
        # plain text while bytes are carried is a state error
        with pytest.raises(RuntimeError, match="carried"):
            ps.append(b"@a\nAC\n+\nII\n", False)
        # a parse refusal: `at` is counted in the cut text, carry included
        full = bytearray(text[nt0:8 * 997])                                   # what the pool would see: the carry, then three members
        pos, target = 0, None
        for i, line in enumerate(bytes(full).split(b"\n")):
            if i % 4 == 1 and pos > carry0 + 10 and target is None:
                target = pos + 3
            pos += len(line) + 1
        assert target is not None and target < formats.record_cut(bytes(full), False)
        full[target] = 9
        tabbed, pos = full[carry0:], target - carry0
        assert ps.append_bgzf(b"".join(_members_of(bytes(tabbed))), False) == (0, False, 0, carry0)
        assert ps.status()[0] == KASA_PARSE_BLANK and ps.status()[2] == carry0 + pos == target
        assert ps.sizes() == before
        for x, y in zip(ps.fetch(), kept):
            assert np.array_equal(x, y)
        # the pool goes on where it was
        n1, ok, nt1, carry1 = ps.append_bgzf(b"".join(ms[5:]), False, final=True)
        assert ok and carry1 == 0 and nt0 + nt1 == len(text)
        _, n, sizes, pool = _plain("reads.fastq")
        assert n0 + n1 == n and ps.sizes() == sizes
        for x, y in zip(ps.fetch(), pool):
            assert np.array_equal(x, y)
    finally:
        ps.close()


def test_fasta_text_without_a_header_is_refused_at_the_first_span():
    """not carried span after span: refused as kasa_parse_append refuses it"""
    ms = _members_of(b"ACGTACGT\n" * 300)
    ps = capi.Parser(0)
    try:
        assert ps.append_bgzf(b"".join(ms[:2]), True) == (0, False, 0, 0)
        assert ps.status()[0] == KASA_PARSE_FASTA_HEADER and ps.sizes() == (0, 0, 0)
        assert ps.append_bgzf(b"".join(_members_of(b">a\nACGT\n")), True, final=True) == (1, True, 8, 0)
    finally:
        ps.close()


# ---- members zlib's compressor never writes (corpus.built_cases; tests/test_inflate_cpu.py has run them on the CPU) -----------
BUILT = {c[0]: c for c in corpus.built_cases()}
BUILT_SPANS = {g: [c[0] for c in corpus.built_cases() if c[0][0] == g and c[2] is not None] for g in "ABCDEF"}
_G = [c[0] for c in corpus.built_cases() if c[0][0] == "G"]
BUILT_SPANS.update({"G%d" % k: _G[100 * k:100 * k + 100] + (_G[300:] if k == 2 else []) for k in range(3)})
assert sum(len(v) for v in BUILT_SPANS.values()) == sum(1 for c in BUILT.values() if c[2] is not None)


def _member_names(names):
    """the case name of every member of the cases' spans put together"""
    return [name for name in names for _ in formats.bgzf_member_table(BUILT[name][1])[0]]


@pytest.mark.parametrize("group", list(BUILT_SPANS))
def test_built_group(group):
    """a whole group as ONE span of many members: zlib's text of every member, each at the running sum of ISIZE"""
    assert capi.device_count() > 0, "no HIP device visible: the inflater needs a real MI355X"
    names = BUILT_SPANS[group]
    span, want = b"".join(BUILT[n][1] for n in names), b"".join(BUILT[n][2] for n in names)
    rows, consumed, walk = formats.bgzf_member_table(span)
    of = _member_names(names)
    assert walk == 0 and consumed == len(span) and len(of) == len(rows)
    text, st, member = capi.bgzf_inflate(0, span)
    assert (st, member) == (0, 0), "member %d (%s): %s" % (member, of[member], capi.inflate_status_text(st))
    if text != want:
        for k, r in enumerate(rows):
            a, b = r[6], r[6] + r[5]
            if text[a:b] != want[a:b]:
                at = next(i for i in range(a, b) if text[i] != want[i])
                pytest.fail("member %d (%s) differs first at its byte %d of %d: %d for %d" % (k, of[k], at - a, r[5], text[at], want[at]))
    assert text == want


@pytest.mark.parametrize("name", [c[0] for c in corpus.built_cases() if c[2] is None])
def test_built_malformed(name):
    _, span, _, status = BUILT[name]
    text, st, member = capi.bgzf_inflate(0, span)
    assert text is None and (st, member) == status, (capi.inflate_status_text(st), member)


@pytest.mark.parametrize("group", list(BUILT_SPANS))
def test_built_texts_round_trip(group):
    """the texts of the built members -- long overlapping runs, far matches, random bytes -- through the device's own
    deflater and back, a text per call"""
    for name in BUILT_SPANS[group]:
        data = BUILT[name][2]
        text, st, _ = capi.bgzf_inflate(0, capi.bgzf_deflate(0, data))
        assert st == 0 and text == data, name


def test_built_members_feed_the_parser():
    """group G's member maker over the FASTQ file (literals and random back-references into itself), one append: the pool of
    the plain text"""
    _, span, text, _ = BUILT["G_over_fastq"]
    assert text == _plain("reads.fastq")[0] and len(formats.bgzf_member_table(span)[0]) > 5
    _, n, sizes, pool = _plain("reads.fastq")
    ps = capi.Parser(0)
    try:
        got = ps.append_bgzf(span, False, final=True)
        assert got == (n, True, len(text), 0), (got, ps.status(), ps.inflate_status())
        assert ps.sizes() == sizes
        for x, y in zip(ps.fetch(), pool):
            assert np.array_equal(x, y)
    finally:
        ps.close()
