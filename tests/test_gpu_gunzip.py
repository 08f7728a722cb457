"""Plain gzip inflated on the device (kasa_gzip_inflate; csrc/kasa_gunzip.h) against Python's zlib: the corpus of
tests/gzip_corpus.py at chunks of 64, 256 and 1024 compressed bytes and the default gives zlib's bytes, or the status and the
member of a file zlib refuses, with nothing written.  The chunk statistics keep a run from passing with everything decoded by
one wavefront: where the corpus knows every block start (groups a, b, h), `confirmed` is the number of chunks that hold a
dynamic block's start and nothing is rejected; without a dynamic block one chunk is confirmed (c); the constructed false
candidate is rejected in a second round (d); 200 000 bytes out of 230 take the capacity rerun (e).  The kernels' own
sequencing (64 offsets a step, the token queue, the fenced copies of symbols, the chain and the write pass, the CRC slices)
has no CPU build; the same rounds over the serial bodies ran under the sanitizers first (tools/gunzip_host_check)."""
import pytest

from kasa_amd import capi
from tests import gzip_corpus as corpus

pytestmark = pytest.mark.gpu

CASES = corpus.cases()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the CPU check of the same files, first (once per session)"""
    return corpus.host_check(str(tmp_path_factory.mktemp("gzip_corpus")))


@pytest.mark.parametrize("chunk", corpus.CHUNKS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_corpus(case, chunk, host):
    assert capi.device_count() > 0, "no HIP device visible: the inflater needs a real MI355X"
    # a file the bodies got wrong under the sanitizers does not go to the device
    run = host["runs"].get((case.name, chunk))
    assert run and run["ok"], "the host check of this file failed: not run on the device"
    cap = len(case.raw) if case.raw is not None else 1 << 22
    text, status, member, stats = capi.gzip_inflate(0, case.gz, cap, chunk)
    if case.raw is not None:
        assert (status, member) == (0, 0), capi.inflate_status_text(status)
        assert text == case.raw
        corpus.check_stats(case, chunk, stats)
        assert stats == {k: run[k] for k in corpus.STATS}               # the device ran the rounds the serial bodies ran
    else:
        assert text is None and (status, member) == case.status, (capi.inflate_status_text(status), member)


@pytest.mark.parametrize("chunk", (64, 0))
def test_short_destination_is_a_limit(chunk):
    by = {c.name: c for c in CASES}
    for name, short in (("a_flush_sync_1000", 1), ("a_flush_sync_1000", 17358), ("f_members", 5000), ("f_members", 11999), ("e_one_byte_200000", 0)):
        c = by[name]
        with pytest.raises(RuntimeError, match=r"the text has %d bytes, the destination takes %d" % (len(c.raw), short)):
            capi.gzip_inflate(0, c.gz, short, chunk)
    text, status, _, _ = capi.gzip_inflate(0, by["f_members"].gz, 12000 + 77, chunk)       # more room than text
    assert status == 0 and text == by["f_members"].raw


def test_chunk_size_below_64_is_refused():
    with pytest.raises(RuntimeError, match="chunkBytes 63"):
        capi.gzip_inflate(0, CASES[0].gz, len(CASES[0].raw), 63)


# ---- the same kernels behind the parser's pool: spans of the file as they come (kasa_gzip_parse_append) ------------------------
def _feed(parser, gz, span, fasta=False):
    """the file in reads of `span` bytes, each behind what the call before asked to see again; (reads, text bytes) or the refusal"""
    buf, at, reads, text = b"", 0, 0, 0
    while True:
        buf += gz[at:at + span]
        at += span
        final = at >= len(gz)
        n, ok, nt, keep = parser.append_gzip(buf, fasta, final)
        if not ok:
            print("refused at byte", at, parser.status(), parser.gzip_status())
            return None
        assert keep <= len(buf)
        reads, text, buf = reads + n, text + nt, buf[keep:]
        if final:
            return reads, text


@pytest.mark.parametrize("span", (700, 1500, 1 << 20))
@pytest.mark.parametrize("name", ("a_flush_full_300", "a_flush_sync_1000", "h_reads_fastq_level1", "h_reads_fastq_level9"))
def test_spans_pool_what_the_text_pools(name, span):
    case = {c.name: c for c in CASES}[name]
    want, got = capi.Parser(0), capi.Parser(0)
    try:
        n, ok = want.append(case.raw, False)
        assert ok and n > 50
        assert _feed(got, case.gz, span) == (n, len(case.raw))
        a, b = want.fetch(), got.fetch()
        assert all((x == y).all() for x, y in zip(a, b))
        code, _, member, stats = got.gzip_status()
        assert (code, member) == (0, 0) and stats["members"] == 1 and stats["rejected"] == 0 and stats["confirmed"] >= 1
    finally:
        want.close()
        got.close()


@pytest.mark.parametrize("case", [c for c in CASES if c.group == "g" or c.name.startswith("f_distance")], ids=lambda c: c.name)
def test_spans_of_a_malformed_file_are_refused_with_its_status(case):
    p = capi.Parser(0)
    try:
        # (the second member of the f cases begins with valid blocks of bytes that are no FASTQ: they go up in one span, so
        # that the block that does not inflate is met before that text is parsed)
        assert _feed(p, case.gz, 700 if case.group == "g" else 1 << 20) is None
        assert p.status()[0] == 11                                      # KASA_PARSE_INFLATE
        code, _, member, _ = p.gzip_status()
        assert (code, member) == case.status
    finally:
        p.close()
