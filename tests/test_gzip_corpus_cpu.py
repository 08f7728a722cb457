"""The chunked gzip inflater without a device.  The corpus of tests/gzip_corpus.py judges itself against zlib (every text, every
stated block start, every refusal), and tools/gunzip_host_check -- the bodies of csrc/kasa_gunzip.h (header validation, the
16-bit symbol decoder, the window resolve, the marker replacement) and the very rounds the device runs, compiled for the CPU
under AddressSanitizer + UBSan, a stand-alone program -- inflates it at every chunk size the GPU test uses and reports the
chunk statistics, so what tests/test_gpu_gunzip.py expects of the device is checked here first: in particular that the fixed
seeds hold no chance candidate in the groups whose `confirmed` count the corpus states."""
import gzip
import re
import zlib

import pytest

from kasa_amd import build as hipbuild, capi
from tests import gzip_corpus as corpus

CASES = corpus.cases()
VALID = [c for c in CASES if c.raw is not None]
TABLED = [c for c in CASES if c.starts]


# ---- the corpus against zlib ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", VALID, ids=lambda c: c.name)
def test_valid_file_inflates_with_zlib(case):
    assert gzip.decompress(case.gz) == case.raw


@pytest.mark.parametrize("case", [c for c in CASES if c.raw is None], ids=lambda c: c.name)
def test_malformed_file_is_refused_by_zlib(case):
    assert corpus.gzip_rejects(case.gz)
    code, member = case.status
    assert 1 <= code <= 14 and member in (0, 1)


@pytest.mark.parametrize("case", TABLED, ids=lambda c: c.name)
def test_every_stated_block_start_is_one(case):
    """zlib inflates the block's text from the stream re-aligned to the bit, given the 32 KiB before as its dictionary"""
    bits = int.from_bytes(case.gz[:-8], "little")
    assert case.starts[0][0] == 8 * case.data_at and case.starts[0][2] == 0
    assert [s[0] for s in case.starts] == sorted({s[0] for s in case.starts})
    for k, (bit, kind, before) in enumerate(case.starts):
        assert (bits >> (bit + 1)) & 3 == ("stored", "fixed", "dynamic").index(kind)
        if kind == "stored":
            # (its padding is counted from the stream's first bit, so it cannot be moved: read as it stands)
            at = (bit + 3 + 7) // 8
            n = int.from_bytes(case.gz[at:at + 2], "little")
            assert n ^ 0xFFFF == int.from_bytes(case.gz[at + 2:at + 4], "little") and case.gz[at + 4:at + 4 + n] == case.raw[before:before + n]
            assert (bits >> bit) & 1 or case.starts[k + 1][::2] == (8 * (at + 4 + n), before + n)
            continue
        # the block alone: its bits moved to bit 0, and behind them (a stored block that follows could not be moved) an empty last block
        if k + 1 < len(case.starts):
            n, until = case.starts[k + 1][0] - bit, case.starts[k + 1][2]
            rest = ((bits >> bit) & ((1 << n) - 1) | 3 << n).to_bytes((n + 10 + 7) // 8, "little")
        else:
            rest, until = (bits >> bit).to_bytes(len(case.gz) - bit // 8, "little"), len(case.raw)
        z = zlib.decompressobj(-15, zdict=case.raw[max(0, before - 32768):before]) if before else zlib.decompressobj(-15)
        assert z.decompress(rest) == case.raw[before:until] and z.eof, (case.name, bit)


def test_corpus_covers_what_it_claims():
    by = {c.name: c for c in CASES}
    # a: every alignment; the first and the last bit of a chunk of 64, 256 and 1024 bytes; many dynamic blocks
    a = by["a_alignments"]
    rel = [s[0] - 8 * a.data_at for s in a.starts if s[1] == "dynamic"]
    assert {r % 8 for r in rel} == set(range(8))
    for chunk in (64, 256, 1024):
        assert {0, 8 * chunk - 1} <= {r % (8 * chunk) for r in rel if r}
    assert any((x // 8192 == y // 8192) for x, y in zip(rel, rel[1:]))                      # two starts in one chunk
    assert sum(s[1] == "dynamic" for s in by["a_flush_full_300"].starts) >= 50 and sum(s[1] == "dynamic" for s in by["a_flush_sync_1000"].starts) >= 10
    # b: the tokens the writer was given are in the files (the block table's text positions are the writer's)
    for name in ("b_distance1_x258", "b_distance32768", "b_match_of_markers", "b_two_windows"):
        c = by[name]
        assert [s[1] for s in c.starts] == ["dynamic"] * len(c.starts) and len(c.starts) >= 3
        for chunk in (64, 256, 1024):
            assert corpus.expected_confirmed(c, chunk) == len(c.starts)                     # every block begins in a chunk of its own
    c = by["b_distance1_x258"]
    at = c.starts[1][2]
    assert c.raw[at - 1:at + 516] == c.raw[at - 1:at] * 517
    c = by["b_distance32768"]
    at = c.starts[1][2]
    assert at == 32768 and c.raw[at:at + 258] == c.raw[:258]
    c = by["b_two_windows"]
    assert len(c.raw) > 65536 and c.starts[2][2] - c.starts[1][2] < 32768
    # c, d, e
    assert all({s[1] for s in by[n].starts} <= {"fixed", "stored"} for n in ("c_fixed_and_stored", "c_stored"))
    d = by["d_false_candidate"]
    kinds = [s[1] for s in d.starts]
    assert kinds == ["dynamic", "stored", "fixed", "dynamic", "dynamic"]
    false_at = d.data_at + corpus.D_FALSE_AT
    assert d.starts[1][0] < 8 * false_at < d.starts[2][0] and (d.gz[false_at] >> 1) & 3 == 2
    for chunk in (64, 256, 1024, 65536):
        first = (corpus.D_FALSE_AT // chunk) * chunk                 # the false header's chunk holds no true dynamic start before it
        assert first > 0 and not [s for s in d.starts if s[1] == "dynamic" and 8 * (d.data_at + first) <= s[0] < 8 * false_at]
    e = by["e_one_byte_200000"]
    assert len(e.raw) == 200000 and len(e.gz) < 320
    # f: five members, two of them empty, one with every optional header field
    f = by["f_members"].gz
    assert f.count(b"\x1f\x8b\x08") == 5 and corpus.rich_header() in f and b"BC" not in corpus.rich_header()
    # g: each status at least once
    assert {c.status[0] for c in CASES if c.status} >= {corpus.CRC, corpus.SHORT, corpus.OVERRUN, corpus.TRUNCATED, corpus.CUT, corpus.BTYPE, corpus.DISTANCE,
                                                        corpus.GZIP_HEADER}
    assert len([c for c in CASES if c.group == "h"]) == 12


# ---- the bodies and the rounds under the sanitizers -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return corpus.host_check(str(tmp_path_factory.mktemp("gzip_corpus")))


def test_host_check_runs_clean(host):
    assert host["returncode"] == 0, host["output"][-4000:]
    assert not re.search(r"runtime error|AddressSanitizer|MISMATCH", host["output"])
    assert len(host["runs"]) == len(CASES) * len(corpus.CHUNKS)
    assert host["output"].rstrip().endswith("%d files, %d runs, 0 wrong" % (len(CASES), len(CASES) * len(corpus.CHUNKS)))


@pytest.mark.parametrize("chunk", corpus.CHUNKS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_host_check_file(host, case, chunk):
    run = host["runs"].get((case.name, chunk))
    assert run and run["ok"], [line for line in host["output"].splitlines() if line.startswith(case.name + " @%d:" % chunk)]
    if case.raw is not None:
        assert (run["status"], run["bytes"]) == (0, len(case.raw))
    else:
        assert run["status"] == case.status[0]
    corpus.check_stats(case, chunk, run)


def test_status_codes_and_symbol_are_the_header_s():
    text = open(hipbuild.HEADER).read()
    for name in ("HEADER", "CUT", "TRUNCATED", "BTYPE", "STORED_LEN", "CODE_LENGTHS", "SYMBOL", "DISTANCE", "OVERRUN", "SHORT", "TRAILING", "CRC", "GZIP_HEADER",
                 "SPAN"):
        m = re.search(r"KASA_INFLATE_%s = (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(corpus, name)
    assert "kasa_gzip_inflate" in capi.EXPORTS and re.search(r"^int kasa_gzip_inflate\(", text, re.M)
    L = capi.lib()
    assert L.kasa_inflate_status_text(13) == b"no gzip member header" and L.kasa_inflate_status_text(14) == b"a block longer than the span limit"
    assert capi.GZIP_STATS == corpus.STATS
