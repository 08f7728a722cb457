"""tests/parse_corpus.py holds what it says it holds -- asserted from the texts alone, without a device --, the host parser
`reads.parse_reads` takes every member the corpus calls parsable and refuses the ones it has to, and the driver's `parse-dump`
tap (`parseRecords`, the specification of the device parser) agrees with `parse_reads` on every member its line format
can carry."""
import os
import subprocess

import numpy as np
import pytest

from kasa_amd import build as hipbuild, capi, reads
from tests import parse_corpus as pc

GROUPS = ("A", "B", "C", "D", "E", "F")


def _T():
    return capi.parse_tile_bytes()


def _parse(tmp_path, text: bytes):
    p = tmp_path / "in.txt"
    p.write_bytes(text)
    return reads.parse_reads(str(p))


def test_the_tile_is_what_the_corpus_is_built_around():
    assert _T() == 4096 and len(pc.corpus(_T())) == len({m.name for m in pc.corpus(_T())})
    assert pc.corpus(_T()) is pc.corpus(_T())
    for g in GROUPS:
        assert pc.group(_T(), g)
    # no text above about 4 tiles but the line of 3T + 1 letters; 64 KB is never reached
    assert all(len(m.text) <= 4 * _T() + 512 for m in pc.corpus(_T()))


@pytest.mark.parametrize("fasta", [False, True], ids=["fastq", "fasta"])
def test_group_a_hits_every_gather_case(fasta):
    seq, names, leads = set(), set(), set()
    for m in pc.group(_T(), "A", fasta):
        letters, name_bytes = pc.pooled_bytes(m.prefill, m.prefill_fasta)
        leads.add((letters % 16, name_bytes % 16))
        s, n = pc.gather_cases(m.text, m.fasta, letters % 16, name_bytes % 16)
        seq |= s
        names |= n
        width = [n for _, n in pc.entries(m.text, m.fasta)[0]]
        assert 1 <= min(width) and max(width) <= 40
    assert len(pc.ALL_CASES) == 1088
    assert seq == pc.ALL_CASES, sorted(pc.ALL_CASES - seq)[:10]
    assert names == pc.ALL_CASES, sorted(pc.ALL_CASES - names)[:10]
    assert {a for a, _ in leads} == set(range(16)) and {b for _, b in leads} == set(range(16))


def test_group_b_runs_lie_where_they_should():
    T = _T()
    members = pc.group(T, "B")
    assert {m.claims["offset"] for m in members} >= {T - 1, T} and any(T - 40 < m.claims["offset"] < T - 1 for m in members)
    for m in members:
        seq, names = pc.entries(m.text, m.fasta)
        for ents in {"lines": (seq,), "headers": (names,), "both": (seq, names)}[m.claims["run"]]:
            d, run, start = 0, 0, None
            for _, n in ents:                    # the first run of one-byte entries and the output offset it starts at
                if n == 1:
                    start = d if run == 0 else start
                    run += 1
                elif run:
                    break
                d += n
            assert run >= 40 and start == m.claims["offset"], (m.name, run, start)


def test_group_c_feeds_and_sizes_are_where_it_says():
    T = _T()
    members = pc.group(T, "C")
    feeds = {}
    for m in members:
        c = m.claims or {}
        if "feed_at" in c:
            assert m.text[c["feed_at"]] == 0x0A, m.name
            feeds.setdefault(c["feed_at"], set()).add(m.fasta)
        if "size" in c:
            assert len(m.text) == c["size"] and (m.text[-1] == 0x0A) == c["final_feed"] and b"\n\n" not in m.text, m.name
        if "line" in c:
            assert max(n for _, n in pc.lines_of(m.text)) == c["line"] == 3 * T + 1
        if "feeds" in c:
            a, n = c["feeds"]
            assert m.text[a:a + n] == b"\n" * n and n == T + 5
    assert feeds == {p: {True, False} for p in (15, 16, 17, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T - 1, 2 * T)}
    assert {(m.claims["size"], m.claims["final_feed"], m.fasta) for m in members if m.claims and "size" in m.claims} == \
        {(s, f, a) for s in (T - 1, T, T + 1, 2 * T) for f in (True, False) for a in (True, False)}
    tile = next(m for m in members if m.name == "C-tile-of-feeds")
    assert tile.text[T:2 * T] == b"\n" * T                                        # a whole tile of the line table is feeds
    assert sum(m.name.endswith("-crlf") and b"\r\n" in m.text and b"\n" not in m.text.replace(b"\r\n", b"") for m in members) == 2


def test_group_d_holds_every_byte_value(tmp_path):
    in_names, in_letters = set(), set()
    for m in pc.group(_T(), "D"):
        seq, names = pc.entries(m.text, m.fasta)
        for s, n in names:
            in_names |= set(m.text[s:s + n - 1])
        for s, n in seq:
            in_letters |= set(m.text[s:s + n])
        if m.claims:
            assert tuple(_parse(tmp_path, m.text).lengths.tolist()) == m.claims["lengths"]
    assert in_names == set(range(256)) - {0x0A}
    assert in_letters == set(range(256)) - {0x0A, 0x20, 0x09} and {0x00, 0x89, 0x8A, 0xA0} <= in_letters


def test_group_f_blanks_sit_at_every_byte_of_a_vector():
    seen, two_tiles = set(), set()
    for m in pc.group(_T(), "F"):
        assert (m.prefill, m.prefill_fasta) == (pc.GOOD, False)
        c = m.claims
        if not c:
            continue
        lead = pc.pooled_bytes(m.prefill, m.prefill_fasta)[0]
        assert lead == 12

        def place(pos):
            d = lead
            for s, n in pc.entries(m.text, m.fasta)[0]:
                if s <= pos < s + n:
                    where = d + pos - s                                                    # the blank's absolute place in the pool
                    return where, d <= where // 16 * 16 and where // 16 * 16 + 16 <= d + n, s  # ..., its vector comes out of this one line
                d += n

        if "tiles" in c:                                                                   # two blanks in different output tiles
            tiles = tuple(place(p)[0] // _T() for p, _ in m.expectation)
            assert tiles == c["tiles"] and tiles[0] < tiles[1], m.name
            two_tiles.add(tiles)
            continue
        where, whole, s = place(m.expectation[0][0])
        assert where % 16 == c["vector_byte"] and whole == c["whole"], m.name
        if len(m.expectation) == 1:
            seen.add((whole, m.text[m.expectation[0][0]], pc.entries(m.text, m.fasta)[0][0][0] % 4, where % 16))   # (the record's source alignment)
        else:                                                                              # two blanks in ONE vector
            assert len(m.expectation) == 2 and place(m.expectation[1][0])[0] // 16 == where // 16
    assert two_tiles == {(0, 1), (0, 2)}
    for whole in (True, False):
        for blank in (0x20, 0x09):
            assert len({s for w, b, s, q in seen if (w, b) == (whole, blank)}) == 2
            for s in {s for w, b, s, q in seen if (w, b) == (whole, blank)}:
                assert {q for w, b, s2, q in seen if (w, b, s2) == (whole, blank, s)} == set(range(16))


@pytest.mark.parametrize("g", GROUPS)
def test_offences_are_all_listed_and_the_host_parser_agrees(g, tmp_path):
    raises = 0
    for m in pc.group(_T(), g):
        found = pc.scan_offences(m.text, m.fasta, m.long_sequence)
        if m.expectation == pc.PARSABLE:
            assert found == [], m.name
            for text in (m.prefill, m.text):
                if text:
                    _parse(tmp_path, text)
        else:
            assert found == m.expectation and found, m.name
            at, code = pc.reported(found, m.fasta)
            assert (at, code) in found
            if any(c in (pc.BLANK, pc.FASTQ_QUALITY) for _, c in found):
                with pytest.raises(RuntimeError):
                    _parse(tmp_path, m.text)
                raises += 1
    assert (raises > 100) == (g == "F")


def test_the_precedence_rule_on_its_own():
    assert pc.reported([(6, pc.BLANK), (40, pc.FASTQ_PLUS)], False) == (40, pc.FASTQ_PLUS)          # classify stage first
    assert pc.reported([(6, pc.BLANK), (3, pc.LONG)], False) == (3, pc.LONG)
    assert pc.reported([(6, pc.BLANK), (9, pc.LONG)], True) == (6, pc.BLANK)                        # FASTA: both after classify
    assert pc.reported([(26, pc.BLANK), (9, pc.LONG)], True) == (9, pc.LONG)
    assert pc.reported([(20, pc.FASTQ_HEADER), (20, pc.FASTQ_LINES)], False) == (20, pc.FASTQ_LINES)
    assert pc.reported([(90, pc.FASTQ_HEADER), (11, pc.FASTQ_QUALITY)], False) == (11, pc.FASTQ_QUALITY)


@pytest.mark.parametrize("seed", pc.POOL_SEEDS)
def test_group_g_scripts_visit_every_branch(seed, tmp_path):
    ops = pc.pool_script(seed)
    assert len(ops) >= 150
    model, pooled_at_fetch = pc.PoolModel(), []
    for op in ops:
        if op[0] == "append":
            _, text, fasta, rs = op
            assert 1 <= len(rs) <= 40
            host = _parse(tmp_path, text)                    # the model's reads are what the reference makes of the text
            want = pc.as_batch(rs)
            assert host.names == want.names and np.array_equal(host.lengths, want.lengths)
            assert np.array_equal(host.offsets, want.offsets) and np.array_equal(host.bases, want.bases)
            model.append(rs)
        elif op[0] == "take":
            assert 1 <= op[1] <= model.sizes()[0]
            model.take(op[1])
        elif op[0] == "fetch":
            assert op[1] + op[2] <= model.sizes()[0]
            pooled_at_fetch.append((op[1], op[2], model.sizes()[0]))
    assert min(model.branches) >= 5, model.branches
    assert model.doubling >= 3 and model.grown_keeping >= 3, (model.doubling, model.grown_keeping)
    assert model.sizes() == (0, 0, 0)
    assert any(n == 0 and first == 0 and pooled > 0 for first, n, pooled in pooled_at_fetch)
    assert any(n == 0 and first == pooled and pooled > 0 for first, n, pooled in pooled_at_fetch)
    assert any(0 < first and 0 < n and first + n < pooled for first, n, pooled in pooled_at_fetch)


@pytest.mark.parametrize("g", GROUPS)
def test_parse_dump_equals_parse_reads(g, tmp_path):
    """The form of test_parse_dump_is_unchanged (tests/test_device_parse_cpu.py) on the corpus."""
    exe = hipbuild.build_host()
    members = [m for m in pc.group(_T(), g) if pc.dump_safe(m)]
    assert members or g == "D"
    path = str(tmp_path / "in.txt")
    for m in members:
        with open(path, "wb") as f:
            f.write(m.text)
        r = subprocess.run([exe, "parse-dump", path, "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                           env=dict(os.environ, KASA_READ_BLOCK="1500", KASA_PARSE_CHUNK="400"))
        assert r.returncode == 0, (m.name, r.stderr[-400:])
        ref = reads.parse_reads(path)
        want = "".join(f"{ref.names[i]}\t{int(ref.lengths[i])}\t{bytes(ref.bases[int(ref.offsets[i]):int(ref.offsets[i + 1])]).decode('latin-1')}\n" for i in range(ref.n))
        streamed = r.stdout.decode("latin-1").split("== streamed\n")[1]
        head, body = streamed.split("\n", 1)
        assert head.startswith("protein=%d" % (1 if ref.protein else 0)) and body == want, m.name
