"""The device parser (kasa_parse_*, kasa_amd/csrc/kasa_parse.h) against `reads.parse_reads` on the same bytes: lengths, name
offsets, names, base offsets and bases exactly equal; chunks that are not in the form the device takes leave the pool as it
was; reads taken out of the pool score bit-equal to the host-parsed ones."""
import ctypes as C

import numpy as np
import pytest

from kasa_amd import capi, reads

pytestmark = pytest.mark.gpu

LENGTHS = (1, 20, 36, 37, 150, 151, 300)


def _host(tmp_path, text: bytes):
    p = tmp_path / "in.txt"
    p.write_bytes(text)
    return str(p), reads.parse_reads(str(p))


def _assert_equal(got, host):
    lengths, name_off, names, off, bases = got
    blob = "".join(host.names).encode("latin-1")
    want_name_off = np.concatenate([[0], np.cumsum([len(n) for n in host.names])]).astype(np.uint64)
    assert np.array_equal(lengths, host.lengths)
    assert np.array_equal(name_off, want_name_off)
    assert names.tobytes() == blob
    assert np.array_equal(off, host.offsets)
    assert np.array_equal(bases, host.bases)


def _pool_vs_host(tmp_path, text: bytes, fasta: bool, chunks=None):
    assert capi.device_count() > 0, "no HIP device visible: the device parser needs a real MI355X"
    path, host = _host(tmp_path, text)
    ps = capi.Parser(0)
    try:
        total = 0
        for a, b in chunks or [(0, len(text))]:
            n, ok = ps.append(text[a:b], fasta)
            assert ok, ps.status()
            total += n
        assert total == host.n
        assert ps.sizes() == (host.n, int(host.offsets[-1]), sum(len(n) for n in host.names))
        _assert_equal(ps.fetch(), host)
        if host.n > 2:                                    # a range in the middle, rebased
            sub = host.slice(1, host.n - 1)
            _assert_equal(ps.fetch(1, host.n - 2), sub)
    finally:
        ps.close()
    # ... and the file-level entry point
    dev = reads.parse_reads_device(path, 0)
    assert dev.names == host.names and dev.fasta == host.fasta and dev.protein == host.protein
    assert np.array_equal(dev.lengths, host.lengths) and np.array_equal(dev.offsets, host.offsets) and np.array_equal(dev.bases, host.bases)
    return host


def _fastq_text(target_bytes: int, seed: int, eol: bytes = b"\n"):
    """Records with lengths from LENGTHS: quality lines that start with '@' and '+', '+' lines that repeat the name, headers
    with spaces, '>' and '@', letters N and lower case."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)
    out, starts, size, i = [], [], 0, 0
    while size < target_bytes:
        L = LENGTHS[i % len(LENGTHS)] if i < 2 * len(LENGTHS) else int(rng.choice(LENGTHS))
        seq = letters[rng.integers(0, letters.shape[0], L)].tobytes()
        qual = bytes(rng.integers(33, 74, L).astype(np.uint8))
        if i % 3 == 0:
            qual = b"@" + qual[1:]
        if i % 3 == 1:
            qual = b"+" + qual[1:]
        name = (b"read%d" % i) + (b" 1:N:0 >x @y" if i % 4 == 0 else b"")
        plus = b"+" + (name if i % 5 == 0 else b"")
        rec = b"@" + name + eol + seq + eol + plus + eol + qual + eol
        starts.append(size)
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out), starts


def test_fastq_one_record_no_line_feed(tmp_path):
    _pool_vs_host(tmp_path, b"@r0 first\nACGTNNacgt\n+\nIIIIIIIIII", False)


def test_fastq_three_records(tmp_path):
    _pool_vs_host(tmp_path, b"@a\nACGT\n+\nIIII\n@b x\nA\n+b x\n@\n@c\nGGGTTTAAACCC\n+\n+IIIIIIIIIII\n", False)


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_fastq_three_tiles(tmp_path, eol):
    T = capi.parse_tile_bytes()
    text, _ = _fastq_text(3 * T, 5, eol)
    assert len(text) > 3 * T
    _pool_vs_host(tmp_path, text, False)


def _fasta_text(T: int):
    rng = np.random.default_rng(11)

    def seq(n):
        return np.frombuffer(b"ACGTNacgt", dtype=np.uint8)[rng.integers(0, 9, n)].tobytes()

    def wrap(s, w=60):
        return b"\n".join(s[i:i + w] for i in range(0, len(s), w)) + b"\n"

    parts = [b">one line\n" + wrap(seq(45)),
             b"\n",                                           # an empty line between records
             b">two lines | x > y\n" + wrap(seq(100)),
             b">\n" + wrap(seq(61)),                          # a header that is '>' alone
             b">empty inside\n" + seq(60) + b"\n\n" + seq(60) + b"\n\n\n" + seq(7) + b"\n",
             b">no sequence\n",
             b">spans tiles\n" + wrap(seq(2 * T + 1234)),
             b"\n\n",
             b">single line\n" + seq(2 * T + 77) + b"\n",
             b">last\n" + wrap(seq(130))]
    return b"".join(parts)


def test_fasta_wrapped_and_long_lines(tmp_path):
    T = capi.parse_tile_bytes()
    host = _pool_vs_host(tmp_path, _fasta_text(T), True)
    assert host.n == 8 and host.names[2] == " " and int(host.lengths[3]) == 127 + 3 and int(host.lengths[4]) == 0


def test_fasta_no_trailing_line_feed_and_chunks(tmp_path):
    T = capi.parse_tile_bytes()
    text = _fasta_text(T)[:-1]
    cut1, cut2 = text.index(b">two lines"), text.index(b">single line")
    _pool_vs_host(tmp_path, text, True, chunks=[(0, cut1), (cut1, cut2), (cut2, len(text))])


def test_appends_and_takes_that_do_not_line_up(tmp_path):
    """Three chunks in, batches of (1, n - 2, 1) out through kasa_parse_take: scores and profile of every batch bit-equal to
    run_batch on the host-parsed reads."""
    from tests.test_gpu_parity import synthetic_world
    assert capi.device_count() > 0
    ix, batch = synthetic_world(29, 4, 3000, 41)
    recs = []
    for r in range(batch.n):
        s = batch.bases[int(batch.offsets[r]):int(batch.offsets[r + 1])].tobytes()
        recs.append(b"@" + batch.names[r].strip().encode() + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")
    text = b"".join(recs)
    _, host = _host(tmp_path, text)
    n = host.n
    assert n == 41
    c1, c2 = sum(len(x) for x in recs[:7]), sum(len(x) for x in recs[:30])
    dix = capi.DeviceIndex(ix)
    dev, ref = capi.Context(dix), capi.Context(dix)
    ps = capi.Parser(0)
    try:
        # one chunk, one read out, then the other two chunks behind what is left
        assert ps.append(text[:c1], False) == (7, True)
        first = 0
        pending = [(1, None), (n - 2, [(c1, c2), (c2, len(text))]), (1, None)]
        for size, more in pending:
            for a, b in more or []:
                assert ps.append(text[a:b], False)[1]
            before = ps.sizes()[0]
            ps.take(dev, size)
            assert ps.sizes()[0] == before - size
            dev.encode(); dev.sort_and_range(False); dev.lookup_score(True, False)
            sub = host.slice(first, first + size)
            ref.run_batch(sub.bases, sub.offsets)
            for x, y in zip(dev.scores(), ref.scores()):
                assert x.tobytes() == y.tobytes()
            assert np.array_equal(dev.profile_limbs(), ref.profile_limbs())
            first += size
        assert first == n and ps.sizes() == (0, 0, 0)
        with pytest.raises(RuntimeError, match="pooled"):
            ps.take(dev, 1)
    finally:
        ps.close(); dev.close(); ref.close(); dix.close()


GOOD = b"@g0\nACGTACGT\n+\nIIIIIIII\n@g1\nTTTT\n+\nIIII\n"
NOT_PARSABLE = {
    "two-line sequence": (b"@a\nACGT\nACGT\n+\nIIIIIIII\n", False, None),
    "quality shorter": (b"@a\nACGT\n+\nIII\n@b\nAC\n+\nII\n", False, 4),
    "quality longer": (b"@a\nACGT\n+\nIIIII\n@b\nAC\n+\nII\n", False, 4),
    "empty sequence line": (b"@a\n\n+\n\n@b\nAC\n+\nII\n", False, 5),
    "tab in a sequence": (b"@a\nAC\tGT\n+\nIIIII\n", False, 6),
    "tab in a FASTA sequence": (b">a\nACGT\nAC\tGT\n", True, 6),
    "space far into a sequence": (b"@a\n" + b"A" * 1500 + b" " + b"C" * 99 + b"\n+\n" + b"I" * 1600 + b"\n", False, 6),
    "long record": (b"@a\n" + b"A" * 2000 + b"\n+\n" + b"I" * 2000 + b"\n", False, 7),
    "long FASTA record": (b">a\n" + (b"A" * 50 + b"\n") * 40, True, 7),
    "no '@'": (b"@a\nAC\n+\nII\nb\nAC\n+\nII\n", False, 2),
    "no '+'": (b"@a\nAC\n-\nII\n", False, 3),
}


@pytest.mark.parametrize("case", list(NOT_PARSABLE), ids=[c.replace(" ", "-") for c in NOT_PARSABLE])
def test_not_parsable_leaves_the_pool_unchanged(case, tmp_path):
    assert capi.device_count() > 0
    text, fasta, code = NOT_PARSABLE[case]
    ps = capi.Parser(0, long_sequence=2000)
    try:
        assert ps.append(GOOD, False) == (2, True)
        before, kept = ps.sizes(), ps.fetch()
        n, ok = ps.append(text, fasta)
        assert (n, ok) == (0, False)
        assert ps.status()[0] != 0 and (code is None or ps.status()[0] == code)
        assert ps.sizes() == before == (2, 12, 6)
        for x, y in zip(ps.fetch(), kept):
            assert np.array_equal(x, y)
        # one letter fewer than the limit is taken, behind the reads that stayed
        ok_text = b"@z\n" + b"A" * 1999 + b"\n+\n" + b"I" * 1999 + b"\n"
        assert ps.append(ok_text, False) == (1, True)
        lengths, _, names, off, bases = ps.fetch()
        assert lengths.tolist() == [9, 5, 2000] and names.tobytes() == b"g0 g1 z " and off.tolist() == [0, 8, 12, 2011]
        assert bases.tobytes() == b"ACGTACGTTTTT" + b"A" * 1999
    finally:
        ps.close()


def test_context_on_another_device_is_refused():
    if capi.device_count() < 2:
        pytest.skip("one device visible")
    from tests.test_gpu_parity import synthetic_world
    ix, _ = synthetic_world(29, 4, 3000, 1)
    dix = capi.DeviceIndex(ix, device=1)
    ctx = capi.Context(dix)
    ps = capi.Parser(0)
    try:
        assert ps.append(GOOD, False) == (2, True)
        rc = capi.lib().kasa_parse_take(ps.h, ctx.h, C.c_uint64(1))
        assert rc == 1                                     # KASA_E_ARG
        assert b"device" in capi.lib().kasa_last_error()
        assert ps.sizes()[0] == 2
    finally:
        ps.close(); ctx.close(); dix.close()
