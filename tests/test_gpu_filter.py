"""--filter on the device below the driver: the record text a pool keeps (kasa_pool_keep_records), the split by flags
(kasa_filter_split, kasa_batch_filter) and its BGZF form, each against tests/filter_spec.py.  T = kasa_parse_tile_bytes()."""
import gzip
import os

import numpy as np
import pytest

from kasa_amd import capi, formats, reads, report
from tests import filter_spec as spec
from tests.test_bgzf_cpu import PAIRS_DIR, check_stream

pytestmark = pytest.mark.gpu


def _seq(rng, n):
    return np.frombuffer(b"ACGTNacgt", dtype=np.uint8)[rng.integers(0, 9, n)].tobytes()


def _fastq(n_reads, seed, eol=b"\n", plus_name=False):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_reads):
        L = int(rng.integers(1, 200))
        name = b"r%d" % i + (b" 1:N:0 x" if i % 3 == 0 else b"")
        out.append(b"@" + name + eol + _seq(rng, L) + eol + b"+" + (name if plus_name and i % 2 == 0 else b"") + eol + bytes(rng.integers(33, 74, L).astype(np.uint8)) + eol)
    return out


def _fasta_corpus(T):
    rng = np.random.default_rng(3)

    def wrap(s, w=60):
        return b"\n".join(s[i:i + w] for i in range(0, len(s), w)) + b"\n"

    return [b">one line\n" + wrap(_seq(rng, 45)),
            b"\n",                                                # an empty line between records (belongs to the record before)
            b">multi-line | x > y\n" + wrap(_seq(rng, 400)),
            b">\n" + wrap(_seq(rng, 61)),                          # a header of one character
            b">empty inside\n" + _seq(rng, 60) + b"\n\n" + _seq(rng, 60) + b"\n\n\n" + _seq(rng, 7) + b"\n",
            b">header alone\n",
            b">crlf\r\n" + _seq(rng, 30) + b"\r\n\r\n" + _seq(rng, 31) + b"\r\n",      # "\r" alone is a line
            b">spans tiles\n" + wrap(_seq(rng, 2 * T + 1234)),
            b"\n\n",
            b">single line\n" + _seq(rng, 2 * T + 77) + b"\n",
            b">last\n" + wrap(_seq(rng, 130))]


def _check_pool(ps, recs, first=0):
    off, text = ps.fetch_records(first)
    assert text == b"".join(recs[first:])
    assert np.array_equal(off, spec.offsets(recs[first:]))


def _append_all(ps, parts, fasta):
    for part in parts:
        n, ok = ps.append(part, fasta)
        assert ok, ps.status()


CASES = {
    "fastq": (lambda T: [b"".join(_fastq(120, 1))], False),
    "fastq-chunks": (lambda T: [b"".join(_fastq(50, 2)[i:i + 3]) for i in range(0, 50, 3)], False),
    "fastq-plus-name": (lambda T: [b"".join(_fastq(40, 3, plus_name=True))], False),
    "fastq-crlf": (lambda T: [b"".join(_fastq(60, 4, eol=b"\r\n"))], False),
    "fastq-no-eol": (lambda T: [b"".join(_fastq(9, 5))[:-1]], False),
    "fasta": (lambda T: [b"".join(_fasta_corpus(T))], True),
    "fasta-no-eol": (lambda T: [b"".join(_fasta_corpus(T))[:-1]], True),
    "fasta-chunks": (lambda T: [b"".join(_fasta_corpus(T)[0:2]), b"".join(_fasta_corpus(T)[2:5]), b"".join(_fasta_corpus(T)[5:9]), b"".join(_fasta_corpus(T)[9:])], True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_records_kept(case):
    assert capi.device_count() > 0, "no HIP device visible: the device parser needs a real MI355X"
    make, fasta = CASES[case]
    parts = make(capi.parse_tile_bytes())
    recs = [r for part in parts for r in spec.records(part, fasta)]
    ps, plain = capi.Parser(0), capi.Parser(0)
    try:
        ps.keep_records()
        _append_all(ps, parts, fasta)
        _append_all(plain, parts, fasta)
        assert ps.sizes()[0] == len(recs)
        _check_pool(ps, recs)
        if len(recs) > 2:                                          # a range in the middle, rebased
            off, text = ps.fetch_records(1, len(recs) - 2)
            assert text == b"".join(recs[1:-1]) and np.array_equal(off, spec.offsets(recs[1:-1]))
        for x, y in zip(ps.fetch(), plain.fetch()):                # keeping records changes nothing else
            assert np.array_equal(x, y)
    finally:
        ps.close(); plain.close()


def test_keep_is_refused_on_a_pool_with_reads_and_fetch_without_keep():
    ps = capi.Parser(0)
    try:
        with pytest.raises(RuntimeError, match="keeps no records"):
            ps.fetch_records()
        text = b"".join(_fastq(5, 6))
        assert ps.append(text, False) == (5, True)
        before = [x.copy() for x in ps.fetch()]
        assert capi.lib().kasa_pool_keep_records(ps.h, 1) == 4    # KASA_E_STATE
        with pytest.raises(RuntimeError, match="must be empty"):
            ps.keep_records()
        assert capi.lib().kasa_pool_fetch_records(ps.h, 0, 0, None, None) == 4
        for x, y in zip(ps.fetch(), before):                       # with keep off, fetch gives what it gave
            assert np.array_equal(x, y)
    finally:
        ps.close()


def test_records_through_take_compaction_and_a_refused_chunk():
    from tests.test_gpu_parity import synthetic_world
    ix, _ = synthetic_world(29, 4, 3000, 1)
    dix = capi.DeviceIndex(ix)
    ctx = capi.Context(dix)
    ps = capi.Parser(0, long_sequence=2000)
    try:
        ps.keep_records()
        first, second = _fastq(40, 7), _fastq(25, 8, eol=b"\r\n")
        assert ps.append(b"".join(first), False) == (40, True)
        ps.take(ctx, 33)                                           # most of the pool leaves: the next append moves the remainder
        _check_pool(ps, first[33:])
        flags = np.arange(33, dtype=np.uint8) % 3 == 0
        assert ctx.filter(flags) == spec.split(first[:33], flags)
        assert ps.append(b"".join(second), False) == (25, True)
        recs = first[33:] + second
        _check_pool(ps, recs)
        assert ps.append(b"@a\nAC\tGT\n+\nIIIII\n", False) == (0, False)    # refused: pool and records as before
        assert ps.append(b"@a\n" + b"A" * 2000 + b"\n+\n" + b"I" * 2000 + b"\n", False) == (0, False)
        assert ps.sizes()[0] == len(recs)
        _check_pool(ps, recs)
        ps.take(ctx, 5)
        assert ctx.filter(np.ones(5, dtype=np.uint8)) == spec.split(recs[:5], [1] * 5)
        _check_pool(ps, recs[5:])
        ps.take(ctx, len(recs) - 5)
        assert ps.sizes() == (0, 0, 0)
        third = _fastq(3, 9)
        assert ps.append(b"".join(third), False) == (3, True)       # an empty pool starts over
        _check_pool(ps, third)
    finally:
        ps.close(); ctx.close(); dix.close()


@pytest.mark.parametrize("fasta", [False, True], ids=["fastq", "fasta"])
def test_records_through_append_bgzf_with_a_carry(fasta):
    T = capi.parse_tile_bytes()
    text = b"".join(_fasta_corpus(T)) if fasta else b"".join(_fastq(60, 10))
    recs = spec.records(text, fasta)
    cut = len(b"".join(recs[:len(recs) // 2])) + 7                 # inside a record: its head is carried to the second span
    ps = capi.Parser(0)
    try:
        ps.keep_records()
        n1, ok, _, carry = ps.append_bgzf(formats.bgzf_compress(text[:cut]), fasta)
        assert ok and carry > 0 and 0 < n1 < len(recs)
        with pytest.raises(RuntimeError, match="must be empty"):   # bytes are carried
            ps.keep_records(False)
        _check_pool(ps, recs[:n1])
        n2, ok, _, carry = ps.append_bgzf(formats.bgzf_compress(text[cut:]), fasta, final=True)
        assert ok and carry == 0 and n1 + n2 == len(recs)
        _check_pool(ps, recs)
    finally:
        ps.close()


# ---- the split on its own ----
def _records_of_sizes(sizes, seed=0):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(33, 127, s - 1).astype(np.uint8)) + b"\n" for s in sizes]


def _check_split(recs, flags, sides=(0, 1)):
    flags = np.asarray(flags, dtype=np.uint8)
    want = spec.split(recs, flags)
    blob, off = b"".join(recs), spec.offsets(recs)
    for side in sides:
        got, n = capi.filter_split(0, blob, off, flags, side)
        assert n == want[2 + side]
        assert got == want[side], (side, len(got), len(want[side]))


def _flag_patterns(n):
    runs = {}
    for run in (1, 2, 63, 64, 65):
        runs["runs%d" % run] = [(i // run) & 1 for i in range(n)]
    runs.update({"all0": [0] * n, "all1": [1] * n, "first": [1] + [0] * (n - 1), "last": [0] * (n - 1) + [1]})
    return runs


ORDERS = {"up": lambda s, rng: sorted(s), "down": lambda s, rng: sorted(s, reverse=True), "mixed": lambda s, rng: list(rng.permutation(s)),
          "mixed2": lambda s, rng: list(rng.permutation(s))}


@pytest.mark.parametrize("order", list(ORDERS))
def test_split_sizes_2_to_40_under_every_flag_pattern(order):
    """Sizes 2..40, eight times over: under the patterns a record starts at every alignment of source and destination."""
    rng = np.random.default_rng(len(order))
    sizes = [int(s) for s in ORDERS[order](list(range(2, 41)) * 8, rng)]
    recs = _records_of_sizes(sizes, 1)
    starts = {(int(a) % 16) for a in spec.offsets(recs)[:-1]}
    assert starts == set(range(16))
    for name, flags in _flag_patterns(len(recs)).items():
        _check_split(recs, flags)
        dst = spec.offsets([r for r, f in zip(recs, flags) if f])
        if name.startswith("runs"):
            assert len({int(a) % 16 for a in dst[:-1]}) == 16, name


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("d1", [-1, 0, 1])
@pytest.mark.parametrize("d2", [-1, 0, 1])
def test_split_junction_at_a_tile_edge(side, d1, d2):
    """Records of one side end at output bytes T + d1 and 2 T + d2; the other side's lie between them."""
    T = capi.parse_tile_bytes()
    mine = [17, T + d1 - 17, 23, (2 * T + d2) - (T + d1) - 23, 9, 40, 2]
    other = [5, 11, 3, 2 * T + 1, 16, 2, 33]
    sizes, flags = [], []
    for a, b in zip(mine, other):
        sizes += [a, b]; flags += [side, side ^ 1]
    recs = _records_of_sizes(sizes, 2)
    ends = np.cumsum(mine)
    assert T + d1 in ends and 2 * T + d2 in ends
    _check_split(recs, flags)


def test_split_a_long_record_one_read_no_read_and_the_capacity():
    T = capi.parse_tile_bytes()
    sizes = [7, 3, 2 * T + 77, 5, 12, 2 * T + 77, 4]
    recs = _records_of_sizes(sizes, 3)
    for flags in ([0, 1, 1, 0, 0, 0, 1], [1, 0, 0, 1, 1, 1, 0], [0] * 7, [1] * 7):
        _check_split(recs, flags)
    one = _records_of_sizes([33], 4)
    _check_split(one, [0]); _check_split(one, [1])
    two = _records_of_sizes([2], 4)
    _check_split(two, [1])
    assert capi.filter_split(0, b"", np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint8), 0) == (b"", 0)
    assert capi.filter_split(0, b"", np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint8), 1) == (b"", 0)
    blob, off, flags = b"".join(recs), spec.offsets(recs), np.array([0, 1, 1, 0, 0, 0, 1], dtype=np.uint8)
    need = len(spec.split(recs, flags)[1])
    assert len(capi.filter_split(0, blob, off, flags, 1, cap=need)[0]) == need
    with pytest.raises(RuntimeError, match="the destination takes"):
        capi.filter_split(0, blob, off, flags, 1, cap=need - 1)
    with pytest.raises(RuntimeError, match="side is"):
        capi.filter_split(0, blob, off, flags, 2)


# ---- through a context ----
@pytest.fixture(scope="module")
def world():
    assert capi.device_count() > 0
    ix = formats.load_index(os.path.join(PAIRS_DIR, "idx"), os.path.join(PAIRS_DIR, "content.txt"))
    path = os.path.join(PAIRS_DIR, "reads.fastq")
    with open(path, "rb") as f:
        text = f.read()
    batch = reads.parse_reads(path)
    dix = capi.DeviceIndex(ix)
    ctx = capi.Context(dix, 12, 7, 3)
    ctx.set_taxa_text(ix.content.taxids, ix.content.names)
    yield ix, text, batch, ctx
    ctx.close(); dix.close()


def _text_of_batch(ix, batch, ctx):
    ctx.encode(); ctx.sort_and_range(False); ctx.lookup_score(True, False)
    den, rclass = report.rank_denominators(ix.freq_at(12), batch.lengths, ix.K, False)
    best = np.array([report.best_score(int(L), 12, 7, 3, False) for L in np.unique(batch.lengths)], dtype=np.float32)
    ctx.rank(den, rclass, 0.0, 100)
    return ctx.text("jsonl", 100, 0, batch.names, batch.lengths, best)


def test_context_filter(world):
    ix, text, batch, ctx = world
    recs = spec.records(text, False)
    assert len(recs) == batch.n
    ps = capi.Parser(0)
    try:
        ps.keep_records()
        assert ps.append(text, False) == (batch.n, True)
        ps.take(ctx, batch.n)
        nb, nr = (capi.C.c_uint64 * 2)(), (capi.C.c_uint64 * 2)()
        assert capi.lib().kasa_batch_filter(ctx.h, None, 3, 0, nb, nr) == 4      # KASA_E_STATE: no flags yet
        _, _, flags = _text_of_batch(ix, batch, ctx)
        assert 0 < int(flags.sum()) < batch.n, "the golden reads have both kinds"
        want = spec.split(recs, flags)
        assert ctx.filter() == want
        assert ctx.filter(flags) == want                          # the same flags as a host array
        other = (np.arange(batch.n) % 5 == 0).astype(np.uint8)
        assert ctx.filter(other) == spec.split(recs, other)
        assert ctx.filter(sides=1) == (want[0], b"", want[2], 0)    # each side alone
        assert ctx.filter(sides=2) == (b"", want[1], 0, want[3])
        assert ctx.filter(sides=0) == (b"", b"", 0, 0)
        assert ctx.filter(np.zeros(batch.n, dtype=np.uint8)) == (b"".join(recs), b"", batch.n, 0)
        for code in (capi.BGZF_FIXED, capi.BGZF_DYNAMIC):
            ctx.set_bgzf_code(code)
            zc, zd, nc, nd = ctx.filter(gzip=True)
            assert (nc, nd) == want[2:]
            for stream, data in ((zc, want[0]), (zd, want[1])):
                check_stream(stream, data, device=True)             # every member at most 65536 bytes, CRC-32 and ISIZE
                assert gzip.decompress(stream + formats.BGZF_EOF) == data
                assert stream == capi.bgzf_deflate(0, data, code)   # what kasa_bgzf_deflate writes for the same bytes
        ctx.set_bgzf_code(capi.BGZF_FIXED)
        with pytest.raises(RuntimeError, match="beyond"):
            capi._check(capi.lib().kasa_batch_filter_fetch_range(ctx.h, 0, None, 0, 1 << 40))
    finally:
        ps.close()


def test_context_without_records_is_refused(world):
    ix, text, batch, ctx = world
    ctx.upload(batch.bases, batch.offsets)
    _, _, flags = _text_of_batch(ix, batch, ctx)
    nb, nr = (capi.C.c_uint64 * 2)(), (capi.C.c_uint64 * 2)()
    assert capi.lib().kasa_batch_filter(ctx.h, None, 3, 0, nb, nr) == 4          # KASA_E_STATE
    with pytest.raises(RuntimeError, match="no records"):
        ctx.filter(flags)
    ps = capi.Parser(0)                                            # ... nor from a pool that keeps none
    try:
        assert ps.append(text, False) == (batch.n, True)
        ps.take(ctx, batch.n)
        with pytest.raises(RuntimeError, match="no records"):
            ctx.filter(flags)
    finally:
        ps.close()
