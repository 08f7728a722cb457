"""Two device pools taken as pairs (kasa_pair_take / kasa_pair_fetch, kasa_amd/csrc/kasa_parse.h) against `reads.parse_pairs`
on the same two texts: lengths, name offsets, names, the 2n + 1 sequence offsets and the interleaved bases exactly equal, whole
and for a rebased range in the middle; pairs taken out of the pools score bit-equal to kasa_batch_upload_segments of the
host-parsed pairs.

One case departs from its description: a pair whose BOTH mates are empty needs an empty read in file 2, and FASTQ cannot spell
one that the device parser takes (an empty sequence line is KASA_PARSE_EMPTY_LINE), so that one pair list has FASTA on both
sides; every other zero-length case keeps FASTQ as file 2."""
import os

import numpy as np
import pytest

from kasa_amd import capi, reads
from tests import helpers

pytestmark = pytest.mark.gpu

_RNG = np.random.default_rng(2024)
_LETTERS = np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)


def _seq(n: int) -> bytes:
    return _LETTERS[_RNG.integers(0, _LETTERS.shape[0], n)].tobytes()


def _fastq(records) -> bytes:
    return b"".join(b"@" + name + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for name, s in records)


def _fasta(records) -> bytes:
    return b"".join(b">" + name + b"\n" + (s + b"\n" if s else b"") for name, s in records)


def _mates(lengths, tag: bytes, long_name_every: int = 0):
    return [(tag + b"%d" % i + (b" " + b"x" * 200 if long_name_every and i % long_name_every == 0 else b""), _seq(n)) for i, n in enumerate(lengths)]


def _host(tmp_path, t1: bytes, t2: bytes):
    p1, p2 = tmp_path / "m1.txt", tmp_path / "m2.txt"
    p1.write_bytes(t1)
    p2.write_bytes(t2)
    return str(p1), str(p2), reads.parse_pairs(str(p1), str(p2))


def _assert_pairs(got, host):
    lengths, name_off, names, off, bases = got
    assert np.array_equal(lengths, host.lengths)
    assert np.array_equal(name_off, np.concatenate([[0], np.cumsum([len(n) for n in host.names])]).astype(np.uint64))
    assert names.tobytes() == "".join(host.names).encode("latin-1")
    assert off.shape[0] == 2 * host.n + 1 and np.array_equal(off, host.offsets)
    assert np.array_equal(bases, host.bases)


def _pools_vs_host(tmp_path, t1: bytes, t2: bytes):
    assert capi.device_count() > 0, "no HIP device visible: the device parser needs a real MI355X"
    p1, p2, host = _host(tmp_path, t1, t2)
    a, b = capi.Parser(0), capi.Parser(0)
    try:
        assert a.append(t1, t1[:1] == b">")[1], a.status()
        assert b.append(t2, t2[:1] == b">")[1], b.status()
        assert a.sizes()[0] == b.sizes()[0] == host.n
        _assert_pairs(capi.pair_fetch(a, b), host)
        if host.n > 2:                                        # a range in the middle, rebased to its first pair
            _assert_pairs(capi.pair_fetch(a, b, 1, host.n - 2), host.slice(1, host.n - 1))
        assert a.sizes()[0] == b.sizes()[0] == host.n         # a fetch leaves the pools as they are
    finally:
        a.close(); b.close()
    dev = reads.parse_pairs_device(p1, p2, 0)
    assert dev.names == host.names and dev.protein == host.protein
    for x, y in ((dev.lengths, host.lengths), (dev.offsets, host.offsets), (dev.bases, host.bases), (dev.seg_read, host.seg_read)):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    return host


# ---- tiny ----
def test_three_pairs_of_one_letter(tmp_path):
    host = _pools_vs_host(tmp_path, b"@a/1\nA\n+\nI\n@b/1\nC\n+\nI\n@c/1\nG\n+\nI\n", b"@a/2\nT\n+\nI\n@b/2\nN\n+\nI\n@c/2\na\n+\nI\n")
    assert host.bases.tobytes() == b"ATCNGa" and host.names[1] == "b/1 b/2 "


def test_one_pair_without_the_last_line_feed(tmp_path):
    host = _pools_vs_host(tmp_path, b"@only/1 x\nACGTNNacgt\n+\nIIIIIIIIII\n", b"@only/2 y\nTTGCA\n+\nIIIII")
    assert host.n == 1 and host.offsets.tolist() == [0, 10, 15]


# ---- lengths: the vector and the byte path, every source alignment mod 4 on both sides ----
def test_every_combination_of_lengths(tmp_path):
    T = capi.parse_tile_bytes()
    L = (1, 15, 16, 17, 31, 32, 33, 150, 151)
    combos = [(x, y) for x in L for y in L]
    combos = combos + combos[::-1]                            # the second round meets other alignments
    host = _pools_vs_host(tmp_path, _fastq(_mates([c[0] for c in combos], b"m", 7)), _fastq(_mates([c[1] for c in combos], b"w", 5)))
    assert int(host.offsets[-1]) > 3 * T and sum(len(n) for n in host.names) > T


# ---- zero-length mates ----
ZERO = {
    "first": [(0, 20), (33, 16), (150, 151)],
    "last": [(150, 151), (33, 16), (0, 20)],
    "two-in-a-row": [(17, 31), (0, 16), (0, 33), (40, 1)],
    "all-of-file-1": [(0, 5), (0, 16), (0, 70)],
}


@pytest.mark.parametrize("case", list(ZERO), ids=list(ZERO))
def test_fasta_records_without_sequence_lines(case, tmp_path):
    pairs = ZERO[case]
    host = _pools_vs_host(tmp_path, _fasta(_mates([p[0] for p in pairs], b"f")), _fastq(_mates([p[1] for p in pairs], b"q")))
    assert [int(host.offsets[2 * r + 1] - host.offsets[2 * r]) for r in range(host.n)] == [p[0] for p in pairs]


@pytest.mark.parametrize("pairs", [[(0, 0), (20, 31)], [(20, 31), (0, 0)], [(16, 16), (0, 0), (0, 0), (5, 0), (0, 7)], [(0, 0)]], ids=["first", "last", "middle", "alone"])
def test_both_mates_empty(pairs, tmp_path):
    """(FASTA on both sides: see the module text)"""
    host = _pools_vs_host(tmp_path, _fasta(_mates([p[0] for p in pairs], b"f")), _fasta(_mates([p[1] for p in pairs], b"g")))
    assert int(host.offsets[-1]) == sum(a + b for a, b in pairs)


# ---- tile edges ----
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("kind", ["mate", "pair"])
def test_a_junction_at_a_tile_edge(kind, delta, tmp_path):
    """the junction between the mates of a pair / between two pairs at output byte k T + delta, k = 1 and 2"""
    T = capi.parse_tile_bytes()
    pairs, total, at = [], 0, []
    for k in (1, 2):
        target = k * T + delta
        while target - total > 700:                           # ordinary pairs up to the neighbourhood of the edge
            pairs.append((150, 151)); total += 301
        room = target - total                                 # 98 .. 700 letters to the junction
        if kind == "mate":
            pairs.append((room, 40)); at.append(2 * len(pairs) - 1); total += room + 40
        else:
            pairs.append((room - 50, 50)); at.append(2 * len(pairs)); total += room
    pairs.append((33, 17))
    host = _pools_vs_host(tmp_path, _fastq(_mates([p[0] for p in pairs], b"m")), _fastq(_mates([p[1] for p in pairs], b"w")))
    assert [int(host.offsets[s]) for s in at] == [T + delta, 2 * T + delta]


def test_a_mate_over_whole_tiles_and_a_ragged_total(tmp_path):
    T = capi.parse_tile_bytes()
    pairs = [(10, 2 * T + 77), (5, 7)]
    host = _pools_vs_host(tmp_path, _fastq(_mates([p[0] for p in pairs], b"m")), _fastq(_mates([p[1] for p in pairs], b"w")))
    assert int(host.offsets[-1]) == 2 * T + 99 and int(host.offsets[-1]) % 16 != 0


# ---- pool states ----
@pytest.fixture(scope="module")
def world():
    """41 synthetic pairs of one index's reads: read 2r is mate 1 of pair r, read 2r + 1 its mate 2 (cut to 100 letters)."""
    from tests.test_gpu_parity import synthetic_world
    assert capi.device_count() > 0
    ix, batch = synthetic_world(29, 4, 3000, 82)
    rec1, rec2 = [], []
    for r in range(41):
        s1 = batch.bases[int(batch.offsets[2 * r]):int(batch.offsets[2 * r + 1])].tobytes()
        s2 = batch.bases[int(batch.offsets[2 * r + 1]):int(batch.offsets[2 * r + 2])].tobytes()[:100]
        rec1.append(_fastq([(b"p%d/1" % r, s1)]))
        rec2.append(_fastq([(b"p%d/2" % r, s2)]))
    return ix, rec1, rec2


def _scores_equal(dev, ref, sub):
    dev.encode(); dev.sort_and_range(False); dev.lookup_score(True, False)
    ref.run_batch(sub.bases, sub.offsets, seg_read=sub.seg_read, n_reads=sub.n)
    for x, y in zip(dev.scores(), ref.scores()):
        assert x.tobytes() == y.tobytes()
    assert np.array_equal(dev.profile_limbs(), ref.profile_limbs())


def test_pools_that_drift_takes_and_compaction(world, tmp_path):
    ix, rec1, rec2 = world
    _, _, host = _host(tmp_path, b"".join(rec1), b"".join(rec2))
    n = host.n
    assert n == 41
    dix = capi.DeviceIndex(ix)
    dev, ref = capi.Context(dix), capi.Context(dix)
    a, b = capi.Parser(0), capi.Parser(0)
    text = lambda rec, i, j: b"".join(rec[i:j])
    try:
        # chunks of different sizes: pool 1 runs ahead by several reads; only the pairs complete in both are there
        assert a.append(text(rec1, 0, 9), False) == (9, True) and b.append(text(rec2, 0, 4), False) == (4, True)
        _assert_pairs(capi.pair_fetch(a, b), host.slice(0, 4))
        before = (a.sizes(), b.sizes())
        with pytest.raises(RuntimeError, match="pooled"):     # more than the shorter pool holds: KASA_E_ARG, nothing moves
            capi.pair_take(a, b, dev, 5)
        with pytest.raises(RuntimeError, match="outside"):
            capi.pair_fetch(a, b, 2, 3)
        assert (a.sizes(), b.sizes()) == before
        assert b.append(text(rec2, 4, 15), False) == (11, True)          # now pool 2 is ahead
        _assert_pairs(capi.pair_fetch(a, b), host.slice(0, 9))
        # a few pairs out, the rest fetched (rebased), more appended to both, out again
        capi.pair_take(a, b, dev, 3)
        assert a.sizes()[0] == 6 and b.sizes()[0] == 12
        _scores_equal(dev, ref, host.slice(0, 3))
        _assert_pairs(capi.pair_fetch(a, b), host.slice(3, 9))
        _assert_pairs(capi.pair_fetch(a, b, 2, 3), host.slice(5, 8))
        assert a.append(text(rec1, 9, 30), False) == (21, True) and b.append(text(rec2, 15, 30), False) == (15, True)
        _assert_pairs(capi.pair_fetch(a, b), host.slice(3, 30))
        # an empty take is an empty batch and moves nothing
        capi.pair_take(a, b, dev, 0)
        assert dev.n_reads == 0 and a.sizes()[0] == b.sizes()[0] == 27
        # most of both pools out: the next append moves the remainders to the pools' other arrays
        capi.pair_take(a, b, dev, 24)
        _scores_equal(dev, ref, host.slice(3, 27))
        assert a.sizes()[0] == b.sizes()[0] == 3
        assert a.append(text(rec1, 30, 41), False) == (11, True) and b.append(text(rec2, 30, 38), False) == (8, True)
        _assert_pairs(capi.pair_fetch(a, b), host.slice(27, 38))
        _assert_pairs(capi.pair_fetch(a, b, 4, 5), host.slice(31, 36))
        capi.pair_take(a, b, dev, 11)
        _scores_equal(dev, ref, host.slice(27, 38))
        assert a.sizes()[0] == 3 and b.sizes() == (0, 0, 0)
        assert b.append(text(rec2, 38, 41), False) == (3, True)
        capi.pair_take(a, b, dev, 3)
        _scores_equal(dev, ref, host.slice(38, 41))
        assert a.sizes() == (0, 0, 0) and b.sizes() == (0, 0, 0)
    finally:
        a.close(); b.close(); dev.close(); ref.close(); dix.close()


def test_one_pool_twice_and_a_missing_pool_are_refused(world):
    ix, rec1, rec2 = world
    dix = capi.DeviceIndex(ix)
    dev = capi.Context(dix)
    a, b = capi.Parser(0), capi.Parser(0)
    try:
        assert a.append(rec1[0], False) == (1, True) and b.append(rec2[0], False) == (1, True)
        for first, second in ((a, a), (None, b), (a, None)):
            with pytest.raises(RuntimeError, match="one pool|NULL"):
                capi.pair_take(first, second, dev, 1)
            with pytest.raises(RuntimeError, match="one pool|NULL"):
                capi.pair_fetch(first, second, 0, 1)
        rc = capi.lib().kasa_pair_take(a.h, b.h, None, 1)
        assert rc == 1                                        # KASA_E_ARG
        assert a.sizes()[0] == 1 and b.sizes()[0] == 1
    finally:
        a.close(); b.close(); dev.close(); dix.close()


# ---- scores ----
@pytest.fixture(scope="module")
def golden_pairs():
    assert capi.device_count() > 0
    d, ix = helpers.load_case("pairs")
    f1, f2 = os.path.join(d, "pair_1.fastq"), os.path.join(d, "pair_2.fastq")
    return ix, open(f1, "rb").read(), open(f2, "rb").read(), reads.parse_pairs(f1, f2)


@pytest.mark.parametrize("frames", [3, 6])
@pytest.mark.parametrize("takes", [1, 2], ids=["one-take", "two-takes"])
def test_golden_pairs_score_like_upload_segments(golden_pairs, frames, takes):
    """CSR scores and the profile tables of the pairs taken out of the pools, bit-equal to the host-parsed ones'"""
    ix, t1, t2, host = golden_pairs
    dix = capi.DeviceIndex(ix)
    dev, ref = capi.Context(dix, 12, 7, frames), capi.Context(dix, 12, 7, frames)
    a, b = capi.Parser(0), capi.Parser(0)
    try:
        assert a.append(t1, False)[1] and b.append(t2, False)[1]
        cuts = [0, host.n] if takes == 1 else [0, host.n // 3, host.n]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            capi.pair_take(a, b, dev, hi - lo)
            _scores_equal(dev, ref, host.slice(lo, hi))
        assert a.sizes() == (0, 0, 0) and b.sizes() == (0, 0, 0)
    finally:
        a.close(); b.close(); dev.close(); ref.close(); dix.close()
