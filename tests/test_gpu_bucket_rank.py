"""bucket_rank64_kernel, the second half of the query sort for 64-bit keys: the pairs arrive ordered by the top 32 key bits
(four radix passes), and every member of a bucket -- a run of equal top bits -- finds its place by counting the members whose
low 28 bits order before its own, ties by input position.

The kernel works on tiles of TILE positions OF THE PASSES' OUTPUT with a halo of HALO on either side, reads the low bits four
members at a time from 16-byte groups, finds a bucket's ends in one 64-bit word of flags per row of 64 positions (and in two
tables when the row's own word has no flag on that side), and hands over to a scan of global memory when a bucket leaves the
staged window.  Buckets of more than LIMIT members are copied through and sorted one by one afterwards.

So the batches here are built from the passes' output backwards: a list of buckets with ascending top bits, each with its
member count and its low bits in input order, fixes where every bucket starts after the passes; the batch itself is a random
interleaving of the buckets that keeps each bucket's members in order (the passes are stable).  Payloads are a permutation
of 0 .. n - 1, so a member in the wrong place among equal keys shows.  Every expectation is oracle.sort_queries on the same
batch, compared with np.array_equal for the kernel (flags 0), the kernel for any key width (4194304) and the library sort
over all key bits (64)."""
import numpy as np
import pytest

from kasa_amd import capi
from oracle import oracle
from tests.test_gpu_parity import _gpu_or_fail, synthetic_world

pytestmark = pytest.mark.gpu

TILE, HALO, LIMIT = 2048, 128, 1024      # RANK_TILE, RANK_HALO, SORT_BUCKET_LIMIT (kasa_hip.hip)
LOW = 28                                 # key bits below a bucket's: 60 - SORT_TOP
FULL = (1 << LOW) - 1
GENERIC, LIBRARY = 4194304, 64


@pytest.fixture(scope="module")
def ctx():
    _gpu_or_fail()
    ix, _ = synthetic_world(71, 4, 3000, 10)
    dix = capi.DeviceIndex(ix)
    c = capi.Context(dix, 12, 7, 3)
    yield c
    c.close(); dix.close()


def mixed_lows(rng, m):
    """Random low bits; half of them drawn from four values, so that ties are common."""
    low = rng.integers(0, 1 << LOW, size=m, dtype=np.uint64)
    few = rng.integers(0, 1 << LOW, size=4, dtype=np.uint64)
    tie = rng.random(m) < 0.5
    low[tie] = few[rng.integers(0, 4, size=m)][tie]
    return low


def filler(rng, total):
    """Bucket sizes 1 .. 5 that add up to `total`."""
    sizes = []
    while total > 0:
        m = min(int(rng.integers(1, 6)), total)
        sizes.append(m)
        total -= m
    return sizes


def make_batch(buckets, seed):
    """buckets: (members, lows or None, neighbour) in the order of the passes' output.  Top bits ascend by an even step from
    an even start; a `neighbour` bucket's top bits are its predecessor's + 1, so the two keys differ in bit 28 only.
    Returns (keys, payloads) and the start of every bucket after the passes."""
    rng = np.random.default_rng(seed)
    keys, label, starts = [], [], []
    top, at = 2, 0
    for b, (m, lows, neighbour) in enumerate(buckets):
        top = top + 1 if neighbour else (top | 1) + 3 + 2 * int(rng.integers(0, 500))
        assert top < 1 << 32
        low = mixed_lows(rng, m) if lows is None else np.asarray(lows, dtype=np.uint64)
        assert low.shape[0] == m and int(low.max(initial=0)) <= FULL
        keys.append((np.uint64(top) << np.uint64(LOW)) | low)
        label.append(np.full(m, b, dtype=np.int64))
        starts.append(at)
        at += m
    keys, label = np.concatenate(keys), np.concatenate(label)
    rng.shuffle(label)                                   # which bucket sits at each place of the batch ...
    q = np.empty_like(keys)
    q[np.argsort(label, kind="stable")] = keys           # ... its members in their order
    payload = rng.permutation(keys.shape[0]).astype(np.uint32)
    return q, payload, starts


def plain(sizes):
    return [(m, None, False) for m in sizes]


def check(ctx, q, payload):
    n = q.shape[0]
    qs, ps = oracle.sort_queries(q, payload)
    for flags in (0, GENERIC, LIBRARY):
        ctx.debug_flags(flags)
        ctx.set_queries(q, payload, n)
        ctx.sort_and_range()
        km, rd = ctx.queries()
        assert np.array_equal(km, qs), f"flags {flags}: keys differ, first at {int(np.flatnonzero(km != qs)[0])} of {n}"
        assert np.array_equal(rd, ps), f"flags {flags}: payloads differ, first at {int(np.flatnonzero(rd != ps)[0])} of {n}"
    ctx.debug_flags(0)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, TILE + HALO - 1, TILE + HALO, TILE + HALO + 1,
                               3 * TILE + 5])
def test_batch_sizes(ctx, n):
    """Batches that end anywhere in a row of 64, in a wavefront's rows, in a tile and around the end of the first tile's halo;
    buckets of 1 to 5 members."""
    rng = np.random.default_rng(100 + n)
    q, payload, _ = make_batch(plain(filler(rng, n)), 200 + n)
    check(ctx, q, payload)


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 7, 8, 9])
def test_short_buckets_at_every_alignment(ctx, m):
    """A bucket of m members starting at every residue mod 4 (the 16-byte groups of four members: ragged first and last
    group, both in one group, whole groups between), twenty times each, short buckets between them."""
    rng = np.random.default_rng(300 + m)
    buckets, at, want = [], 0, []
    for rep in range(20):
        for r in range(4):
            for s in filler(rng, int(rng.integers(0, 9))):
                buckets.append((s, None, False)); at += s
            while at % 4 != r:
                buckets.append((1, None, False)); at += 1
            want.append((len(buckets), r))
            buckets.append((m, None, False)); at += m
    q, payload, starts = make_batch(buckets, 400 + m)
    assert all(starts[b] % 4 == r for b, r in want)
    check(ctx, q, payload)


@pytest.mark.parametrize("m", [63, 64, 65, 127, 128, 129, 200])
def test_buckets_longer_than_a_row(ctx, m):
    """Buckets that cover one or more rows of 64 positions without a flag in them (the row's entry in the two tables), starting
    at every residue mod 4 and at the first, a middle and the last position of a row."""
    rng = np.random.default_rng(500 + m)
    buckets, at, want = [], 0, []
    for r in (0, 1, 2, 3, 31, 62, 63, 64, 65):
        for s in filler(rng, int(rng.integers(1, 40))):
            buckets.append((s, None, False)); at += s
        while at % 64 != r % 64:
            buckets.append((1, None, False)); at += 1
        want.append((len(buckets), r % 64))
        buckets.append((m, None, False)); at += m
    buckets += plain(filler(rng, 77))
    q, payload, starts = make_batch(buckets, 600 + m)
    assert all(starts[b] % 64 == r for b, r in want)
    check(ctx, q, payload)


@pytest.mark.parametrize("m", [LIMIT - 1, LIMIT, LIMIT + 1])
@pytest.mark.parametrize("start", [37, TILE - 300, TILE + 100])
def test_buckets_at_the_limit(ctx, m, start):
    """LIMIT members are ranked by counting, LIMIT + 1 are copied through and sorted on their own: inside the first tile, over
    a tile boundary (members on either side see the bucket leave their window), and inside the second tile's window."""
    rng = np.random.default_rng(700 + m + start)
    q, payload, starts = make_batch(plain(filler(rng, start)) + [(m, None, False)] + plain(filler(rng, 450)), 800 + m + start)
    assert start in starts
    check(ctx, q, payload)


def _ends(m):
    e = {1, 2, m - 1, m}
    if m > HALO + 1:
        e |= {m - (HALO - 1), m - HALO, m - (HALO + 1), HALO - 1, HALO, HALO + 1}
    return sorted(x for x in e if 1 <= x <= m)


@pytest.mark.parametrize("m,e", [(m, e) for m in (2, 5, 130, 300) for e in _ends(m)])
def test_buckets_over_a_tile_boundary(ctx, m, e):
    """A bucket of m members that ends e positions after a tile boundary, at both inner boundaries of a batch of three tiles
    and five.  m - e, the bucket's reach before the boundary, is below, exactly and above HALO (the members behind the
    boundary find its start in their halo, at its first position, or not at all: the scan of global memory); e likewise for
    the members before the boundary and the bucket's end."""
    rng = np.random.default_rng(900 + 7 * m + e)
    n = 3 * TILE + 5
    first, second = TILE + e - m, 2 * TILE + e - m
    buckets = plain(filler(rng, first)) + [(m, None, False)] + plain(filler(rng, second - first - m)) + [(m, None, False)]
    buckets += plain(filler(rng, n - second - m))
    q, payload, starts = make_batch(buckets, 1000 + 7 * m + e)
    assert first in starts and second in starts and q.shape[0] == n
    check(ctx, q, payload)


@pytest.mark.parametrize("m", [2, 5, 130, 300])
def test_buckets_at_the_ends_of_the_batch(ctx, m):
    """A bucket at position 0, and a bucket that ends exactly at n: with the batch ending 1, HALO and HALO + 1 positions into
    its last tile (the window's end is the batch's end, inside and outside the tile before's halo) and at a tile's end."""
    rng = np.random.default_rng(1100 + m)
    for tail in (1, HALO, HALO + 1, TILE):
        n = 2 * TILE + tail
        q, payload, starts = make_batch([(m, None, False)] + plain(filler(rng, n - 2 * m)) + [(m, None, False)], 1200 + m + tail)
        assert starts[-1] == n - m
        check(ctx, q, payload)


@pytest.mark.parametrize("tail", [1, 5, HALO, 300])
@pytest.mark.parametrize("m", [500, LIMIT])
def test_bucket_from_before_the_last_tiles_halo_to_the_end(ctx, tail, m):
    """The last bucket begins more than HALO before the last tile and runs to n: its members in the last tile see no flag on
    the left, those in the tile before see none on the right although the window is cut by the batch's end or not at all."""
    rng = np.random.default_rng(1300 + tail + m)
    n = 3 * TILE + tail
    q, payload, starts = make_batch(plain(filler(rng, n - m)) + [(m, None, False)], 1400 + tail + m)
    assert starts[-1] == n - m and n - m < 3 * TILE - HALO
    check(ctx, q, payload)


def _patterns(m):
    d = np.arange(m, dtype=np.uint64)
    return {
        "equal": np.full(m, 0x5A5A5A5, dtype=np.uint64),                          # the rank is the input order
        "bit0": np.uint64(0x1234560) | (d * np.uint64(7) // np.uint64(3) & np.uint64(1)),
        "bit27": (((d * np.uint64(5) // np.uint64(3)) & np.uint64(1)) << np.uint64(27)) | np.uint64(0x234567),
        "extremes": np.where((d * np.uint64(3) // np.uint64(2)) % np.uint64(2) == 0, np.uint64(0), np.uint64(FULL)),
        "descending": np.uint64(FULL) - d * np.uint64(3),                         # every member moves
        "descending_pairs": np.uint64(1000) - (d // np.uint64(2)),                # ... and ties keep their order
    }


@pytest.mark.parametrize("pattern", ["equal", "bit0", "bit27", "extremes", "descending", "descending_pairs"])
def test_value_patterns(ctx, pattern):
    """Low bits that differ in bit 0 only, in bit 27 only, are all equal, are 0 and 2^28 - 1, or descend: buckets of 2 to 150
    members at every residue mod 4, one over the first tile boundary."""
    rng = np.random.default_rng(1500)
    buckets, at = [], 0
    for r, m in enumerate([2, 3, 4, 5, 6, 9, 16, 37, 64, 150, 11, 21]):
        for s in filler(rng, int(rng.integers(1, 30))):
            buckets.append((s, None, False)); at += s
        while at % 4 != r % 4:
            buckets.append((1, None, False)); at += 1
        buckets.append((m, _patterns(m)[pattern], False)); at += m
    buckets += plain(filler(rng, TILE - 20 - at)) + [(40, _patterns(40)[pattern], False)] + plain(filler(rng, 100))
    q, payload, starts = make_batch(buckets, 1600)
    assert TILE - 20 in starts
    check(ctx, q, payload)


@pytest.mark.parametrize("m", [1, 3, 8, 70])
def test_neighbouring_buckets_differ_in_the_lowest_top_bit(ctx, m):
    """Two buckets whose keys differ in bit 28 only, with the same low bits in both: they must not merge.  At every residue
    mod 4 of the border between them."""
    rng = np.random.default_rng(1700 + m)
    buckets = []
    for r in range(4):
        low = mixed_lows(rng, m)
        buckets += plain(filler(rng, 13 + r)) + [(m, low, False), (m, low[::-1].copy(), True)]
    buckets += plain(filler(rng, 50))
    q, payload, _ = make_batch(buckets, 1800 + m)
    tops = np.unique(q >> np.uint64(LOW))
    assert np.count_nonzero(np.diff(tops) == 1) == 4
    check(ctx, q, payload)


def test_all_singletons(ctx):
    """Every position carries a flag: nothing to count, every pair stays where it is."""
    q, payload, _ = make_batch(plain([1] * (2 * TILE + 77)), 1900)
    check(ctx, q, payload)


@pytest.mark.parametrize("n", [1000, 5000])
def test_one_bucket_is_the_batch(ctx, n):
    """One flag, at position 0.  1000 members are ranked (the tables' 'none' on the right is the batch's end); 5000 are listed
    as one long bucket by its first member and sorted on their own."""
    q, payload, _ = make_batch([(n, None, False)], 2000 + n)
    check(ctx, q, payload)
