"""The row merge by classes: the first class's launch sweeps all reads, the upper classes and the long one walk the rows
score_main_kernel listed for them, and every walk fetches the next row it takes while it merges the current one.

Batches come in through set_queries with kHigh == kLow, over an index that has taxa 1 and 2 on every k-mer and further taxa
on three kinds of k-mers, so that a query leaves one staging record per taxon beyond the two register taxa:

    kind A: 16 further taxa, kind B: 1, kind C: 4, kind N: not in the index

and a read of a + b + c + n distinct k-mers gets a row of 2 + 16 a + b + 4 c records (0 without a match).  The tests do not
rely on that sum: they read the lengths back (kasa_batch_staged_lengths) and derive every expectation from those.  Output is
compared with the oracle as test_adversarial_queries_vs_oracle does (profile tables, per-read CSR bit for bit)."""
import numpy as np
import pytest

from kasa_amd import capi, formats
from oracle import oracle
from tests import helpers
from tests.test_gpu_parity import _gpu_or_fail, assert_csr_equal, csr_rows

pytestmark = pytest.mark.gpu

RMAX = 1024                      # longest row of the third class (kasa_hip.hip)
NO_DENSE = 33554432              # test tap: handed-over reads go to the general kernel, where last_slow_reads() counts them
POOL = {"A": 1400, "B": 400, "C": 400, "N": 64}


class World:
    """Index + k-mer pools.  n_taxa counts the content's rows (taxon 0 = non_unique); only taxa 1 .. 23 have k-mers."""

    def __init__(self, n_taxa, seed=1):
        rng = np.random.default_rng(seed)
        letters = np.arange(1, 21, dtype=np.uint64)
        n_all = sum(POOL.values())
        v = np.zeros(4 * n_all, dtype=np.uint64)
        for _ in range(12):
            v = (v << np.uint64(5)) | letters[rng.integers(0, 20, size=v.shape[0])]
        v = rng.permutation(np.unique(v))[:n_all]
        assert v.shape[0] == n_all
        self.pool, at = {}, 0
        for kind, n in POOL.items():
            self.pool[kind] = v[at:at + n]
            at += n
        content = formats.Content(["non_unique"] + [f"T{i}" for i in range(1, n_taxa)], np.arange(n_taxa, dtype=np.uint32) * np.uint32(7))
        further = {"A": range(3, 19), "B": range(19, 20), "C": range(20, 24)}
        km, tx = [], []
        for kind, taxa in further.items():
            for t in [1, 2] + list(taxa):
                km.append(self.pool[kind])
                tx.append(np.full(self.pool[kind].shape[0], content.taxids[t], dtype=np.uint32))
        self.ix = formats.make_index(np.concatenate(km), np.concatenate(tx), content)
        self.n_taxa = n_taxa

    def batch(self, reads, seed):
        """reads: one (a, b, c, n) per read -> (k-mers, read ids); the k-mers of a read are distinct."""
        rng = np.random.default_rng(seed)
        q, rd = [], []
        for r, counts in enumerate(reads):
            for kind, n in zip("ABCN", counts):
                if n:
                    q.append(rng.choice(self.pool[kind], size=n, replace=False))
                    rd.append(np.full(n, r, dtype=np.uint32))
        return np.concatenate(q), np.concatenate(rd)


def row_of(length):
    """A read whose row has `length` records by the sum above (length >= 2)."""
    return ((length - 2) // 16, (length - 2) % 16, 0, 0)


_worlds = {}


def world(n_taxa):
    if n_taxa not in _worlds:
        _worlds[n_taxa] = World(n_taxa)
    return _worlds[n_taxa]


def expected(w, q, rd, n_reads):
    p = oracle.params(12, 12, 3)
    iv = oracle.IndexView(w.ix)
    qs, rs_ = oracle.sort_queries(q, rd)
    a, b = oracle.ranges(iv, p, qs)
    return oracle.compare(iv, p, qs, rs_, a, b, n_reads, True, closed_form=False)


def run(ctx, q, rd, n_reads):
    ctx.profile_reset()
    ctx.set_queries(q, rd, n_reads)
    ctx.sort_and_range()
    ctx.lookup_score(True, coverage=False)
    ca, cu, _ = ctx.profile()
    return ca, cu, ctx.scores()


def assert_equals_oracle(out, res):
    ca, cu, scores = out
    assert np.array_equal(cu, res.count_unique)
    np.testing.assert_allclose(ca, res.count_all, rtol=1e-12, atol=0)
    assert_csr_equal(csr_rows(*scores), helpers.csr_from_dense(res.M))


def classes_of(lengths, handed, n_taxa):
    """What kasa_ctx_row_classes must say for rows of these lengths, `handed` of which are reads the fast kernels gave away
    (their length is a count of taxa, far below 256)."""
    second_hi = 512 if n_taxa <= 2048 else 256
    second = int(np.count_nonzero((lengths > 256) & (lengths <= second_hi)))
    third = int(np.count_nonzero((lengths > second_hi) & (lengths <= RMAX)))
    long_ = int(np.count_nonzero(lengths > RMAX))
    return (lengths.shape[0] - handed - second - third - long_, second, third, long_)


@pytest.mark.parametrize("n_taxa", [30, 2100], ids=["three_classes", "two_classes_wide_bitmap"])
def test_lengths_on_both_sides_of_every_bound(n_taxa):
    """Rows of b - 3 .. b + 3 records for b = 256, 512, RMAX (so b - 1, b, b + 1 are there even if the sum in the module's
    docstring were off by two), rows of the long class (reads of 300 queries), a long read with a short row, rows without
    records.  A row beyond RMAX of a read below 256 queries is no merge row: the general kernel takes the read."""
    _gpu_or_fail()
    w = world(n_taxa)
    reads, over = [], []
    for b in (256, 512, RMAX):
        for d in range(-3, 4):
            if b + d > RMAX:
                over.append(len(reads))
            reads.append(row_of(b + d))
    reads += [(0, 0, 300, 0)] * 3                 # 1202 records, 300 queries: the long class
    reads += [(0, 300, 0, 0)]                      # 302 records of a long read
    reads += [(0, 0, 0, 5), (0, 0, 0, 0), (3, 0, 0, 2), (0, 1, 0, 0)]   # no match, no query at all, short rows
    q, rd = w.batch(reads, 10)
    n_reads = len(reads)
    res = expected(w, q, rd, n_reads)
    dix = capi.DeviceIndex(w.ix)
    ctx = capi.Context(dix, 12, 12, 3)
    ctx.debug_flags(NO_DENSE)
    ctx.keep_staged_lengths(True)
    out = run(ctx, q, rd, n_reads)
    lengths = ctx.staged_lengths()
    print("staged lengths:", lengths.tolist())
    print("row classes:", ctx.row_classes(), "general reads:", ctx.last_slow_reads())
    for b in (256, 512, RMAX):
        for v in (b - 1, b) + ((b + 1,) if b < RMAX else ()):
            assert v in lengths, f"no row of {v} records"
    assert ctx.last_slow_reads() == len(over)      # RMAX + 1 .. RMAX + 3: the general kernel's
    assert all(lengths[r] <= n_taxa for r in over)  # (what it left there is the read's taxa, not 1025 records)
    assert np.count_nonzero(lengths > RMAX) == 3    # the long class only
    assert np.count_nonzero(lengths == 0) == 2
    assert ctx.row_classes() == classes_of(lengths, len(over), n_taxa)
    got = ctx.row_classes()
    assert got[3] == 3 and got[2] >= 3 and (got[1] >= 3 if n_taxa <= 2048 else got[1] == 0)
    assert_equals_oracle(out, res)
    ctx.close(); dix.close()


@pytest.mark.parametrize("short", [True, False], ids=["all_rows_short", "no_row_short"])
def test_empty_classes(short):
    """Upper classes without rows are not launched; a first class without rows sweeps and finds nothing."""
    _gpu_or_fail()
    w = world(30)
    rng = np.random.default_rng(11)
    if short:
        reads = [row_of(int(v)) for v in rng.integers(2, 200, size=200)]
    else:
        reads = [row_of(int(v)) for v in rng.integers(257, RMAX + 1, size=60)]
    q, rd = w.batch(reads, 11)
    res = expected(w, q, rd, len(reads))
    dix = capi.DeviceIndex(w.ix)
    ctx = capi.Context(dix, 12, 12, 3)
    ctx.keep_staged_lengths(True)
    out = run(ctx, q, rd, len(reads))
    lengths = ctx.staged_lengths()
    got = ctx.row_classes()
    print("row classes:", got)
    assert got == classes_of(lengths, 0, 30)
    if short:
        assert got == (len(reads), 0, 0, 0)
    else:
        assert got[0] == 0 and got[1] > 0 and got[2] > 0 and got[3] == 0
    assert_equals_oracle(out, res)
    ctx.close(); dix.close()


def test_many_rows_per_wavefront():
    """Three workgroups per launch over about 300 reads whose classes alternate read by read -- first, second, third,
    no match at all, a read for the general kernel, first -- and two rows of the long class (a list shorter than the grid)."""
    _gpu_or_fail()
    w = world(30)
    rng = np.random.default_rng(12)
    reads = []
    for _ in range(50):
        reads += [row_of(int(rng.integers(2, 257))), row_of(int(rng.integers(257, 513))), row_of(int(rng.integers(513, RMAX + 1))),
                  (0, 0, 0, int(rng.integers(0, 6))), row_of(int(rng.integers(RMAX + 1, RMAX + 200))), row_of(int(rng.integers(2, 257)))]
    reads.insert(100, (0, 0, 300, 0))
    reads.append((0, 0, 290, 3))
    q, rd = w.batch(reads, 12)
    n_reads = len(reads)
    res = expected(w, q, rd, n_reads)
    dix = capi.DeviceIndex(w.ix)
    ctx = capi.Context(dix, 12, 12, 3)
    ctx.keep_staged_lengths(True)
    ctx.row_merge_blocks(3)
    capped = run(ctx, q, rd, n_reads)
    lengths = ctx.staged_lengths()
    got = ctx.row_classes()
    print("row classes:", got)
    assert got == classes_of(lengths, 50, 30)
    assert got[1] == 50 and got[2] == 50 and got[3] == 2 and np.count_nonzero(lengths == 0) >= 50
    assert_equals_oracle(capped, res)
    ctx.row_merge_blocks(0)
    plain = run(ctx, q, rd, n_reads)
    assert ctx.row_classes() == got
    assert np.array_equal(capped[0].view(np.uint64), plain[0].view(np.uint64)) and np.array_equal(capped[1], plain[1])
    (off_c, tax_c, sc_c), (off_p, tax_p, sc_p) = capped[2], plain[2]
    assert np.array_equal(off_c, off_p) and np.array_equal(tax_c, tax_p) and np.array_equal(sc_c.view(np.uint32), sc_p.view(np.uint32))
    ctx.close(); dix.close()


def test_class_counts_after_a_staging_retry():
    """A fresh context starts with room for max(65536, 8 per read) staging records; 150 rows of 600 to 1000 records need
    more, so the first attempt's fast kernels are rerun with a larger buffer.  The counts are those of the rerun alone."""
    _gpu_or_fail()
    w = world(30)
    rng = np.random.default_rng(13)
    reads = [row_of(int(v)) for v in rng.integers(600, 1001, size=150)] + [row_of(int(v)) for v in rng.integers(2, 500, size=50)]
    q, rd = w.batch(reads, 13)
    res = expected(w, q, rd, len(reads))
    dix = capi.DeviceIndex(w.ix)
    ctx = capi.Context(dix, 12, 12, 3)
    ctx.keep_staged_lengths(True)
    out = run(ctx, q, rd, len(reads))
    lengths = ctx.staged_lengths()
    assert int(lengths.sum()) > 65536               # (the first attempt could not have held them)
    got = ctx.row_classes()
    print("row classes:", got)
    assert sum(got) == len(reads)
    assert got == classes_of(lengths, 0, 30)
    assert_equals_oracle(out, res)
    ctx.close(); dix.close()
