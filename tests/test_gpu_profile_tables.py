"""The profile-table kernels: profile_group_table_kernel (group keys of narrow records, up to eight levels) and
profile_table_kernel (per-read keys of wide records, windows of at most eight levels) count keys in LDS cells whose layout --
per level the largest |T| with a cell (nn) and the level's first row -- comes to the kernels packed into two 64-bit arguments.

Batches come in through set_queries.  An index is made of FAMILIES: a base k-mer x and, for a depth j, a k-mer that shares
exactly K - j leading letters with x and carries g[j] taxa of its own (depth 0 is x itself).  Families differ in their first
k_low letters, so the query x meets, at level lv (k = k_high - lv), the taxa of the depths 0 .. lv and nothing else:

    |T| at level lv = g[0] + ... + g[lv]

and a taxon of depth j has one group key per run of levels j .. nK - 1 over which that sum stays the same.  Every expectation
comes from the oracle (oracle.compare on the same index and queries): count_unique exactly, count_all to 1e-12, the per-read CSR
bit for bit.  `layout` below restates prof_table_layout (kasa_hip.hip) so that the tests can say which |T| is the last with a
cell; the values it gives are spelled out where they are used.

Not reached at test sizes, and so not tested: the leftover list filling up (it holds at least 2^20 keys) and hits > maxHits
(maxHits stays 65535 until a workgroup sees 65 k keys per counter)."""
import numpy as np
import pytest

from kasa_amd import capi, formats
from oracle import oracle
from tests import helpers
from tests.test_gpu_parity import _gpu_or_fail, assert_csr_equal, csr_rows

pytestmark = pytest.mark.gpu

CELLS = 67108864                 # test tap: group keys always through the per-|T| cells (profile_group_table_kernel)
BUDGET = (160 * 1024 - 2048 * 8 - 1024) // 4       # 32-bit cells of a workgroup's table (profile_from_keys)
ROUND = 256 * 1024 * 8           # keys of one round of all workgroups on 256 CUs


def layout(n_k, lo, hi, n_taxa, budget):
    """prof_table_layout: nn per level for the window [lo, hi); all zero when not even |T| = 1 fits everywhere."""
    nn = [0] * n_k
    per_taxon = budget // n_taxa
    if hi - lo <= 0 or per_taxon < hi - lo:
        return nn
    left = per_taxon - (hi - lo)
    for lv in range(lo, hi):
        nn[lv] = 1

    def grow(lv, up_to):
        nonlocal left
        while lo <= lv < hi and nn[lv] < up_to and left > 0:
            nn[lv] += 1
            left -= 1
    for lv in range(lo, hi):
        grow(lv, 2)
    if hi == n_k:
        grow(n_k - 2, 4)
        grow(n_k - 1, 24)
        grow(n_k - 2, 8)
    for up_to in range(3, 9):
        for lv in range(hi - 1, lo - 1, -1):
            grow(lv, up_to)
    return nn


def group_layout(n_k, n_taxa):
    """(range cells?, nn) of the one pass over group keys."""
    rc = n_k * n_taxa <= BUDGET // 3
    return rc, layout(n_k, 0, n_k, n_taxa, BUDGET - n_k * n_taxa if rc else BUDGET)


def windows(n_k):
    """The level windows of per-read keys (wide records: n_k > 8)."""
    w = [(n_k - 4, n_k)]
    hi = n_k - 4
    while hi > 0:
        w.append((max(0, hi - 8), hi))
        hi -= 8
    return w


def pack(letters):
    """[n, K] letters -> k-mers (first letter most significant): u64 for K = 12, KEY128 for K = 25."""
    n, K = letters.shape
    if K == 12:
        out = np.zeros(n, dtype=np.uint64)
        for p in range(K):
            out |= letters[:, p].astype(np.uint64) << np.uint64(5 * (K - 1 - p))
        return out
    out = np.zeros(n, dtype=formats.KEY128_DTYPE)
    for i in range(n):
        v = 0
        for p in range(K):
            v = (v << 5) | int(letters[i, p])
        out[i] = (v & 0xFFFFFFFFFFFFFFFF, v >> 64)
    return out


class Families:
    """specs: one g vector (new taxa per depth) per family.  n_taxa counts the content's rows; only the first few dozen taxa
    carry k-mers unless the families are dealt out over `blocks` blocks of taxa.  queries(): every family's x; variants(): the deeper k-mers of the families as queries of their own."""

    def __init__(self, K, k_low, n_taxa, specs, seed, blocks=1):
        rng = np.random.default_rng(seed)
        n = len(specs)
        depth = max(len(g) for g in specs)
        heads = np.unique(rng.integers(0, 20 ** k_low, size=2 * n + 64))
        heads = rng.permutation(heads)[:n]
        assert heads.shape[0] == n
        L = rng.integers(1, 21, size=(n, K)).astype(np.uint8)
        for p in range(k_low):                                  # distinct first k_low letters: families never meet
            L[:, p] = (heads // 20 ** (k_low - 1 - p)) % 20 + 1
        self.x = pack(L)
        content = formats.Content(["non_unique"] + [f"T{i}" for i in range(1, n_taxa)], np.arange(n_taxa, dtype=np.uint32) * np.uint32(7))
        g = np.zeros((n, depth), dtype=np.int64)
        for f, s in enumerate(specs):
            g[f, :len(s)] = s
        assert g.sum(axis=1).max() < min(n_taxa, 64)
        width = int(g.sum(axis=1).max())                        # family f takes its taxa from block f % blocks of `width` taxa
        assert blocks * width < n_taxa
        first = 1 + (np.arange(n) % blocks)[:, None] * width + np.cumsum(g, axis=1) - g   # first taxon of a depth
        km, tx, self.var = [], [], []
        for j in range(depth):
            rows = np.flatnonzero(g[:, j] > 0)
            if rows.shape[0] == 0:
                continue
            Lj = L[rows].copy()
            if j:
                Lj[:, K - j] = Lj[:, K - j] % 20 + 1             # another letter there: K - j letters shared with x
            kj = pack(Lj)
            if j:
                self.var.append(kj)
            for t in range(int(g[:, j].max())):
                has = g[rows, j] > t
                km.append(kj[has])
                tx.append(content.taxids[first[rows[has], j] + t])
        self.ix = formats.make_index(np.concatenate(km), np.concatenate(tx).astype(np.uint32), content)
        self.K, self.n_taxa = K, n_taxa

    def queries(self):
        return self.x

    def variants(self):
        return np.concatenate(self.var) if self.var else self.x[:0]


def spread(q, n_reads, seed):
    """Read ids for the queries: every read gets some."""
    rng = np.random.default_rng(seed)
    rd = rng.integers(0, n_reads, size=q.shape[0]).astype(np.uint32)
    rd[:min(n_reads, q.shape[0])] = np.arange(min(n_reads, q.shape[0]), dtype=np.uint32)
    return rd


def expected(ix, k_high, k_low, q, rd, n_reads):
    p = oracle.params(k_high, k_low, 3, K=25 if formats.is_wide(ix.kmer) else 12)
    iv = oracle.IndexView(ix)
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


def check(fam, k_high, k_low, q, n_reads, seed, flags=CELLS, again=False):
    rd = spread(q, n_reads, seed)
    res = expected(fam.ix, k_high, k_low, q, rd, n_reads)
    dix = capi.DeviceIndex(fam.ix)
    ctx = capi.Context(dix, k_high, k_low, 3)
    ctx.debug_flags(flags)
    assert_equals_oracle(run(ctx, q, rd, n_reads), res)
    keys = ctx.batch_stats()["profile_keys"]
    print("profile keys:", keys)
    if again:                                                   # the same context once more: reused buffers
        assert_equals_oracle(run(ctx, q, rd, n_reads), res)
        assert ctx.batch_stats()["profile_keys"] == keys
    ctx.close(); dix.close()
    return keys, res


def unit(n_k, s, m=1):
    g = [0] * n_k
    g[s] = m
    return g


def six_level_specs(nn):
    """The level ranges of -k 12 7 for a table with `nn`."""
    specs = []
    specs += [unit(6, s) for s in range(6)]                     # |T| = 1 from level s down to the shallowest: range cells; a start at each level
    specs += [[1, 0, 0, 0, 0, 1], [1, 0, 0, 1, 0, 0], [1, 0, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0],   # |T| = 1 ends one .. four levels above it
              [0, 1, 0, 0, 1, 0], [0, 0, 1, 0, 0, 2]]
    for lv in (5, 4, 1):                                        # the last cell and the first leftover: shallowest, the one above, a deep level
        specs += [unit(6, lv, max(nn[lv], 1)), unit(6, lv, nn[lv] + 1)]
        for m in (max(nn[lv], 2), nn[lv] + 1):                  # ... and reached from |T| = 1 at the levels above
            g = unit(6, lv, m - 1)
            g[0] = 1
            specs.append(g)
    specs += [[1, 1, 1, 1, 1, 1], [2, 0, 2, 0, 2, 0], [3, 3, 3, 3, 3, 3]]   # |T| changes at every level
    return specs


def test_layout_values():
    """The layouts the tests below rely on (no device work: the restated prof_table_layout, by hand)."""
    assert BUDGET == 36608
    assert group_layout(6, 1400) == (True, [2, 2, 2, 2, 4, 8])
    assert group_layout(6, 2033) == (True, [2, 2, 2, 2, 2, 2])          # 6 * 2033 = 12198 <= 12202: the last count with range cells
    assert group_layout(6, 2034) == (False, [2, 2, 2, 2, 4, 5])         # the first without
    assert group_layout(6, 6000) == (False, [1, 1, 1, 1, 1, 1])
    assert group_layout(6, 7000) == (False, [0, 0, 0, 0, 0, 0])         # 36608 // 7000 = 5 < 6 levels: no table
    assert group_layout(8, 1400) == (True, [2, 2, 2, 2, 2, 2, 4, 2])
    assert windows(19) == [(15, 19), (7, 15), (0, 7)] and windows(9) == [(5, 9), (0, 5)]
    assert layout(19, 15, 19, 1400, BUDGET)[15:] == [2, 2, 4, 18]
    assert layout(19, 7, 15, 1400, BUDGET)[7:15] == [3, 3, 3, 3, 3, 3, 4, 4]
    assert layout(19, 0, 7, 1400, BUDGET)[:7] == [3, 3, 4, 4, 4, 4, 4]
    assert layout(9, 5, 9, 1400, BUDGET)[5:] == [2, 2, 4, 18]
    assert layout(9, 0, 5, 1400, BUDGET)[:5] == [5, 5, 5, 5, 6]


@pytest.mark.parametrize("n_taxa", [1400, 2033, 2034, 6000, 7000],
                         ids=["range_cells", "last_with_range_cells", "first_without", "nn_one_everywhere", "no_table"])
def test_six_levels(n_taxa):
    """-k 12 7 over 120 copies of every level range (more than 8192 keys: all eight key slots of a thread are used), x and the
    deeper k-mers as queries.  nn: 1400 taxa [2, 2, 2, 2, 4, 8] with range cells; 2033 [2] * 6 with, 2034 [2, 2, 2, 2, 4, 5]
    without range cells (nK * nTaxa <= budget / 3 on either side); 6000 [1] * 6; 7000 no table: every key leaves as a leftover."""
    _gpu_or_fail()
    rc, nn = group_layout(6, n_taxa)
    assert rc == (n_taxa <= 2033)
    fam = Families(12, 7, n_taxa, six_level_specs(nn) * 120, seed=n_taxa)
    q = np.concatenate((fam.queries(), fam.variants(), fam.queries()[::3]))     # (a third of the x twice: hits of 2)
    keys, res = check(fam, 12, 7, q, 24, seed=1, again=(n_taxa == 1400))
    assert keys > 8192
    assert res.count_unique[5].sum() > 0 and res.count_unique[0].sum() > 0


def test_six_levels_on_the_product_path():
    """The same keys without the test tap: whatever profile_from_keys chooses for a fresh context."""
    _gpu_or_fail()
    fam = Families(12, 7, 1400, six_level_specs(group_layout(6, 1400)[1]) * 10, seed=5)
    check(fam, 12, 7, np.concatenate((fam.queries(), fam.variants())), 8, seed=2, flags=0)


def test_eight_levels():
    """-k 12 5: nn = [2, 2, 2, 2, 2, 2, 4, 2] at 1400 taxa.  Keys spanning all eight levels with |T| = 1 (a range cell), 2 (a cell
    at every level) and 3 (a leftover at every level, the first and the last included); |T| = 3 over the levels 0 .. 5 and 7 around
    the one level that has a cell for it; |T| stepping at every level."""
    _gpu_or_fail()
    assert group_layout(8, 1400) == (True, [2, 2, 2, 2, 2, 2, 4, 2])
    specs = [unit(8, 0, 1), unit(8, 0, 2), unit(8, 0, 3), unit(8, 0, 4), unit(8, 0, 5),
             [1, 0, 0, 0, 0, 0, 0, 1], [2, 0, 0, 0, 0, 0, 0, 1], [1, 1, 1, 1, 1, 1, 1, 1], [3, 0, 0, 0, 0, 0, 1, 0],
             unit(8, 7, 2), unit(8, 7, 3), unit(8, 6, 4), unit(8, 6, 5), unit(8, 3, 1)]
    fam = Families(12, 5, 1400, specs * 250, seed=8)
    keys, _ = check(fam, 12, 5, np.concatenate((fam.queries(), fam.variants())), 16, seed=3)
    assert keys > 8192


_wide = {}


def wide_world():
    """K = 25, 1400 taxa: families that start at a depth s with m taxa, |T| = m from level s on, and families whose |T| steps
    up across a window edge.  s: in each window of -k 25 7 ([0, 7), [7, 15), [15, 19)) and of -k 25 17 ([0, 5), [5, 9)), and on
    both sides of every edge; m: on both sides of nn in each window (3 | 4 at the levels 0 .. 1 and 7 .. 12, 4 | 5 at 2 .. 6 and
    13 .. 14, 2 | 3 at 15 .. 16, 4 | 5 at 17, 18 | 19 at 18; nine levels: 5 | 6 at 0 .. 3, 6 | 7 at 4, 2 | 3 at 5 .. 6, 18 | 19 at 8)."""
    if "w" not in _wide:
        specs = []
        for s in (0, 1, 2, 4, 5, 6, 7, 8, 12, 13, 14, 15, 16, 17, 18):
            for m in (1, 2, 3, 4, 5, 6, 7, 18, 19):
                specs.append(unit(19, s, m))
        for s in (4, 6, 14):                                    # a step in |T| right at a window's edge
            g = [0] * 19
            g[0], g[s], g[s + 1] = 2, 1, 2
            specs.append(g)
        _wide["w"] = Families(25, 7, 1400, specs * 4, seed=25)
    return _wide["w"]


@pytest.mark.parametrize("k_low,n_windows", [(7, 3), (17, 2)], ids=["19_levels_three_windows", "9_levels_two_windows"])
def test_wide_records(k_low, n_windows):
    """More than eight levels: 64-byte records, per-read keys, profile_table_kernel once per level window."""
    _gpu_or_fail()
    n_k = 25 - k_low + 1
    assert len(windows(n_k)) == n_windows
    fam = wide_world()
    check(fam, 25, k_low, np.concatenate((fam.queries(), fam.variants()[::2])), 12, seed=4, flags=0, again=(k_low == 7))


def test_hit_counts():
    """One k-mer in 5000 reads (its leader's keys carry up to 128 hits each: 40 of them per taxon and level range) next to
    k-mers met once, with |T| = 1 (range cells), 2 and 3 (cells at 30 taxa: the table has room for |T| <= 8 everywhere)."""
    _gpu_or_fail()
    assert min(group_layout(6, 30)[1]) >= 8
    specs = [unit(6, 0, 1), unit(6, 0, 1), [1, 0, 0, 1, 0, 1], [1, 0, 0, 1, 0, 1], unit(6, 2, 3), unit(6, 2, 3)]
    fam = Families(12, 7, 30, specs, seed=9)
    x = fam.queries()
    many = np.repeat(x[[0, 2, 4]], 5000)
    rd_many = np.tile(np.arange(5000, dtype=np.uint32), 3)          # read r holds each of the three once
    q = np.concatenate((many, x[[1, 3, 5]]))
    rd = np.concatenate((rd_many, np.array([5000, 5001, 7], dtype=np.uint32)))
    n_reads = 5002
    res = expected(fam.ix, 12, 7, q, rd, n_reads)
    assert res.count_unique[:, 1:].max() >= 5000
    dix = capi.DeviceIndex(fam.ix)
    ctx = capi.Context(dix, 12, 7, 3)
    ctx.debug_flags(CELLS)
    assert_equals_oracle(run(ctx, q, rd, n_reads), res)
    ctx.close(); dix.close()


def test_several_rounds():
    """270 000 families of six nested k-mers, one taxon each at the depths 0 .. 5 (1.62 M records; |T| = lv + 1 at level lv, so
    at 2000 taxa cells up to nn = [2] * 6, range cells, and leftovers beyond), every record a query once and 400 000 of them drawn again with
    replacement.  The group stage folds equal keys of neighbouring queries into one (hits > 1), which leaves about 4.5 keys per
    record (measured: 4 549 484 keys from 1.02 M records): more than three full rounds of 256 workgroups and a partial one, so
    that the keys fetched ahead for the next round and the per-round barriers are exercised.  Twice on one context.

    The families are dealt out over 333 blocks of six taxa.  With all of them on the same six taxa a cell of count_all is the
    oracle's sequential double sum of 2 M terms 1 / |T|, and that sum is itself 1.9e-12 off the exact rational value (measured
    against fractions.Fraction; the library's 64.64 sums are exact), beyond the 1e-12 of the comparison.  A sum of N terms is
    off by at most N * 2^-53 relative; 811 families a block with 7.5 queries each are about 6 100 terms a cell: 7e-13 (asserted)."""
    _gpu_or_fail()
    assert group_layout(6, 2000) == (True, [2, 2, 2, 2, 2, 2])
    fam = Families(12, 7, 2000, [[1, 1, 1, 1, 1, 1]] * 270_000, seed=77, blocks=333)
    assert 1_600_000 <= fam.ix.kmer.shape[0] <= 1_620_000
    every = np.concatenate((fam.queries(), fam.variants()))
    rng = np.random.default_rng(78)
    q = np.concatenate((every, every[rng.integers(0, every.shape[0], size=400_000)]))
    keys, res = check(fam, 12, 7, q, 8, seed=6, again=True)
    terms = max((lv + 1) * res.count_all[lv].max() for lv in range(6))      # (a term at level lv is 1 / (lv + 1) at least)
    assert terms * 2.0 ** -53 < 8e-13
    assert keys > 3 * ROUND and keys % ROUND != 0
