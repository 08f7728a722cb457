"""The score_other* kernels: the other taxa's staging records of the reads score_main_kernel kept.  Every case compares the
profile tables and the per-read scores (as bits: a record out of flush order shows there) with the oracle, once through the
flat kernel of the record width (flags 0: score_other_flat_kernel, score_other_flat16_kernel) and once through the per-lane
kernel (flags 32: score_other_kernel<8, *> and <16, *>)."""
import ctypes as C
import functools

import numpy as np
import pytest

from kasa_amd import capi, formats, reads
from oracle import oracle
from tests import helpers
from tests.test_gpu_parity import (_check_against_oracle, _gpu_or_fail, assert_csr_equal, crowded_wide_world, csr_rows,
                                   synthetic_world)
from tests.test_oracle_properties import random_case

pytestmark = pytest.mark.gpu

FLAGS = [0, 32]
FLAG_IDS = ["flat", "per_lane"]
SEEDS = [1, 13, 14, 16, 21]                   # of test_adversarial_queries_vs_oracle's cases; see test_adversarial_seeds_reach_every_branch
LIVE, POOL, SPLIT, SAT, DEEP = 0, 1, 2, 3, 8   # counters of kasa_debug_record_stats


@functools.lru_cache(maxsize=None)
def adversarial_case(seed):
    """The case test_adversarial_queries_vs_oracle builds for `seed` (at most 3000 index entries, 6000 queries and 50 reads:
    reads begin and end inside wavefronts), with the oracle's result."""
    rng = np.random.default_rng(5000 + seed)
    letters = [[1, 2], [1, 2, 30], [3, 4, 5, 30, 31], list(range(1, 21))][seed % 4]
    k_low = int(rng.integers(5, 12))
    k_high = int(rng.integers(k_low, 13))
    n_taxa = int(rng.integers(2, 40))
    n_reads = int(rng.integers(1, 50))
    ix, q, rd = random_case(seed, int(rng.integers(1, 3000)), int(rng.integers(5, 6000)), n_taxa, letters, k_high, k_low, n_reads)
    return query_case(ix, q, rd, n_reads, k_high, k_low)


def query_case(ix, q, rd, n_reads, k_high, k_low):
    p = oracle.params(k_high, k_low, 3)
    iv = oracle.IndexView(ix)
    qs, rs_ = oracle.sort_queries(q, rd)
    a, b = oracle.ranges(iv, p, qs)
    res = oracle.compare(iv, p, qs, rs_, a, b, n_reads, True, closed_form=False)
    return ix, q, rd, n_reads, k_high, k_low, res


def run_queries(case, flags):
    """Scores the case's queries, checks tables and scores against the oracle; returns kasa_debug_record_stats' counters."""
    ix, q, rd, n_reads, k_high, k_low, res = case
    dix = capi.DeviceIndex(ix)
    ctx = capi.Context(dix, k_high, k_low, 3)
    ctx.debug_flags(flags)
    ctx.set_queries(q, rd, n_reads)
    ctx.sort_and_range()
    ctx.lookup_score(True, coverage=False)
    stats = np.zeros(32, np.uint64)
    L = capi.lib()
    L.kasa_debug_record_stats.argtypes = [C.c_void_p, C.c_void_p]
    rc = L.kasa_debug_record_stats(ctx.h, stats.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    ca, cu, _ = ctx.profile()
    assert np.array_equal(cu, res.count_unique)
    np.testing.assert_allclose(ca, res.count_all, rtol=1e-12, atol=0)
    assert_csr_equal(csr_rows(*ctx.scores()), helpers.csr_from_dense(res.M))
    ctx.close(); dix.close()
    return stats


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("seed", SEEDS)
def test_narrow_adversarial(seed, flags):
    """32-byte records; tiny alphabets and tens of taxa: pool blocks, split queries, saturated level counts, long segments."""
    _gpu_or_fail()
    run_queries(adversarial_case(seed), flags)


def test_adversarial_seeds_reach_every_branch():
    """Conditions on the inputs of test_narrow_adversarial, so that another choice of SEEDS cannot silently stop reaching a
    branch of the kernels.  Summed over SEEDS = [1, 13, 14, 16, 21]: 1596 live queries, 137 queries with a pool
    block, 24 split queries, 39 REC_SAT queries, 481 segments of three or more levels.  (Of the 24 seeds of that test, 16 have no
    live query at all: every read goes to the general kernel.)"""
    _gpu_or_fail()
    total = sum(run_queries(adversarial_case(seed), 0).astype(object) for seed in SEEDS)
    print("record stats over", SEEDS, {n: int(total[i]) for n, i in (("live", LIVE), ("pool", POOL), ("split", SPLIT), ("sat", SAT), ("deep", DEEP))})
    for name, i in (("live queries", LIVE), ("queries with a pool block", POOL), ("split queries", SPLIT), ("REC_SAT queries", SAT),
                    ("segments of three or more levels", DEEP)):
        assert int(total[i]) > 0, f"no {name} in SEEDS: {[int(x) for x in total]}"


@functools.lru_cache(maxsize=None)
def world(*args, **kw):
    return synthetic_world(*args, **kw)


def check_world(ix, batch, k_high, k_low, flags):
    """Tables and scores against the oracle -- and the fast path kept reads, so the score_other kernel of `flags` had work: a
    read the general kernel scores (after a fallback, or all of them once a pool retry has made the context sticky) passes them by."""
    slow = _check_against_oracle(ix, batch, k_high, k_low, 3, flags)
    print("reads of the general kernel:", slow, "of", batch.n)
    assert slow < batch.n // 2, f"{slow} of {batch.n} reads went to the general kernel"


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("krange", [(12, 6), (12, 5)], ids=["7_levels", "8_levels"])
def test_narrow_seven_and_eight_levels(krange, flags):
    """With eight events the flush order fills its 24 bits: order_pos8 masks nothing out."""
    _gpu_or_fail()
    ix, batch = world(21, 8, 6000, 300)
    check_world(ix, batch, krange[0], krange[1], flags)


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("krange", [(25, 7), (25, 20), (18, 13), (25, 5)], ids=["19_levels", "6_levels", "6_levels_from_18", "21_levels"])
def test_wide_few_taxa(krange, flags):
    """64-byte records: score_other_flat16_kernel with its table of 19 rows (up to 19 levels) and of 25 (-k 25 5)."""
    _gpu_or_fail()
    ix, batch = world(61, 8, 6000, 400, K=25)
    check_world(ix, batch, krange[0], krange[1], flags)


@functools.lru_cache(maxsize=None)
def crowded(n_taxa):
    return crowded_wide_world(n_taxa)


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("n_taxa", [30, 300], ids=["lists_of_tens", "lists_of_hundreds"])
def test_wide_crowded(n_taxa, flags):
    """The world of test_wide_records_on_large_taxon_sets.  Measured on an MI355X: its rows are longer than the fast path takes, and
    all 80 reads go to the general kernel (79 to 80 of 80 from 8 taxa on) -- so this checks the hand-over and the scores, and the
    score_other kernels get their long lists from test_wide_shared_stretch below."""
    _gpu_or_fail()
    ix, batch = crowded(n_taxa)
    _check_against_oracle(ix, batch, 25, 7, 3, flags)


@functools.lru_cache(maxsize=None)
def shared_stretch_world(n_taxa, stretch):
    """A 128-bit index of n_taxa random 200-base genomes that share `stretch` bases in the middle, and 80 reads of 150 bases: every
    read spans the stretch, a query inside it meets all n_taxa taxa (more segments than the 8 a wide record holds inline: a pool
    block), a query outside it one -- so a wavefront of 64 queries has hundreds of items, while the read's row stays within what
    the fast path takes."""
    rng = np.random.default_rng(29)
    alphabet = np.frombuffer(b"ACGT", dtype=np.uint8)
    L = 200
    shared = alphabet[rng.integers(0, 4, size=stretch)]
    genomes = []
    for g in range(n_taxa):
        s = alphabet[rng.integers(0, 4, size=L)]
        s[(L - stretch) // 2:(L - stretch) // 2 + stretch] = shared
        genomes.append(s)
    content = formats.Content(["non_unique"] + [f"T{g}" for g in range(n_taxa)],
                              np.concatenate(([0], 100 + np.arange(n_taxa))).astype(np.uint32))
    p = oracle.params(25, 7, 3, K=25)
    kms, tids = [], []
    for g, s in enumerate(genomes):
        km, _ = oracle.encode(s, np.array([0, L], dtype=np.int64), p)
        kms.append(km); tids.append(np.full(km.shape[0], 100 + g, dtype=np.uint32))
    ix = formats.make_index(np.concatenate(kms), np.concatenate(tids), content)
    return ix, reads.synthetic_reads(genomes, 80, 150, 9)


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("n_taxa,stretch", [(12, 30), (24, 30)], ids=["12_taxa", "24_taxa"])
def test_wide_shared_stretch(n_taxa, stretch, flags):
    """Wide queries with a pool block and wavefronts of more than 64 items on the fast path: the carry from round to round of
    the flat kernel's items, and the per-lane kernel's walk over pool segments.  A stretch of 30 bases (ten queries of a read
    reach the lowest level inside it) keeps all 80 reads on the fast path, measured for 10 to 24 taxa; from 45 bases on nine in ten
    go to the general kernel."""
    _gpu_or_fail()
    ix, batch = shared_stretch_world(n_taxa, stretch)
    check_world(ix, batch, 25, 7, flags)


@functools.lru_cache(maxsize=None)
def small_case(seed, n_q, n_reads):
    """The first n_q queries of a random case of n_reads reads."""
    ix, q, rd = random_case(seed, 400, 2 * n_q, 12, list(range(1, 21)), 12, 7, n_reads)
    return query_case(ix, q[:n_q].copy(), rd[:n_q].copy(), n_reads, 12, 7)


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("n_q,n_reads", [(40, 1), (128, 5)], ids=["one_read_below_64", "two_full_wavefronts"])
def test_wavefront_edges(n_q, n_reads, flags):
    """One read and fewer than 64 queries (a padded wavefront); a multiple of 64 (no padding, the items' total at sBase[64]).
    Seed 3 leaves 35 and 117 live queries (most seeds leave none of one read's 40)."""
    _gpu_or_fail()
    stats = run_queries(small_case(3, n_q, n_reads), flags)
    assert int(stats[LIVE]) > 0, "no live query: the score_other kernels had nothing to do"
