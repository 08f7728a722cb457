"""The query sort on the hand-made batches of tests/sort_corpus.py, both key widths: kasa_radix.h's hist_kernel, starts_kernel
and pass_kernel, then the bucket kernels and the long-bucket path of sort_and_range_impl, through Context.set_queries ->
sort_and_range -> queries.  tests/test_sort_corpus_cpu.py shows on the CPU that every case holds what its family claims, in
the order in which the named pass reads the pairs.

Every expectation is numpy's stable sort of the batch (np.argsort(kind="stable"), np.lexsort((lo, hi))), keys and payloads
compared with np.array_equal; the payloads are a permutation of 0 .. n - 1.  Every case runs under the product path (flags
0), the look-back first (524288), the other split of passes and buckets (2097152), for 64-bit keys the bucket kernel for any
key width (4194304), and two controls: the library's passes over the same bits (512) and the library over all bits (64).  A
failure that spares the controls points at the hand-written kernels.  The chain cases -- 530 tiles, more than the 512
workgroups of pass_kernel that the chip holds at once -- run under 0, 524288 and 64; the buckets of 2^20 and 2^20 + 1
members under 0 and 128.  The index is the tiny one of synthetic_world: the lookup that follows the sort must simply not fail.

Out of scope: the branch for more than 2^18 long buckets (SORT_BIG_CAP) needs at least 2^28 pairs.

The builder's full-width sort (flush_brick: 8 passes for 64-bit keys, 16 for 128-bit ones) gets two skewed inputs at the end.

Durations on an MI355X (pytest --durations=15), the file's 451 tests in 9.9 s: test_chain 0.40 to 0.66 s a case (one digit,
64-bit keys, pass 0 the slowest; 128-bit keys 0.40 to 0.51 s), test_back_to_back 0.59 s (64-bit) and 0.41 s (128-bit), the two
contexts' setup 0.31 s once, test_longest_bucket 0.13 s; every other test, the builder's included, stays below that."""
import numpy as np
import pytest

from kasa_amd import capi, formats
from oracle import oracle
from tests import sort_corpus as sc
from tests.test_gpu_parity import _gpu_or_fail, synthetic_world

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs():
    _gpu_or_fail()
    made = {}
    for width in sc.WIDTHS:
        K = sc.LETTERS[width]
        ix, _ = synthetic_world(71 if width == 64 else 71 + K, 4, 3000, 10, K=K)
        dix = capi.DeviceIndex(ix)
        made[width] = (capi.Context(dix, K, 7, 3), dix)
    yield {w: c for w, (c, _) in made.items()}
    for c, dix in made.values():
        c.close(); dix.close()


def sort_on_device(ctx, keys, payload, flags):
    ctx.debug_flags(flags)
    try:
        ctx.set_queries(keys, payload, keys.shape[0])
        ctx.sort_and_range()
        return ctx.queries()
    finally:
        ctx.debug_flags(0)


def check(ctx, c, expect=None, flags=None):
    ks, ps = expect or sc.reference(c.keys, c.payload)
    for f in flags or c.flags:
        km, rd = sort_on_device(ctx, c.keys, c.payload, f)
        assert km.shape[0] == c.n, f"{c.name}, flags {f}: {km.shape[0]} pairs of {c.n}"
        assert np.array_equal(km, ks), f"{c.name}, flags {f}: keys differ, first at {sc.first_difference(km, ks)} of {c.n}"
        assert np.array_equal(rd, ps), f"{c.name}, flags {f}: payloads differ, first at {sc.first_difference(rd, ps)} of {c.n}"


@pytest.mark.parametrize("name", [n for f in ("one_digit", "ends", "rows", "tile_runs", "descending") for n in sc.case_names(f)])
def test_pass_families(ctxs, name):
    """A digit pattern in one pass of the product path: one digit per tile; digits 0 and 255 only; rows of 64 distinct digits, of
    one digit, stripes of one digit, lanes 0 and 63 alone with a digit; a digit's run of a tile's length at a tile's edge, a digit
    only in a partial last tile, only in the first and last tile; digits that fall, in runs of 1 to T pairs."""
    c = sc.case(name)
    check(ctxs[c.width], c)


@pytest.mark.parametrize("name", sc.case_names("buckets128"))
def test_wide_buckets(ctxs, name):
    """bucket_rank_kernel<Key128> on buckets laid out by hand, their low part of 85 bits (the product path) and of 93: batch
    sizes, alignments, rows, the limit, tile boundaries and halo, both ends, singletons, one bucket, neighbours, and low parts
    that only a right 128-bit compare orders."""
    c = sc.case(name)
    check(ctxs[c.width], c)


@pytest.mark.parametrize("name", sc.case_names("long"))
def test_long_buckets(ctxs, name):
    """bucket_bounds_kernel and the segmented sort: long buckets at position 0, over a tile boundary, ending at n, side by side,
    three in a batch."""
    c = sc.case(name)
    check(ctxs[c.width], c)


@pytest.mark.parametrize("name", sc.case_names("long", large=True))
def test_longest_bucket(ctxs, name):
    """SORT_BIG_LONGEST members are the last the segmented sort takes; one more, and the library sorts over all bits."""
    c = sc.case(name)
    check(ctxs[c.width], c)


@pytest.mark.parametrize("name", sc.case_names("chain", large=True))
def test_chain(ctxs, name):
    """530 tiles: the last workgroups take their tile numbers only after earlier ones have retired, and look back over them."""
    c = sc.case(name)
    check(ctxs[c.width], c)


@pytest.mark.parametrize("width", sc.WIDTHS)
def test_back_to_back(ctxs, width):
    """On one context a chain batch, then one pair, then a batch of one digit: nothing of the earlier batch is left in the
    histogram, the tile counter or the look-back words."""
    ctx = ctxs[width]
    chain = sc.case("chain/one digit/%d/pass 1" % width)
    chain_sorted = sc.reference(chain.keys, chain.payload)
    one = sc.Case("one pair", "back_to_back", width, chain.keys[:1].copy(), np.zeros(1, dtype=np.uint32), ())
    digit = sc.case("one_digit/one pass/%d/pass 1" % width)
    for f in (sc.PRODUCT, sc.FIRST):
        check(ctx, chain, chain_sorted, (f,))
        check(ctx, one, None, (f,))
        check(ctx, digit, None, (f,))


# ---- the builder's sort over all key bits, under skew ---------------------------------------------------------------------------
def _skewed(which):
    if which == "homopolymers":                                  # every pass of more than two tiles sees a single digit
        seqs, taxa = [np.full(10000, ord(ch), dtype=np.uint8) for ch in "ALW"], [1, 2, 3]
    else:                                                        # one sequence of period two
        seqs, taxa = [np.tile(np.frombuffer(b"AL", dtype=np.uint8), 5000)], [2]
    off = np.concatenate(([0], np.cumsum([s.shape[0] for s in seqs]))).astype(np.int64)
    return np.concatenate(seqs), off, taxa


@pytest.mark.parametrize("K", [12, 25])
@pytest.mark.parametrize("brick", [0, 4099])
@pytest.mark.parametrize("which", ["homopolymers", "period two"])
def test_builder_sorts_skewed_pairs(which, brick, K):
    """flush_brick's radix sort over all key bits on amino-acid sequences of one letter (one per taxon, three taxa) and of two
    letters in turn, in one brick and in a brick per sequence: the index of the oracle's pairs (kLow = 1) of the same sequences."""
    _gpu_or_fail()
    content = formats.Content(["non_unique", "Taxon 1", "Taxon 2", "Taxon 3"], np.asarray([0, 11, 22, 33], dtype=np.uint32))
    bases, off, taxa = _skewed(which)
    seq_taxid = content.taxids[np.asarray(taxa)]
    km, seq = oracle.encode(bases, off, oracle.params(K, 1, 3, K=K, protein=True))
    want = formats.make_index(km, seq_taxid[seq], content)
    b = capi.Builder(content.taxids, K, 3, None, brick)
    b.add(bases, off, seq_taxid, protein=True)
    n, m = b.finish()
    got_km, got_tax, tp, tc, freq = b.fetch()
    st = b.stats()
    b.close()
    assert st["pairs_in"] == km.shape[0] == int(off[-1]) and st["bricks"] == (len(taxa) if brick else 1)
    assert n == want.n and m == want.trie_prefix.shape[0]
    assert np.array_equal(got_km, want.kmer), f"k-mers differ, first at {sc.first_difference(got_km, want.kmer)} of {n}"
    assert np.array_equal(got_tax, want.taxid)
    assert np.array_equal(tp, want.trie_prefix) and np.array_equal(tc, want.trie_count)
    assert np.array_equal(freq, want.freq)
