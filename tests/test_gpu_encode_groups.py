"""The encoder's group form (encode_group_kernel: one wavefront per group of consecutive short reads, ranking in 256 buckets
per read) against what it bypasses: the oracle's encoder for the keys, debug flag 8 (slots from a stable sort by read instead of
the encoder's ranking) and debug flag 64 (the library sort over all key bits) for everything behind it.

What the C ABI shows of a slot is the read it lies in (kasa_batch_fetch_queries turns slots back into read ids), so the ranks
inside a read are checked through what they decide: the records of a read are written to its slots and scored in slot order --
two k-mers on one slot lose an event, two in the wrong order change the groups and the float sums.  The per-read rows and the
profile tables must equal those of the flag-8 run and of the oracle bit for bit.

A DNA read in three frames has no k-mer or at least three (L > 3 K + 1 bases give L - 3 K + 1 windows): reads of exactly one or two
k-mers do not exist, the lists below take 3 and 4 in their place and several lengths that give none."""
import numpy as np
import pytest

from kasa_amd import capi, formats, reads
from oracle import oracle
from tests import helpers
from tests.test_gpu_parity import _gpu_or_fail, assert_csr_equal, csr_rows, synth_genomes_of

pytestmark = pytest.mark.gpu

KMER_COUNTS = [0, 3, 4, 63, 64, 65, 127, 128, 129, 130, 131, 191, 192]     # k-mers of a read; a read of c > 0 k-mers has c + 20 bases (-k 12 7)
_WORLD = {}


def world():
    """A tiny index (6 taxa of 6000 bases, sibling genomes 3 % apart) and the genomes as a pool to cut reads from."""
    if not _WORLD:
        genomes = synth_genomes_of(91, 6, 6000)
        content = formats.Content(["non_unique"] + [f"Taxon {g}" for g in range(6)], np.concatenate(([0], 100 + np.arange(6))).astype(np.uint32))
        p = oracle.params(12, 7, 3)
        kms, tids = [], []
        for g, s in enumerate(genomes):
            km, _ = oracle.encode(s, np.array([0, s.shape[0]], dtype=np.int64), p)
            kms.append(km)
            tids.append(np.full(km.shape[0], 100 + g, dtype=np.uint32))
        _WORLD["ix"] = formats.make_index(np.concatenate(kms), np.concatenate(tids), content)
        _WORLD["pool"] = np.concatenate(genomes)
    return _WORLD["ix"], _WORLD["pool"]


def bases_of(count, rng):
    """Bases of a read with `count` k-mers at -k 12 7 (count 0: one of the lengths too short for a window)."""
    return count + 20 if count else int(rng.choice([0, 1, 22]))


def batch_from(parts):
    lens = [int(p.shape[0]) for p in parts]
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    b = np.concatenate(parts).astype(np.uint8) if sum(lens) else np.zeros(0, dtype=np.uint8)
    return reads.ReadBatch(b, off, None, np.asarray([l + 1 for l in lens], dtype=np.uint32))


def cut_reads(lengths, rng, error=0.01):
    """Reads of the given lengths cut from the genomes, 1 % substitutions."""
    _, pool = world()
    parts = []
    for L in lengths:
        a = int(rng.integers(0, pool.shape[0] - 1024))
        s = pool[a:a + L].copy()
        m = rng.random(L) < error
        s[m] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(m.sum()))]
        parts.append(s)
    return batch_from(parts)


def run(ix_dev, batch, flags, kh=12, kl=7, frames=3, protein=False, score=True):
    """-> (encoded keys, reads), (sorted keys, reads), profile + rows, encoder_ranked."""
    ctx = capi.Context(ix_dev, kh, kl, frames)
    ctx.set_protein(protein)
    ctx.debug_flags(flags)
    ctx.upload(batch.bases, batch.offsets)
    ctx.encode()
    ranked = ctx.batch_stats()["encoder_ranked"]
    enc = tuple(a.copy() for a in ctx.queries())
    ctx.sort_and_range()
    srt = tuple(a.copy() for a in ctx.queries())
    out = None
    if score:
        ctx.lookup_score(True)
        ca, cu, ct = ctx.profile()
        out = (ca.copy(), cu.copy(), ct.copy(), csr_rows(*[a.copy() for a in ctx.scores()]))
    ctx.close()
    return enc, srt, out, ranked


def check_batch(batch, expect_ranked=1, kh=12, kl=7, frames=3, protein=False, against_flag8=True):
    """The product path against the oracle's encoder and sort, the flag-64 sort and (rows, profile) the flag-8 slots and the oracle."""
    ix, _ = world()
    p = oracle.params(kh, kl, frames, protein=protein)
    km_o, rd_o = oracle.encode(batch.bases, batch.offsets, p)
    ks_o, rs_o = oracle.sort_queries(km_o, rd_o)
    dix = capi.DeviceIndex(ix)
    enc, srt, out, ranked = run(dix, batch, 0, kh, kl, frames, protein)
    assert ranked == expect_ranked
    assert np.array_equal(enc[0], km_o) and np.array_equal(enc[1], rd_o)                   # keys and payload, position by position
    assert np.array_equal(srt[0], ks_o) and np.array_equal(srt[1], rs_o)
    _, srt64, _, _ = run(dix, batch, 64, kh, kl, frames, protein, score=False)
    assert np.array_equal(srt[0], srt64[0]) and np.array_equal(srt[1], srt64[1])
    if against_flag8:
        enc8, srt8, out8, ranked8 = run(dix, batch, 8, kh, kl, frames, protein)
        assert ranked8 == 0                                                                  # the independent path: slots from the sort by read
        assert np.array_equal(enc[0], enc8[0]) and np.array_equal(enc[1], enc8[1])
        assert np.array_equal(srt[0], srt8[0]) and np.array_equal(srt[1], srt8[1])
        for a, b in zip(out[:3], out8[:3]):
            assert np.array_equal(a, b)
        assert_csr_equal(out[3], out8[3])
    res, nq = oracle.identify_batch(ix, batch.bases, batch.offsets, p, True)
    assert nq == km_o.shape[0]
    assert np.array_equal(out[1], res.count_unique)
    assert_csr_equal(out[3], helpers.csr_from_dense(res.M))
    dix.close()


def ragged_lengths(n_lists, seed):
    rng = np.random.default_rng(seed)
    counts = np.array(KMER_COUNTS * n_lists)
    rng.shuffle(counts)
    return [bases_of(int(c), rng) for c in counts], rng


def test_group_size_is_exposed():
    _gpu_or_fail()
    assert 2 <= capi.encode_group_reads() <= 16


def test_keys_and_slots_over_ragged_groups():
    """Reads of 0, 3, 4, 63, 64, 65, 127 ... 192 k-mers, the list 250 times over and shuffled: group and round boundaries fall everywhere;
    many groups exceed the k-mers one pass of a wavefront holds and are taken in parts."""
    _gpu_or_fail()
    lengths, rng = ragged_lengths(250, 5)
    check_batch(cut_reads(lengths, rng))


@pytest.mark.parametrize("which", ["1", "G-1", "G", "G+1", "2G+1"])
def test_batches_of_about_one_group(which):
    _gpu_or_fail()
    G = capi.encode_group_reads()
    n = {"1": 1, "G-1": G - 1, "G": G, "G+1": G + 1, "2G+1": 2 * G + 1}[which]
    for seed in (11, 12, 13):                                              # (three draws: zero-k-mer reads at the start, inside, at the end of a group)
        lengths, rng = ragged_lengths(2, seed + n)
        lengths = lengths[:n]
        if not any(L > 22 for L in lengths):
            lengths[-1] = 150
        check_batch(cut_reads(lengths, rng))
    check_batch(cut_reads([212] * n, np.random.default_rng(n)))           # every read at the form's limit: 192 k-mers
    check_batch(cut_reads([0] * (n - 1) + [150], np.random.default_rng(n)))


def test_ranking_worst_cases():
    """Reads whose k-mers are all equal (ranks follow the windows; a bucket of 192 fills a byte counter to its limit), reads of one
    repeated codon pattern (three k-mers, everything in at most three buckets), reads with N, ordinary reads -- mixed in one batch."""
    _gpu_or_fail()
    rng = np.random.default_rng(77)
    _, pool = world()
    parts = []
    for r in range(120):
        kind = r % 6
        if kind == 0:
            parts.append(np.full([150, 212, 151, 83][(r // 6) % 4], ord("ACGT"[(r // 24) % 4]), dtype=np.uint8))
        elif kind == 1:
            pat = [b"GCT", b"AAG", b"ACACAT", b"TTTTTA"][(r // 6) % 4]
            parts.append(np.frombuffer(pat * 40, dtype=np.uint8)[:int(rng.integers(40, 213))].copy())
        elif kind == 2:
            s = cut_reads([int(rng.integers(60, 213))], rng).bases.copy()
            s[rng.integers(0, s.shape[0], size=int(rng.integers(1, 12)))] = ord("N")
            parts.append(s)
        elif kind == 3:                                                    # a genome stretch twice: every k-mer has an equal one in the read
            s = cut_reads([70], rng).bases
            parts.append(np.concatenate([s, s, s])[:int(rng.integers(141, 211))].copy())
        else:
            parts.append(cut_reads([int(rng.integers(23, 213))], rng).bases)
    check_batch(batch_from(parts))


def test_hand_over_to_the_other_forms():
    """Batches the group form does not take: a read of 193 k-mers (the 512-k-mer form of the one-read kernel), six frames, one frame,
    amino-acid input.  Keys equal the oracle's, the sort equals the flag-64 sort and the oracle's, the rows the oracle's."""
    _gpu_or_fail()
    rng = np.random.default_rng(3)
    lengths, _ = ragged_lengths(3, 8)
    check_batch(cut_reads(lengths + [213], rng))                           # 193 k-mers in the last read
    check_batch(cut_reads([213] + lengths, rng))
    check_batch(cut_reads(lengths[:20], rng), frames=6)
    check_batch(cut_reads([150, 30, 600, 0, 151, 333], rng), frames=1)
    _, pool = world()
    lut = oracle.codon_table()
    code = (pool & 14) >> 1
    parts = []
    for L in [0, 5, 12, 13, 14, 50, 64, 100, 130, 192, 30]:
        a = int(rng.integers(0, pool.shape[0] - 3 * 200))
        c = code[a:a + 3 * L].reshape(-1, 3).astype(np.int64)
        aa = (lut[c[:, 0] * 64 + c[:, 1] * 8 + c[:, 2]] + 64).astype(np.uint8)
        aa[aa == ord("[")] = ord("*")
        parts.append(aa)
    lens = [int(p.shape[0]) for p in parts]
    prot = reads.ReadBatch(np.concatenate(parts), np.concatenate(([0], np.cumsum(lens))).astype(np.int64), None,
                           np.asarray([l + 1 for l in lens], dtype=np.uint32), True)
    check_batch(prot, protein=True)


@pytest.mark.parametrize("pairs", [1300, 8192, 8193, 39000], ids=["part_of_a_tile", "one_tile", "one_tile_and_one", "five_tiles"])
def test_sort_behind_the_group_form(pairs):
    """The radix passes take their digit counts from a pass over the keys the encoder wrote; batches that end inside the first tile
    of 8192 pairs, at its end, one pair behind it and in the fifth tile, sorted like the library sort over all bits (flag 64).
    The same context then sorts queries handed in from outside (kasa_batch_set_queries) and two more batches in a row: nothing
    of an earlier batch may be left over."""
    _gpu_or_fail()
    ix, _ = world()
    rng = np.random.default_rng(pairs)
    n130 = (pairs - 132) // 130
    last = pairs - 130 * n130                                              # 132 ... 261 k-mers in one or two more reads
    lengths = [150] * n130 + ([last + 20] if last <= 192 else [last - 130 + 20, 150])
    batch = cut_reads(lengths, rng)
    other = cut_reads([150, 97, 212, 0, 151] * 40, rng)
    p = oracle.params(12, 7, 3)
    dix = capi.DeviceIndex(ix)
    ctx = capi.Context(dix, 12, 7, 3)

    def sorted_pairs(b, flags):
        ctx.debug_flags(flags)
        ctx.upload(b.bases, b.offsets)
        n = ctx.encode()
        ctx.sort_and_range()
        km, rd = ctx.queries()
        return n, km.copy(), rd.copy()

    n, km0, rd0 = sorted_pairs(batch, 0)
    assert n == pairs and ctx.batch_stats()["encoder_ranked"] == 1
    _, km64, rd64 = sorted_pairs(batch, 64)
    assert np.array_equal(km0, km64) and np.array_equal(rd0, rd64)
    ks_o, rs_o = oracle.sort_queries(*oracle.encode(batch.bases, batch.offsets, p))
    assert np.array_equal(km0, ks_o) and np.array_equal(rd0, rs_o)
    # queries from outside on the same context
    ctx.debug_flags(0)
    q = rng.integers(1, 1 << 58, size=pairs + 7, dtype=np.uint64)
    rd = rng.integers(0, 50, size=pairs + 7).astype(np.uint32)
    ctx.set_queries(q, rd, 50)
    ctx.sort_and_range()
    km, r2 = ctx.queries()
    qs, rs_ = oracle.sort_queries(q, rd)
    assert np.array_equal(km, qs) and np.array_equal(r2, rs_)
    # two batches in a row
    for b in (other, batch):
        _, km, r2 = sorted_pairs(b, 0)
        ks, rs = oracle.sort_queries(*oracle.encode(b.bases, b.offsets, p))
        assert np.array_equal(km, ks) and np.array_equal(r2, rs)
    ctx.close(); dix.close()
