"""kasa_batch_encode on the hand-made reads of tests/encode_corpus.py, form by form: encode_group_kernel, encode_kernel with
192 and with 512 ranked k-mers a read, encode_kernel with the read id as payload, and its second launch over long sequences --
under 64-bit and 128-bit keys, the built-in codon table and one that tells all code triples apart.  tests/test_encode_corpus_cpu.py
shows on the CPU that every case holds what its family claims, lands in the form it names, and that the plain reference equals
the oracle.

Per case: upload (kasa_batch_upload; kasa_batch_upload_segments for segments; kasa_batch_upload_device for the batch whose
offsets start at 21), encode, then
  - batch_stats()["encoder_ranked"] is what the case says,
  - queries() equals the reference's keys and read ids position by position,
  - payload() (kasa_batch_fetch_payload: qRead as the encoder left it) equals the reference's slots and is a permutation of
    0 .. nQ - 1 where the encoder ranked, the read ids where it did not,
  - a case that a ranking form takes runs once more under debug flag 8: the read-id form on the same input, the same keys.
Everything is integers: plain equality.  A failure names the case, the form, the read, strand, window and letter where the
keys first differ and both keys in hex (encode_corpus.describe_difference).

The contexts are shared by all cases of one (K, kHigh, kLow, frames, table): every case also runs behind some other one.
test_back_to_back does so on a fresh context with chosen neighbours."""
import numpy as np
import pytest

from kasa_amd import capi
from tests import encode_corpus as ec
from tests.test_gpu_parity import _gpu_or_fail, synthetic_world

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    """-> ctx(case): the shared context of the case's geometry on a tiny index of its key width (the encoder never reads the index)"""
    _gpu_or_fail()
    dix, ctxs = {}, {}

    def index(K):
        if K not in dix:
            dix[K] = capi.DeviceIndex(synthetic_world(71 if K == 12 else 96, 4, 3000, 10, K=K)[0])
        return dix[K]

    def ctx(c, fresh=False):
        key = (c.K, c.k_high, c.k_low, ec.FRAMES[c.mode], c.lut)
        if fresh:
            return capi.Context(index(c.K), c.k_high, c.k_low, ec.FRAMES[c.mode], np.array(ec.table(c.lut)))
        if key not in ctxs:
            ctxs[key] = capi.Context(index(c.K), c.k_high, c.k_low, ec.FRAMES[c.mode], np.array(ec.table(c.lut)))
        return ctxs[key]

    yield ctx
    for x in list(ctxs.values()) + list(dix.values()):
        x.close()


def encode_on_device(ctx, c, debug):
    """-> keys, read ids, payload words, encoder_ranked of the case under the debug flags"""
    bases, off = c.batch()
    ctx.set_protein(c.mode == "protein")
    ctx.debug_flags(debug)
    bufs = []
    try:
        if c.seg_read is not None:
            ctx.upload(bases, off, np.asarray(c.seg_read, dtype=np.uint32), c.n_reads)
        elif c.shift:
            bufs = [capi.DeviceBuffer(bases.nbytes + 64), capi.DeviceBuffer(off.nbytes)]
            bufs[0].write(bases)
            bufs[1].write(off)
            ctx.upload_resident(bufs[0].ptr, bufs[1].ptr, len(c.seqs))
        else:
            ctx.upload(bases, off)
        n = ctx.encode()
        ranked = ctx.batch_stats()["encoder_ranked"]
        km, rd = ctx.queries()
        pay = ctx.payload()
        assert n == km.shape[0] == pay.shape[0]
        return km, rd, pay, ranked
    finally:
        ctx.debug_flags(0)
        for b in bufs:
            b.close()


def first_bad(got, want):
    return int(np.flatnonzero(got != want)[0])


def check(ctx, c, with_flag8=True):
    e = ec.expected(c)
    what = "%s [%s; %s]" % (c.name, c.form, c.why)
    km, rd, pay, ranked = encode_on_device(ctx, c, c.debug)
    assert ranked == int(c.ranked), "%s: encoder_ranked %d" % (what, ranked)
    assert km.shape == e.keys.shape and np.array_equal(km, e.keys), "%s: %s" % (what, ec.describe_difference(c, km, e.keys))
    assert np.array_equal(rd, e.read), "%s: read ids differ, first at k-mer %d" % (what, first_bad(rd, e.read))
    n = e.keys.shape[0]
    if c.ranked:
        if not np.array_equal(pay, e.slot):
            i = first_bad(pay, e.slot)
            first = int(e.read_count[:int(e.read[i])].sum())
            raise AssertionError("%s: slots differ at %d of %d k-mers, first at k-mer %d (read %d, its k-mer %d of %d, key %x): slot %d, expected %d"
                                 % (what, int((pay != e.slot).sum()), n, i, int(e.read[i]), i - first, int(e.read_count[int(e.read[i])]), ec.key_int(e.keys[i]), int(pay[i]), int(e.slot[i])))
        assert np.array_equal(np.sort(pay), np.arange(n, dtype=np.uint32)), "%s: the slots are no permutation" % what
        if with_flag8:                                                                   # the read-id form on the same input
            km8, rd8, pay8, ranked8 = encode_on_device(ctx, c, c.debug | 8)
            assert ranked8 == 0, what
            assert np.array_equal(km8, e.keys), "%s under flag 8: %s" % (what, ec.describe_difference(c, km8, e.keys))
            assert np.array_equal(rd8, e.read) and np.array_equal(pay8, e.read), "%s under flag 8: the payload is not the read id" % what
    else:
        assert np.array_equal(pay, e.read), "%s: the payload is not the read id, first at k-mer %d" % (what, first_bad(pay, e.read))


@pytest.mark.parametrize("name", ec.case_names())
def test_case(device, name):
    """every case of every family under the form it is built for (and, where that form ranks, under the read-id form); the
    cases of K = 25 are the 128-bit runs of alphabet, codons, geometry and bounds"""
    c = ec.case(name)
    check(device(c), c)


def test_second_sweep_of_the_long_launch(device):
    """one sequence of a whole sweep of the second launch's grid, a chunk and 7 windows: 4.2 M bases, the one case that moves more
    than a few hundred kilobytes"""
    c = ec.case("long K12 dna3 second sweep")
    check(device(c), c)


BACK_TO_BACK = [("long K12 dna3 %d" % (ec.ENC_LONG_MIN + 1), "bounds K12 dna3 %d" % (ec.SMALL_RM + 1)),
                ("bounds K12 dna3 %d" % (2 * ec.ENC_CHUNK + 1), "group_parts zeros"),
                ("group_parts totals", "geometry K12 dna3 none without k-mers"),
                ("bounds K12 dna6 2x%d" % (ec.ENC_RANK_MAX // 2), "bounds K12 dna6 2x%d" % (ec.SMALL_RM // 2 - 1)),
                ("bounds K25 dna3 %d" % (ec.ENC_RANK_MAX + 1), "bounds K25 dna3 %d" % ec.SMALL_RM),
                ("segments K12 dna3", "segments K12 dna3 as reads"),
                ("long K12 dna3 pair of 40000", "group_parts many")]


@pytest.mark.parametrize("a,b", BACK_TO_BACK)
def test_back_to_back(device, a, b):
    """two different cases on one fresh context, a b a b: a longer batch before a shorter one, another form, segments before
    plain reads, a batch without any k-mer -- nothing of the first may show in the second"""
    ca, cb = ec.case(a), ec.case(b)
    assert (ca.K, ca.k_high, ca.k_low, ec.FRAMES[ca.mode], ca.lut) == (cb.K, cb.k_high, cb.k_low, ec.FRAMES[cb.mode], cb.lut)
    ctx = device(ca, fresh=True)
    try:
        for c in (ca, cb, ca, cb):
            check(ctx, c, with_flag8=False)
    finally:
        ctx.close()


def test_payload_tap_states(device):
    """kasa_batch_fetch_payload: only between kasa_batch_encode and the sort; it changes nothing"""
    c = ec.case("group_parts many")
    ctx = device(c, fresh=True)
    try:
        with pytest.raises(RuntimeError, match="kasa_batch_fetch_payload"):
            ctx.payload()
        bases, off = c.batch()
        ctx.upload(bases, off)
        with pytest.raises(RuntimeError, match="kasa_batch_fetch_payload"):
            ctx.payload()
        ctx.encode()
        p1, q1 = ctx.payload(), ctx.queries()
        p2, q2 = ctx.payload(), ctx.queries()
        assert np.array_equal(p1, p2) and np.array_equal(q1[0], q2[0]) and np.array_equal(q1[1], q2[1]) and np.array_equal(p1, ec.expected(c).slot)
        ctx.sort_and_range()
        with pytest.raises(RuntimeError, match="kasa_batch_fetch_payload"):
            ctx.payload()
        e = ec.expected(c)
        ctx.set_queries(e.keys, e.read, c.n_reads)                                       # queries from outside: not the encoder's
        with pytest.raises(RuntimeError, match="kasa_batch_fetch_payload"):
            ctx.payload()
    finally:
        ctx.close()
