"""kasa_batch_rank and kasa_batch_text on hand-made score rows (tests/rank_corpus.py, installed with the test tap
kasa_batch_set_scores) against std::sort itself (tests/rank_reference.cpp) and kasa_amd/report.py's writers: hit counts at
every seam of the kernels, ties inside, on the edge of and beyond the print, rows on which std::sort leaves introsort, the
selection arithmetic at its limits, rank_kernel's output slabs, text_write_kernel's staging buffer at every alignment."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

from kasa_amd import capi, formats, report
from oracle import oracle
from tests import rank_corpus as rc, rank_expect as rx

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in rc.cases()}
FLAGS = (0, 256, 1048576)         # debug flags: none; ties left to the host; every exact class in the largest kernel form


class _World:
    def __init__(self):
        self.taxids, self.names = rc.taxa()
        rng = np.random.default_rng(8)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=300)]
        self.genome = genome
        content = formats.Content(list(self.names), self.taxids.copy())
        km, _ = oracle.encode(genome, np.array([0, genome.shape[0]], dtype=np.int64), oracle.params(12, 7, 3))
        owners = self.taxids[1 + np.arange(km.shape[0]) % 3]                      # a handful of k-mers, three taxa own them
        self.ix = formats.make_index(km, owners.astype(np.uint32), content)
        assert self.ix.content.n_taxa == rc.N_TAXA
        self.dix = capi.DeviceIndex(self.ix)
        self.ctx = {}

    def context(self, case):
        """The case as a loaded batch: reads of three bases, nothing run on them, the case's rows installed."""
        if case.name not in self.ctx:
            ctx = capi.Context(self.dix, 12, 7, 3)
            ctx.upload(np.full(3 * case.n, ord("A"), dtype=np.uint8), np.arange(case.n + 1, dtype=np.int64) * 3)
            ctx.set_taxa_text(self.taxids, self.names)
            ctx.set_scores(case.off, case.tax, case.score)
            self.ctx[case.name] = ctx
        return self.ctx[case.name]

    def close(self):
        for ctx in self.ctx.values():
            ctx.close()
        self.dix.close()


@pytest.fixture(scope="module")
def world():
    assert capi.device_count() > 0
    w = _World()
    yield w
    w.close()


@pytest.fixture
def cached_dtoa(monkeypatch):
    """report.ReadWriter formats the same few numbers again and again: its dtoa behind a cache (the values are unchanged)."""
    monkeypatch.setattr(report, "dtoa", functools.lru_cache(maxsize=None)(report.dtoa))


def _check_entries(case, beasts, flags, meta, ent, n_flag):
    ref, e = rx.reference(case), rx.expected(case, beasts)
    what = (case.name, beasts, flags)
    assert meta.shape == (case.n, 4)
    assert np.array_equal(meta[:, 3].astype(np.int64), ref.cnt), what                                  # the hit count
    assert np.array_equal(meta[:, 2], ref.max_score.view(np.uint32)), what                             # the largest k-mer score, as bits
    flagged = (meta[:, 1] >> 31).astype(bool)
    n = (meta[:, 1] & 0x7FFFFFFF).astype(np.int64)
    assert n_flag == int(flagged.sum()), what
    if flags == 256:                                   # rank_kernel alone: what it must leave, and what it must not
        must = (ref.cnt > rc.RANK_ROWS) | (e.n_print > rc.RANK_CAP) | ((ref.cnt > 16) & e.tie_inside)
        assert flagged[must].all(), (what, np.flatnonzero(must & ~flagged)[:5])
        assert not flagged[ref.cnt <= 16].any(), what
    else:                                              # exactly the reads std::sort heap-sorts where the print needs the whole sort
        assert np.array_equal(flagged, e.flagged), (what, np.flatnonzero(flagged != e.flagged)[:5])
    assert not n[flagged].any()
    un = ~flagged
    assert np.array_equal(n[un], e.n_print[un]), (what, np.flatnonzero(un & (n != e.n_print))[:5])
    rows = np.flatnonzero(un & (n > 0))
    a, k = meta[rows, 0].astype(np.int64), n[rows]
    by_start = np.argsort(a, kind="stable")
    assert ((a + k)[by_start][:-1] <= a[by_start][1:]).all() and (rows.shape[0] == 0 or int((a + k).max()) <= ent.shape[0]), what
    step = np.arange(int(k.sum())) - np.repeat(np.cumsum(k) - k, k)
    got, want = np.repeat(a, k) + step, np.repeat(ref.off[rows].astype(np.int64), k) + step
    assert np.array_equal(ent["tax"][got], ref.tax[want]), what
    assert np.array_equal(ent["score"][got].view(np.uint32), ref.score[want].view(np.uint32)), what
    assert np.array_equal(ent["rel"][got].view(np.uint64), ref.rel[want].view(np.uint64)), what      # bit for bit: IEEE division on both sides
    return rows.shape[0], int(flagged.sum())


@pytest.mark.parametrize("name", list(CASES))
def test_entries(world, name):
    """Every unflagged read's entries = the leading hits of std::sort's order that some writer prints, bit for bit; meta = (first
    entry, count | flag, max k-mer score, hits); entry ranges disjoint and inside nEntries; the flagged reads exactly those the
    reference names (debug flag 256: those rank_kernel must leave, none of up to 16 hits)."""
    case = CASES[name]
    ctx = world.context(case)
    t0 = time.perf_counter()
    checked = left = 0
    for beasts in sorted(set(case.beasts) | {0}):
        for flags in FLAGS:
            ctx.debug_flags(flags)
            meta, ent, n_flag = ctx.rank(case.den, case.rclass, case.threshold, beasts, pinned=False)
            c, f = _check_entries(case, beasts, flags, meta, ent, n_flag)
            checked += c
            left += f if flags == 0 else 0
    ctx.debug_flags(0)
    want_left = sum(int(rx.expected(case, b).flagged.sum()) for b in sorted(set(case.beasts) | {0}))
    assert left == want_left
    print("\nrank corpus %s: %d ranked reads compared, %d left flagged (reference: %d), %.2f s" % (name, checked, left, want_left, time.perf_counter() - t0))


def _text_runs(case):
    """(beasts, first read number): every -b of the case, the first read numbers taken in turn"""
    return [(b, case.first_reads[i % len(case.first_reads)]) for i, b in enumerate(case.beasts)]


@pytest.mark.parametrize("fmt", ["json", "jsonl", "tsv", "kraken"])
@pytest.mark.parametrize("name", list(CASES))
def test_text(world, cached_dtoa, name, fmt):
    """The bytes of kasa_batch_text = report.ReadWriter's over the reference's order, the read offsets = the lengths of its
    pieces, the contamination flags = report.is_contaminant; a batch with a read left to the host gets a state error."""
    case = CASES[name]
    if fmt not in case.formats:
        return                                          # (a text-staging case is cut to the byte for one format)
    ctx = world.context(case)
    ctx.debug_flags(0)
    ref = rx.reference(case)
    t0 = time.perf_counter()
    n_bytes = refused = 0
    for beasts, first in _text_runs(case):
        e = rx.expected(case, beasts)
        _, _, n_flag = ctx.rank(case.den, case.rclass, case.threshold, beasts, pinned=False)
        assert n_flag == int(e.flagged.sum())
        if e.flagged.any():
            assert lib_text_rc(ctx, case, fmt, beasts, first) == 4      # KASA_E_STATE
            refused += 1
            continue
        text, offs, cont = ctx.text(fmt, beasts, first, case.names, case.lengths, case.best)
        want = rx.pieces(case, beasts, fmt, first, world.taxids, world.names)
        size = np.array([len(p) for p in want], dtype=np.uint64)
        assert np.array_equal(offs, np.concatenate(([0], np.cumsum(size, dtype=np.uint64)))), (name, fmt, beasts, first)
        whole = b"".join(want)
        if text != whole:
            at = next(i for i in range(min(len(text), len(whole))) if text[i] != whole[i]) if len(text) == len(whole) else -1
            r = int(np.searchsorted(offs, max(at, 0), side="right") - 1)
            assert False, (name, fmt, beasts, first, "read", r, text[int(offs[r]):int(offs[r + 1])][:300], want[r][:300])
        hit = np.flatnonzero(ref.cnt > 0)
        want_cont = np.zeros(case.n, dtype=np.uint8)
        want_cont[hit] = [report.is_contaminant(case.best[case.rclass[r]], ref.max_score[r]) for r in hit]
        assert np.array_equal(cont, want_cont), (name, fmt, beasts)
        n_bytes += len(whole)
    print("\ntext corpus %s %s: %d bytes compared, %d batches refused, %.2f s" % (name, fmt, n_bytes, refused, time.perf_counter() - t0))


def lib_text_rc(ctx, case, fmt, beasts, first):
    """kasa_batch_text's return code itself"""
    enc = [s.encode("latin-1") for s in case.names]
    off = np.zeros(case.n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in enc], dtype=np.uint64)
    lengths = np.ascontiguousarray(case.lengths, dtype=np.uint32)
    best = np.ascontiguousarray(case.best, dtype=np.float32)
    tp = capi.TextParams(ctx.TEXT_FORMATS[fmt], beasts, first, C.c_char_p(b"".join(enc)), off.ctypes.data_as(C.POINTER(C.c_uint64)),
                         lengths.ctypes.data_as(C.POINTER(C.c_uint32)), best.ctypes.data_as(C.POINTER(C.c_float)), int(best.shape[0]), 0, 0.5, 11.0)
    n = C.c_uint64(0)
    return capi.lib().kasa_batch_text(ctx.h, C.byref(tp), C.byref(n))


def test_text_staging_groups_on_the_device(world):
    """The staging case as the device lays it out: every group of the plan starts at its misalignment and has its bytes (so the
    kernel was at, and one byte over, its LDS buffer for every m)."""
    case = CASES["staging jsonl"]
    (fmt, first), plan = next(iter(case.staging.items()))
    ctx = world.context(case)
    ctx.rank(case.den, case.rclass, case.threshold, case.beasts[0], pinned=False)
    _, offs, _ = ctx.text(fmt, case.beasts[0], first, case.names, case.lengths, case.best)
    for g, (m, total) in plan.items():
        assert int(offs[g * 64]) % 16 == m and int(offs[g * 64 + 64] - offs[g * 64]) == total


def test_set_scores_tap(world):
    """kasa_batch_set_scores: what was given comes back from kasa_batch_scores_fetch -- right after an upload with nothing else
    run, and over the rows of a complete run; rank and text results of the batch become invalid; every refusal of the header."""
    lib = capi.lib()
    case = CASES["arith"]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    off, tax, sc = case.off.copy(), case.tax.copy(), case.score.copy()
    call = lambda ctx, o, t, s, n: lib.kasa_batch_set_scores(ctx.h, p(o), p(t), p(s), C.c_uint64(n))
    ctx = capi.Context(world.dix, 12, 7, 3)
    assert call(ctx, off, tax, sc, case.n) == 4                                   # KASA_E_STATE: no batch is loaded
    # after a complete run of real reads
    L = 60
    starts = np.arange(case.n) % (world.genome.shape[0] - L)
    bases = np.concatenate([world.genome[s:s + L] for s in starts])
    ctx.run_batch(bases, np.arange(case.n + 1, dtype=np.int64) * L, True)
    own = ctx.scores()
    assert int(own[0][-1]) > 0                                                     # the run left rows of its own
    ctx.set_taxa_text(world.taxids, world.names)
    ctx.rank(case.den, case.rclass, 0.0, 3, pinned=False)
    ctx.text("jsonl", 3, 0, case.names, case.lengths, case.best)
    ctx.set_scores(off, tax, sc)
    with pytest.raises(RuntimeError):                                              # the old ranking is not this batch's any more
        ctx.text("jsonl", 3, 0, case.names, case.lengths, case.best)
    for c in (ctx, world.context(case)):                                           # (the second: right after its upload)
        o, t, s = c.scores()
        assert np.array_equal(o, off) and np.array_equal(t, tax) and np.array_equal(s.view(np.uint32), sc.view(np.uint32))
    meta, ent, n_flag = ctx.rank(case.den, case.rclass, case.threshold, 3, pinned=False)
    _check_entries(case, 3, 0, meta, ent, n_flag)
    # refusals: KASA_E_ARG
    assert call(ctx, off[:-1], tax, sc, case.n - 1) == 1                           # not the batch's read count
    bad = off.copy(); bad[0] = 1
    assert call(ctx, bad, tax, sc, case.n) == 1                                    # offsets do not start at 0
    bad = off.copy(); bad[3] = bad[4] + 1
    assert call(ctx, bad, tax, sc, case.n) == 1                                    # offsets descend
    row = next(r for r in range(case.n) if off[r + 1] - off[r] >= 3)
    lo = int(off[row])
    bad = tax.copy(); bad[lo + 1] = rc.N_TAXA
    assert call(ctx, off, bad, sc, case.n) == 1                                    # a taxon index beyond the index's taxa
    bad = tax.copy(); bad[lo + 1] = bad[lo]
    assert call(ctx, off, bad, sc, case.n) == 1                                    # equal neighbours
    bad = tax.copy(); bad[lo], bad[lo + 1] = tax[lo + 1], tax[lo]
    assert call(ctx, off, bad, sc, case.n) == 1                                    # descending
    with pytest.raises(RuntimeError):                                              # a refused call leaves no half-installed rows to rank
        ctx.set_scores(off, bad, sc)
    ctx.set_scores(off, tax, sc)
    o, t, s = ctx.scores()
    assert np.array_equal(o, off) and np.array_equal(t, tax)
    ctx.close()


def test_coherence_column_and_threshold(cached_dtoa):
    """--coherence: the scores of a real run stay when the rows are replaced; kasa_batch_text prints them and flags a read at
    coherence >= coherenceThreshold -- with the threshold on one fetched score, and one ulp above it."""
    from tests.test_gpu_rank import _world
    ix, batch = _world("pairs")
    dix = capi.DeviceIndex(ix)
    ctx = capi.Context(dix, 12, 7, 3)
    ctx.run_batch(batch.bases, batch.offsets, True)
    coh = ctx.coherence()
    n_taxa = ix.content.n_taxa
    rng = np.random.default_rng(6)
    off, tax, sc = [0], [], []
    for r in range(batch.n):
        k = int(rng.integers(0, 6))
        tax.append(np.sort(rng.choice(np.arange(1, n_taxa), size=k, replace=False)))
        sc.append(1.0 + rng.integers(0, 4, k))
        off.append(off[-1] + k)
    case = rc.Case("coherence", np.asarray(off, dtype=np.uint64), np.concatenate(tax).astype(np.uint32), np.concatenate(sc).astype(np.float32),
                   np.ones((1, n_taxa)), np.zeros(batch.n, dtype=np.uint32), np.array([1500.0], dtype=np.float32), batch.names, batch.lengths, beasts=[3])
    ctx.set_scores(case.off, case.tax, case.score)
    ctx.set_taxa_text(ix.content.taxids, ix.content.names)
    ref = rx.reference(case)
    meta, ent, n_flag = ctx.rank(case.den, case.rclass, 0.0, 3, pinned=False)
    _check_entries(case, 3, 0, meta, ent, n_flag)
    pick = coh[ref.cnt > 0]
    at = float(np.sort(pick)[pick.shape[0] // 2])                                  # a score some read with hits has
    seen = set()
    for thr in (np.float32(at), np.nextafter(np.float32(at), np.float32(np.inf))):
        for fmt in ("json", "jsonl", "tsv", "kraken"):
            text, offs, cont = ctx.text(fmt, 3, 0, case.names, case.lengths, case.best, coherence=True, coherence_threshold=float(thr))
            want = rx.pieces(case, 3, fmt, 0, ix.content.taxids, ix.content.names, coherence=coh)
            assert text == b"".join(want), (fmt, float(thr))
            want_cont = ((ref.cnt > 0) & (coh >= thr)).astype(np.uint8)            # (best = 1500: the error rule never fires)
            assert np.array_equal(cont, want_cont)
            seen.add(int(want_cont.sum()))
    assert len(seen) == 2                                                          # the ulp moved a read across
    ctx.close(); dix.close()
