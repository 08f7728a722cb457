"""The lookup stage at the end of kasa_batch_sort_and_range on the hand-made corpus of tests/lookup_corpus.py, against that
file's plain reference: the sorted queries, then per sorted query the deepest matched level and the representative index
position as kasa_batch_fetch_lookup returns them -- through lookup_tile_kernel (flags 0: tile_bounds_kernel, spans staged on
chip up to 1536 records) and through lookup_kernel (debug flag 2).  What the stage leaves per tile and level (the first
closing position, and from it tileNext) has no tap: the families that depend on it -- groups open over tiles and over a chunk
of 1024 tiles -- are compared through profile tables and per-read scores, whose float32 bits follow the flush order.
tests/test_lookup_corpus_cpu.py shows that the corpus holds every category it is meant to."""
import functools
import time

import numpy as np
import pytest

from kasa_amd import capi
from oracle import oracle
from tests import helpers, lookup_corpus as lc
from tests.test_gpu_parity import assert_csr_equal, csr_rows

pytestmark = pytest.mark.gpu

LOOKUP_FLAGS = (0, 2)              # lookup_tile_kernel; lookup_kernel
SCORE_FLAGS = (0, 1)               # the score kernels as chosen; every read through the general kernel or the replay
SCORED = lc.SCORED                 # the open-group cases; a staged and an unstaged batch of the others per key width


class _Devices:
    """one DeviceIndex per index of the corpus, made when first asked for"""

    def __init__(self):
        self.dix = {}

    def index(self, case):
        if case.index not in self.dix:
            self.dix[case.index] = capi.DeviceIndex(case.ix)
        return self.dix[case.index]

    def close(self):
        for d in self.dix.values():
            d.close()


@pytest.fixture(scope="module")
def devices():
    assert capi.device_count() > 0, "no HIP device visible: the lookup corpus needs a real MI355X"
    d = _Devices()
    yield d
    d.close()


def _sort_and_range(devices, case, window, flags):
    ctx = capi.Context(devices.index(case), window[0], window[1], 3)
    ctx.debug_flags(flags)
    ctx.set_queries(case.q, case.payload, case.n_reads)
    ctx.sort_and_range()
    return ctx


def _same(case, window, flags, what, got, want, where=None):
    """got == want at every sorted position (of `where`); else the failure names the first one"""
    bad = np.flatnonzero((got != want) if where is None else ((got != want) & where))
    if bad.shape[0] == 0:
        return
    p = int(bad[0])
    t = p // lc.TILE
    span = int(case.spans[t, 0])
    pytest.fail("%s, k %d..%d, flags %d: %s differs at %d sorted positions, first at %d (tile %d, p %% 4 = %d, the tile's span %d: %s): %d, reference %d"
                % (case.name, window[0], window[1], flags, what, bad.shape[0], p, t, p % 4, span, "staged" if span <= lc.LSPAN else "not staged", int(got[p]), int(want[p])))


def _check_sorted(case, ctx, flags):
    km, rd = ctx.queries()
    want_km, want_rd = case.sorted
    assert np.array_equal(km, want_km), (case.name, flags, "sorted keys")
    assert np.array_equal(rd, want_rd), (case.name, flags, "payload: equal keys out of their order", int(np.flatnonzero(rd != want_rd)[0]))


@pytest.mark.parametrize("name", lc.case_names())
def test_lookup(devices, name):
    """queries() = the stable sort of the shuffled input, keys and payload; depth = the reference everywhere, rep = the reference
    wherever the query matches, and the same through both kernels where it does not."""
    case = lc.case(name)
    t0 = time.perf_counter()
    compared = 0
    for window in case.windows:
        ref = lc.reference(name, *window)
        reps = {}
        for flags in LOOKUP_FLAGS:
            ctx = _sort_and_range(devices, case, window, flags)
            _check_sorted(case, ctx, flags)
            depth, rep = ctx.lookup()
            ctx.close()
            _same(case, window, flags, "depth", depth, ref.depth)
            _same(case, window, flags, "rep", rep, ref.rep, ref.depth > 0)
            reps[flags] = rep
            compared += case.n
        _same(case, window, 0, "rep of an unmatched query (against flags 2)", reps[0], reps[2], ref.depth == 0)
    staged = int((case.spans[:, 0] <= lc.LSPAN).sum())
    print("\nlookup corpus %s: %d queries compared (%d windows, 2 kernels), %d staged tiles, %d not staged, %.2f s"
          % (name, compared, len(case.windows), staged, case.spans.shape[0] - staged, time.perf_counter() - t0))


@functools.lru_cache(maxsize=None)
def _oracle_scores(name, window):
    case = lc.case(name)
    p = oracle.params(window[0], window[1], 3, K=case.letters)
    iv = oracle.IndexView(case.ix)
    qs, rd = case.sorted
    a, b = oracle.ranges(iv, p, qs)
    res = oracle.compare(iv, p, qs, rd, a, b, case.n_reads, True, closed_form=False)
    return res, helpers.csr_from_dense(res.M)


@pytest.mark.parametrize("score_flags", SCORE_FLAGS, ids=["kernels_as_chosen", "general_kernel"])
@pytest.mark.parametrize("lookup_flags", LOOKUP_FLAGS, ids=["lookup_tile", "lookup_per_query"])
@pytest.mark.parametrize("name", SCORED)
def test_scores(devices, name, lookup_flags, score_flags):
    """Profile tables and per-read scores (as bits: an event out of flush order shows there) against the oracle, for the
    open-group families and a staged and an unstaged batch of the others.  Every score path takes a group's flush position
    beyond its tile from tileNext (the group kernels write it into the records); with debug flag 1 all reads go through the
    general kernel or the replay, which compute the positions anew from tileNext (flush_positions_kernel)."""
    case = lc.case(name)
    t0 = time.perf_counter()
    for window in case.score_windows:
        res, rows = _oracle_scores(name, window)
        ctx = _sort_and_range(devices, case, window, lookup_flags | score_flags)
        ctx.lookup_score(True, coverage=False)
        general, _ = ctx.counters()
        st = ctx.batch_stats()
        ca, cu, _ = ctx.profile()
        got = csr_rows(*ctx.scores())
        ctx.close()
        print("\nlookup corpus scores %s flags %d: %d reads, %d on the general kernel, %d replayed, %d dense" % (name, lookup_flags | score_flags, case.n_reads, general, st["replay_reads"], st["dense_reads"]), end="")
        if score_flags & 1:
            assert general + st["replay_reads"] == case.n_reads, (name, general, st)
        assert np.array_equal(cu, res.count_unique), (name, window, lookup_flags, score_flags)
        np.testing.assert_allclose(ca, res.count_all, rtol=1e-12, atol=0)
        assert_csr_equal(got, rows)
    print("\nlookup corpus scores %s: %.2f s" % (name, time.perf_counter() - t0))
