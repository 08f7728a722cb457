"""The score stage (kasa_batch_score: score_main_kernel, score_other_flat_kernel / score_other_flat16_kernel / score_other_kernel,
the row merges, score_dense_kernel, score_kernel and its later passes, the sorted-event replay, the staging retry) on the
hand-made reads of tests/score_corpus.py, against the plain replay of the reference's records (group_corpus.replay, which
tests/test_score_corpus_cpu.py holds to the sequential oracle): per read the score row as bits, for 64-byte records the profile
tables too.  The stage is fed the REFERENCE's records -- set_queries, sort_and_range, records_import(encode(reference)),
score(True) -- so that a fault of the group stage can neither mask nor cause a failure here; one run per family scores the
records the product's own group() made instead (fetched and imported again: kasa_batch_group leaves them in sorted order);
the route is still held to facts restated from the reference's records there.

Every case and window runs under every route its record width has (ROUTES: eleven for narrow records, nine for 64-byte ones).  Where score_corpus restates the decision -- which
reads score_main_kernel hands on and why (kasa_ctx_hand_over_reasons), which of those score_dense_kernel keeps, the row-merge
classes, the staged row lengths, the staging records, the profile keys of 64-byte records -- the route taken is asserted, not only the result.  A failure names
case, window, flags, read, taxon, the read's first slot and its phase in a 128-byte line.

MEASURED (MI355X, pytest --durations=0): the file's 96 tests in 15.5 s, 2646 runs (case x window x route) in test_scores.  The
slowest, each with the building of its case and reference: order128 order chunks 1.37 s and pairs 1.20 s (2160 queries, two
windows x nine routes), sizes128 count (120 003 queries) 1.00 s, order128 order single 0.93 s, the three staging batches of 1000
reads 0.63 s, order128 split pairs 0.34 s; everything else below 0.3 s, the eleven tests through group() 0.01 to 0.11 s each.
"""
import functools
import time

import numpy as np
import pytest

from kasa_amd import capi
from tests import group_corpus as gc, helpers, score_corpus as sc
from tests.test_gpu_parity import assert_csr_equal, csr_rows

pytestmark = pytest.mark.gpu

GENERAL, LANE_CELLS, SECOND, THIRD, NO_DENSE, NO_REPLAY, ALL_REPLAY = 1, 8192, 16384, 8388608, 33554432, 536870912, 1073741824
ROUTES = {0: "the product route", 32: "per-lane score_other", 1024: "prefetching score_main", 4: "the sorting merge", GENERAL: "the general kernel for every read",
          GENERAL + LANE_CELLS: "the general kernel, a lane owns its cells", GENERAL + SECOND: "the general kernel's second pass",
          GENERAL + SECOND + THIRD: "the general kernel's third pass", NO_DENSE: "never dense", GENERAL + NO_REPLAY: "the general kernel, never the replay",
          GENERAL + ALL_REPLAY: "the sorted-event replay for every read"}
NARROW_ONLY = (1024, GENERAL + SECOND + THIRD)
FAMILIES = ("take", "phase", "slots", "registers", "order", "sizes", "rule", "rows", "taxa", "dense", "general")


def routes_of(rw):
    return [f for f in ROUTES if rw == 8 or f not in NARROW_ONLY]


class _Devices:
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
    assert capi.device_count() > 0, "no HIP device visible: the score corpus needs a real MI355X"
    d = _Devices()
    yield d
    d.close()


@functools.lru_cache(maxsize=4)
def _expected(name, window):
    """the reference's records in the device's layout and their replay -- once per case and window"""
    kh, kl = window
    case, recs, rw = sc.case(name), sc.ref(name, kh, kl), gc.rec_words(kh, kl)
    rec, pool = gc.encode(recs, rw, kh, kl)
    M, ca, cu = gc.replay(case, recs, kh, kl)
    return rec, pool, helpers.csr_from_dense(M), ca, cu


def _where(case, window, flags, f=None, taxon=None):
    rw = gc.rec_words(*window)
    s = "%s (built for %s), k %d..%d, flags %d (%s)" % (case.name, case.built_for, window[0], window[1], flags, ROUTES[flags])
    if f is not None:
        s += ": read %d of %d queries, first slot %d (slot %d of its 64-slot window, %d records into its line)" % (f.read, f.n, f.first_slot, f.first_slot % sc.TAKE, f.phase(rw))
        s += ", %s" % ("kept by score_main_kernel, a row of %d records, register taxa %s" % (f.row, list(f.regs)) if f.why is None else "handed on for its " + sc.WHY[f.why])
    if taxon is not None:
        s += ", taxon %d" % taxon
    return s


def _check_scores(case, window, flags, scores, want_rows, facts):
    got = csr_rows(*scores)
    assert len(got) == len(want_rows) == case.n_reads, _where(case, window, flags)
    for r, ((tg, sg), (tw, sw)) in enumerate(zip(got, want_rows)):
        if np.array_equal(tg, tw) and np.array_equal(sg.view(np.uint32), sw.view(np.uint32)):
            continue
        g, w = dict(zip(tg.tolist(), sg)), dict(zip(tw.tolist(), sw))
        t = min(t for t in set(g) | set(w) if t not in g or t not in w or g[t].view(np.uint32) != w[t].view(np.uint32))
        pytest.fail("%s: score %r (bits %s), the replay's %r (bits %s); %d taxa in the row, %d in the replay's" % (
            _where(case, window, flags, facts[r], t), g.get(t), g[t].view(np.uint32) if t in g else None, w.get(t), w[t].view(np.uint32) if t in w else None, len(g), len(w)))
    assert_csr_equal(got, want_rows)


def _check_route(case, window, flags, ctx, facts):
    """the route taken, from the context's diagnostics against score_corpus's restatement"""
    st, why, classes = ctx.batch_stats(), ctx.hand_over_reasons(), ctx.row_classes()
    at = _where(case, window, flags)
    with_queries = sum(1 for f in facts if f.n)
    assert st["queries"] == case.n, at
    if flags & GENERAL:
        least = None if flags & NO_REPLAY else (1 if flags & ALL_REPLAY else sc.ESR_MIN_KMERS)      # the replay takes reads of that many queries
        replayed = sum(1 for f in facts if least and f.n >= least)
        assert (st["replay_reads"], st["general_reads"]) == (replayed, case.n_reads - replayed), "%s: %d reads replayed, %d on the general kernel" % (at, st["replay_reads"], st["general_reads"])
        assert st["dense_reads"] == 0 and classes == (0, 0, 0, 0), at
        if flags & SECOND and any(f.taxa and (not least or f.n < least) for f in facts):
            assert st["second_pass_reads"] > 0, at + ": no read on the second pass"
            if flags & THIRD:
                assert ctx.third_pass_reads() > 0, at + ": no read on the third pass"
        return
    want_why = sc.why_counts(facts)
    assert why == want_why, "%s: score_main_kernel handed on %s reads for (%s), the case is built for %s" % (at, list(why), ", ".join(sc.WHY), list(want_why))
    handed = [f for f in facts if f.why is not None]
    rest = [f for f in handed if not f.keeps_rule] if sc.dense_runs(case, window[0], window[1], flags) else handed
    dense = len(handed) - len(rest)
    replayed = sum(1 for f in rest if f.n >= sc.ESR_MIN_KMERS)
    assert (st["dense_reads"], st["replay_reads"], st["general_reads"]) == (dense, replayed, len(rest) - replayed), \
        "%s: %d reads on score_dense_kernel, %d replayed, %d on the general kernel, built for %d, %d and %d" % (
        at, st["dense_reads"], st["replay_reads"], st["general_reads"], dense, replayed, len(rest) - replayed)
    n_taxa = case.ix.content.n_taxa
    bitmap = n_taxa <= sc.BM_WORDS * 32 and not flags & 4
    want_classes = sc.row_classes(facts, n_taxa) if bitmap else (len(facts) - len(handed), 0, 0, 0)
    assert classes == want_classes, "%s: row-merge classes %s, built for %s" % (at, classes, want_classes)
    lengths = ctx.staged_lengths()
    for f in facts:
        if f.why is None and int(lengths[f.read]) != f.row:
            pytest.fail("%s: a staging row of %d records" % (_where(case, window, flags, f), int(lengths[f.read])))
    if not handed:
        assert st["staging_records"] == sum(f.row for f in facts), at
        if gc.rec_words(*window) == 16 and any(f.row for f in facts):      # (the keys of the row merge: 64-byte records, a batch with rows)
            assert st["profile_keys"] == sum(f.keys for f in facts), "%s: %d profile keys, built for %d" % (at, st["profile_keys"], sum(f.keys for f in facts))


def _run_window(devices, case, window, group=False, routes=None):
    kh, kl = window
    rw = gc.rec_words(kh, kl)
    rec, pool, want_rows, ca, cu = _expected(case.name, window)
    ctx = capi.Context(devices.index(case), kh, kl, 3)
    ctx.keep_staged_lengths(True)
    ctx.set_queries(case.q, case.payload, case.n_reads)
    ctx.sort_and_range()
    if group:                                          # (kasa_batch_group leaves its records in sorted order: back in through the import, as a read owner takes them)
        ctx.group()
        ctx.records_import(*ctx.records())
    else:
        ctx.records_import(rec, pool)
    assert ctx.rec_words == rw
    runs = 0
    for flags in (routes_of(rw) if routes is None else routes):
        facts = sc.facts(case.name, kh, kl, bool(flags & 4))
        ctx.debug_flags(flags)
        for again in range(2 if flags == 0 else 1):               # (a second score() of the same records: the same bits)
            if rw == 16:
                ctx.profile_reset()
            ctx.score(True)
            _check_scores(case, window, flags, ctx.scores(), want_rows, facts)
            if rw == 16:                                         # (also after group(): 64-byte records get their whole profile from score())
                got_ca, got_cu, _ = ctx.profile()
                assert np.array_equal(got_cu, cu), _where(case, window, flags) + ": countUnique"
                np.testing.assert_allclose(got_ca, ca, rtol=1e-12, atol=0, err_msg=_where(case, window, flags) + ": countAll")
            _check_route(case, window, flags, ctx, facts)
            runs += 1
        if flags == 0 and case.family == "rows":
            ctx.row_merge_blocks(1)
            ctx.score(True)
            _check_scores(case, window, flags, ctx.scores(), want_rows, facts)
            ctx.row_merge_blocks(0)
            runs += 1
    ctx.debug_flags(0)
    ctx.close()
    return runs


@pytest.mark.parametrize("name", sc.case_names())
def test_scores(devices, name):
    """per window and route: the score rows as bits (for 64-byte records the profile too), the route taken"""
    case = sc.case(name)
    t0 = time.perf_counter()
    runs = sum(_run_window(devices, case, window) for window in case.windows)
    print("\nscore corpus %s: %d queries, %d reads, %d runs (windows x routes), %.2f s" % (name, case.n, case.n_reads, runs, time.perf_counter() - t0))


@pytest.mark.parametrize("name", [sc.case_names(f)[0] for f in FAMILIES])
def test_through_the_group_stage(devices, name):
    """the family's first case through kasa_batch_group in place of the import, the product route, every window"""
    case = sc.case(name)
    for window in case.windows:
        _run_window(devices, case, window, group=True, routes=[0])
