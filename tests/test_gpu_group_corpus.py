"""The group stage (kasa_batch_group: group2_kernel, its second launch, group_kernel with walk_segments and coop_walk, the pool's
retry loop) on the hand-made corpus of tests/group_corpus.py, against that file's plain reference: per sorted query the event
record kasa_batch_records_fetch returns -- depth everywhere; position, Fmax, event order, segment count, the ordered
segments, the 3-bit level sizes, both flags and the exact sizes of every matched query -- under every route of group_stage
the record width has (ROUTES), with the route a case was built for read back from batch_stats().  Then the profile made by
the group stage and, after the records went back in through kasa_batch_records_import, the per-read scores as bits against
the sequential oracle.  tests/test_group_corpus_cpu.py shows that the corpus holds every category it is meant to and that
the reference is the oracle.

One deviation from "the flags equal the reference" is the kernel's documented own: group_kernel's cooperative form marks
every list it walked by wavefront REC_SAT ("a long list always carries its exact sizes"), whether or not a level reaches 7.
Such a record -- more than INL segments, more than LONG_STEPS_CROWDED entries walked -- must then carry the right exact sizes.

Not compared: the 3-bit and 16-bit size fields of levels the window does not have (lv >= kHigh - kLow + 1).  group_kernel leaves
them zero; group2_kernel's general form (any level count but six, 128-bit keys) leaves the size of the shallowest level there.
No reader looks at them.

Kept out: the profile-key capacity retry (more than 2^20 keys of one batch) and pools near 2^32 words need batches far beyond
a few seconds.

MEASURED (MI355X, pytest --durations=0): the file's 125 tests in 25.2 s, 23.9 s of it in the tests' calls.  The slowest: a pool case
(38 400 queries, 300 pool blocks of 250 segments; a test per route) 0.17 s under the flags that lead with group_kernel, 1.3 s
without followers (38 400 blocks), 1.6 to 1.9 s on the product route and with --coverage (the pool's retry; the oracle's scores of
38 400 reads); a walk case (21 507 queries, 18 to 28 runs of windows x routes) 0.75 to 1.35 s; order128 0.55 s; the batch of
70 001 queries 0.45 s; everything else below 0.5 s.
Tiles group2_kernel listed / listed again, summed over the windows with narrow records, flags 0 (every other route: 0 / 0):
  family      runs   listed  again      family      runs   listed  again
  walk         294    213     213       span         286     27      27
  count        110     24      24       park         180     24      21
  split         46      1       1       pool           8      0       0   (38 of 38 listed, then the batch again on group_kernel)
  order         46      6       6       ends          98      0       0
  flush         46      0       0       lookup main   74     19      19
  followers     92      0       0       lookup open   10      0       0
  hits          51      0       0
A walk case lists the 11 tiles of 41 and more entries of its 21, under every window but the one-level one; park 1025 is 1 / 0,
park 4097 1 / 1, park 513 1 / 1 under eight levels and under 128-bit keys; span 1792 + 60 with walks of 40 is 1 / 1, + 50 is 0 / 0.
"""
import functools
import time

import numpy as np
import pytest

from kasa_amd import capi
from oracle import oracle
from tests import group_corpus as gc, helpers
from tests.test_gpu_parity import assert_csr_equal, csr_rows

pytestmark = pytest.mark.gpu

ROUTES = {0: "the product route", 16777216: "group_kernel alone", 262144: "COOP from the first batch", 131072: "never COOP", 2048: "no followers",
          4096: "no staged span"}
COVERAGE_FAMILIES = ("split", "hits", "pool")


def routes_of(case, rw):
    if rw == 16:
        return [0, 2048, 4096]
    return [0, 16777216, 262144] + ([131072] if case.never_coop else []) + [2048]


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
    assert capi.device_count() > 0, "no HIP device visible: the group corpus needs a real MI355X"
    d = _Devices()
    yield d
    d.close()


@functools.lru_cache(maxsize=8)
def _expected(name, window):
    """the reference, its encoding, and what the comparison needs of it as arrays -- once per case and window"""
    kh, kl = window
    recs, rw = gc.ref(name, kh, kl), gc.rec_words(kh, kl)
    rec, pool = gc.encode(recs, rw, kh, kl)
    d = np.array([r.d for r in recs], dtype=np.uint32)
    nseg = np.array([len(r.segs) for r in recs], dtype=np.int64)
    off = rec[:, gc.SEG0[rw] + gc.INL[rw] - 1].astype(np.int64)
    lead = np.array(gc.leaders(recs), dtype=bool)
    return recs, rw, rec, pool, d, nseg, off, lead


@functools.lru_cache(maxsize=4)
def _oracle(name, window, coverage=False):
    case = gc.case(name)
    p = oracle.params(window[0], window[1], 3, K=case.letters, coverage=coverage)
    iv = oracle.IndexView(case.ix)
    qs, rd = case.sorted
    a, b = oracle.ranges(iv, p, qs)
    per_read = not case.large and not coverage
    res = oracle.compare(iv, p, qs, rd, a, b, case.n_reads, per_read, closed_form=False)
    return res, (helpers.csr_from_dense(res.M) if per_read else None)


def _where(case, window, flags, p):
    return "%s, k %d..%d, flags %d (%s): sorted position %d (tile %d, wavefront %d, lane %d, item %d)" % (
        case.name, window[0], window[1], flags, ROUTES[flags], p, p // gc.TILE, p % gc.TILE // gc.WAVE, p % gc.WAVE // 2, p % 2)


def _fail_at(case, window, flags, p, got, want, wide, skip=()):
    g, w = got.fields(wide), want.fields(wide)
    for f in w:
        if f not in skip and g.get(f) != w[f]:
            if isinstance(w[f], tuple) and isinstance(g.get(f), tuple) and len(w[f]) == len(g[f]) > 8:
                i = [a != b for a, b in zip(g[f], w[f])].index(True)
                pytest.fail("%s: %s[%d] is %r, reference %r (the list visits %d + %d entries around entry %d)" % (_where(case, window, flags, p), f, i, g[f][i], w[f][i], want.walk[0], want.walk[1], want.rep))
            pytest.fail("%s: %s is %r, reference %r (the list visits %d + %d entries around entry %d)" % (_where(case, window, flags, p), f, g.get(f), w[f], want.walk[0], want.walk[1], want.rep))
    return None


def _compare(case, window, flags, rec, pool):
    """every record against the reference; -> the pool blocks {offset: (end, representative, depth)}"""
    kh, kl = window
    recs, rw, exp, exp_pool, d, nseg, exp_off, lead = _expected(case.name, window)
    wide, inl, seg0 = rw == 16, gc.INL[rw], gc.SEG0[rw]
    assert rec.shape == exp.shape, (case.name, window, flags, rec.shape)
    bad = np.flatnonzero((rec[:, 2] & 31) != d)
    if bad.shape[0]:
        p = int(bad[0])
        pytest.fail("%s: d is %d, reference %d (%d positions differ)" % (_where(case, window, flags, p), int(rec[p, 2] & 31), int(d[p]), bad.shape[0]))
    matched, is_list = d > 0, nseg > inl
    if not wide:                                        # (the size fields of levels the window does not have: see the docstring)
        rec = rec.copy()
        rec[:, 3] &= np.uint32(0xFF | (((1 << (3 * (kh - kl + 1))) - 1) << 8))
    # records without a pool block: word for word what the encoder makes of the reference
    rows = np.flatnonzero(matched & ~is_list & (rec != exp).any(axis=1))
    if rows.shape[0]:
        p = int(rows[0])
        _fail_at(case, window, flags, p, gc.decode_one(rec[p].tolist(), pool, rw, kh, kl), recs[p], wide)
        pytest.fail("%s: the record's words %s, the reference's %s" % (_where(case, window, flags, p), rec[p].tolist(), exp[p].tolist()))
    # lists: the words before the pool offset (REC_SAT: see the docstring), then the block
    head = rec[:, :seg0 + inl - 1].copy()
    want_head = exp[:, :seg0 + inl - 1].copy()
    if not wide:
        head[:, 2] &= ~np.uint32(gc.REC_SAT)
        want_head[:, 2] &= ~np.uint32(gc.REC_SAT)
    head_bad = (head != want_head).any(axis=1)
    blocks, done = {}, set()
    n_pool = int(pool.shape[0])
    for p in np.flatnonzero(is_list).tolist():
        w, r = rec[p], recs[p]
        off, sat, want_sat = int(w[seg0 + inl - 1]), bool(w[2] & gc.REC_SAT) and not wide, r.sat
        if not head_bad[p] and (off, sat, id(r.segs)) in done:           # (this very block against this very list: a query before has done it)
            continue
        n_words = len(r.segs) - (inl - 1) + 1 + (gc.POOL_SIZES if sat else 0)
        ok = not head_bad[p] and 1 <= off and off + n_words <= n_pool
        if ok and sat == want_sat:
            eo, skip = int(exp_off[p]), (gc.POOL_SIZES if sat else 0)
            ok = int(pool[off]) == len(r.segs) and np.array_equal(pool[off + 1 + skip:off + n_words], exp_pool[eo + 1 + skip:eo + n_words])
            if ok and sat:
                ok = gc.decode_one(w.tolist(), pool, rw, kh, kl).sizes == r.sizes
        elif ok:
            g = gc.decode_one(w.tolist(), pool, rw, kh, kl)
            allowed = sat and sum(r.walk) > gc.LONG_STEPS_CROWDED
            ok = allowed and g.sizes == r.sizes and g.block_nseg == len(r.segs) and _fail_at(case, window, flags, p, g, r, wide, skip=("REC_SAT",)) is None
        if not ok:
            if not (1 <= off and off + n_words <= n_pool):
                pytest.fail("%s: the pool block [%d, %d) is not inside [1, %d)" % (_where(case, window, flags, p), off, off + n_words, n_pool))
            g = gc.decode_one(w.tolist(), pool, rw, kh, kl)
            _fail_at(case, window, flags, p, g, r, wide)
            pytest.fail("%s: the pool block's first word is %r for %d segments (REC_SAT %r, reference %r)" % (_where(case, window, flags, p), g.block_nseg, len(r.segs), sat, want_sat))
        done.add((off, sat, id(r.segs)))
        seen = blocks.setdefault(off, (off + n_words, r.rep, r.d))
        assert seen == (off + n_words, r.rep, r.d), "%s: its pool block at %d is also that of a list of representative %d, depth %d" % (_where(case, window, flags, p), off, seen[1], seen[2])
    ends = sorted((o, e) for o, (e, _, _) in blocks.items())
    for (o0, e0), (o1, _) in zip(ends, ends[1:]):
        assert e0 <= o1, "%s, k %d..%d, flags %d: the pool blocks [%d, %d) and [%d, ...) overlap" % (case.name, kh, kl, flags, o0, e0, o1)
    # a follower's words are its leader's: word 2 less the order, word 3, the segment words (with the pool offset)
    if flags != 2048:
        fol = np.flatnonzero(matched & ~lead)
        mask2 = np.uint32(31 | gc.REC_SPLIT | (0 if wide else gc.REC_SAT))
        cols = [3] + list(range(seg0, rw))
        same = ((rec[fol, 2] & mask2) == (rec[fol - 1, 2] & mask2)) & (rec[fol][:, cols] == rec[fol - 1][:, cols]).all(axis=1)
        if not same.all():
            p = int(fol[np.flatnonzero(~same)[0]])
            pytest.fail("%s: a follower's words %s are not its leader's %s" % (_where(case, window, flags, p), rec[p].tolist(), rec[p - 1].tolist()))
    return blocks


def _run(devices, case, window, flags, coverage=False):
    ctx = capi.Context(devices.index(case), window[0], window[1], 3)
    ctx.debug_flags(flags)
    ctx.set_queries(case.q, case.payload, case.n_reads)
    ctx.sort_and_range()
    ctx.group(coverage=coverage)
    return ctx


def _check_route(case, window, flags, st, rw, pool_words):
    kh, kl = window
    n_tiles = (case.n + gc.TILE - 1) // gc.TILE
    want = (0, 0)
    if rw == 8 and flags == 0:
        want = gc.listed_tiles(gc.tile_facts(gc.ref(case.name, kh, kl), case.ix.n), kh - kl + 1, case.wide)
        if 4 * want[0] > n_tiles and pool_words > max(65536, case.n):
            want = (0, 0)      # (more than a quarter of the tiles listed: the context turns to group_kernel; the pool outgrown: the batch again, there)
    got = (st["group_tiles_listed"], st["group_tiles_listed_again"])
    assert st["group_tiles"] == n_tiles and got == want, "%s, k %d..%d, flags %d (%s): group2_kernel listed %d of %d tiles and its second launch %d, the case is built for %d and %d" % (
        case.name, kh, kl, flags, ROUTES[flags], got[0], st["group_tiles"], got[1], want[0], want[1])
    return got


def _params():
    """a test per case; the pool cases (38 400 lists of 250 segments a run) a test per route"""
    out = []
    for n in gc.case_names():
        c = gc.case(n)
        out += [(n, f) for f in routes_of(c, gc.rec_words(*c.windows[0]))] if c.family == "pool" else [(n, None)]
    return out


@pytest.mark.parametrize("name,only", _params(), ids=["%s%s" % (n, "" if f is None else " flags %d" % f) for n, f in _params()])
def test_records(devices, name, only):
    """Per window and route: the records, the pool conditions, the followers, the route taken; for narrow records the profile
    straight after the group stage; for the cases with score windows, and for all wide records, the scores."""
    case = gc.case(name)
    t0 = time.perf_counter()
    runs, listed = 0, {}
    for window in case.windows:
        rw = gc.rec_words(*window)
        for flags in (routes_of(case, rw) if only is None else [only]):
            if rw == 8 and case.wide and max(len(r.segs) for r in gc.ref(name, *window)) >= gc.NSEG_CAP:
                # 128-bit keys have no cooperative kernel: a list of 255 or more segments under narrow records is refused, on every route
                with pytest.raises(RuntimeError, match="255 or more taxa of a 128-bit index"):
                    _run(devices, case, window, flags)
                continue
            ctx = _run(devices, case, window, flags)
            rec, pool = ctx.records()
            st = ctx.batch_stats()
            assert ctx.rec_words == rw
            blocks = _compare(case, window, flags, rec, pool)
            got = _check_route(case, window, flags, st, rw, pool.shape[0])
            if flags == 0 and rw == 8:
                listed[window] = got
            if case.family == "pool":
                assert pool.shape[0] > 65536 > case.n, (name, window, flags, pool.shape[0])
            res, rows = _oracle(name, window)
            if rw == 8:
                ca, cu, _ = ctx.profile()
                assert np.array_equal(cu, res.count_unique), "%s, k %d..%d, flags %d: countUnique" % (name, window[0], window[1], flags)
                np.testing.assert_allclose(ca, res.count_all, rtol=1e-12, atol=0, err_msg="%s, k %d..%d, flags %d: countAll" % (name, window[0], window[1], flags))
            if not case.large and (rw == 16 or window in case.score_windows):
                ctx.records_import(rec, pool)
                ctx.score(True)
                if rw == 16:
                    ca, cu, _ = ctx.profile()
                    assert np.array_equal(cu, res.count_unique), "%s, k %d..%d, flags %d: countUnique" % (name, window[0], window[1], flags)
                    np.testing.assert_allclose(ca, res.count_all, rtol=1e-12, atol=0, err_msg="%s, k %d..%d, flags %d: countAll" % (name, window[0], window[1], flags))
                assert_csr_equal(csr_rows(*ctx.scores()), rows)
            ctx.close()
            runs += 1
            del blocks
    print("\ngroup corpus %s: %d queries, %d runs (windows x routes), tiles listed / listed again on the product route %s, %.2f s"
          % (name, case.n, runs, {"%d..%d" % w: v for w, v in listed.items()}, time.perf_counter() - t0))


@pytest.mark.parametrize("name", [n for n in gc.case_names() if gc.case(n).family in COVERAGE_FAMILIES])
def test_coverage_counts_once(devices, name):
    """group(coverage=True): countTotal against the oracle with coverage -- once per matched group, also where the pool's retry
    runs the kernel a second time"""
    case = gc.case(name)
    window = case.windows[0]
    res, _ = _oracle(name, window, True)
    ctx = _run(devices, case, window, 0, coverage=True)
    rec, pool = ctx.records()
    _compare(case, window, 0, rec, pool)
    _, cu, ct = ctx.profile()
    ctx.close()
    assert np.array_equal(ct, res.count_total), "%s, k %d..%d: countTotal" % (name, window[0], window[1])
    if gc.rec_words(*window) == 8:
        assert np.array_equal(cu, res.count_unique)
