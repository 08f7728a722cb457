"""The corpus of hand-made indices and query batches for the group stage (tests/group_corpus.py) is what it claims to be -- one
assertion per category, computed from the reference, so that an edit of the corpus or of a kernel constant cannot silently
move a case off its edge --, its decoder reads what its encoder writes, and its plain reference, replayed event by event, is
the sequential oracle: score bits, countUnique, countAll.  No device here: tests/test_gpu_group_corpus.py feeds the same
cases to kasa_batch_group."""
import os
import re

import numpy as np
import pytest

from oracle import oracle
from tests import group_corpus as gc, lookup_corpus as lc
from tests.group_corpus import replay as _replay

KS = (12, 25)
SMALL = gc.case_names(large=False)
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kasa_amd", "csrc", "kasa_hip.hip")


def _primary(name):
    c = gc.case(name)
    return c, gc.ref(name, *c.windows[0])


def _names(family, K=None):
    return [n for n in gc.case_names(large=False) if gc.case(n).family == family and (K is None or gc.case(n).letters == K)]


def _group_entries(r):
    return range(r.rep - r.walk[0], r.rep + r.walk[1] + 1)


# ---- the constants ------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    """every restated constant, found by its name in kasa_hip.hip"""
    src = open(HIP).read()

    def const(name):
        m = re.search(r"static constexpr (?:int|uint32_t) (?:\w+ = \w+, )*%s = ([^,;]+)[,;]" % name, src)
        assert m, name
        v = m.group(1).strip().rstrip("u")
        return eval(re.sub(r"(\d+)u", r"\1", v), {"TILE": gc.TILE})

    for name in ("TILE", "RANGE_LETTERS", "G2_STEPS", "LONG_STEPS", "LONG_STEPS_CROWDED", "G2_OVF", "GOVF", "G2_SPAN", "GSPAN", "GMARGIN", "POOL_SIZES",
                 "REC_SPLIT", "REC_SAT"):
        assert const(name) == getattr(gc, name), name
    assert const("GITEMS") * 64 == gc.WAVE
    for rw in (8, 16):
        m = re.search(r"struct RecTraits<%d> \{ static constexpr int LEVELS = (\d+), INL = (\d+), SEG0 = (\d+), OBITS = (\d+); \};" % rw, src)
        assert m and (int(m.group(2)), int(m.group(3)), int(m.group(4))) == (gc.INL[rw], gc.SEG0[rw], gc.OBITS[rw]), rw
    assert "constexpr int OVF = (PACK6 ? G2_OVF : G2_OVF / 2) * PARKX;" in src and "constexpr bool PACK6 = NL <= 6;" in src
    assert re.search(r"group2_kernel<uint64_t, 6, 0, 4><<<", src), "the second launch: four times the park buffer"
    assert "for (uint32_t a0 = 1;; a0 += %d)" % gc.COOP_CHUNK in src and "for (uint32_t b0 = 1;; b0 += %d)" % gc.COOP_CHUNK in src
    assert "n == 255u ? pool[w[7]] : n" in src and "(cl < 7u ? cl : 7u)" in src


# ---- decoder and encoder ------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.case_names())
def test_decode_reads_what_encode_writes(name):
    """decode(encode(reference)) is the reference, for every window; pool blocks lie behind word 0, one behind the other, and
    only lists longer than INL have one"""
    c = gc.case(name)
    for kh, kl in c.windows:
        recs, rw = gc.ref(name, kh, kl), gc.rec_words(kh, kl)
        rec, pool = gc.encode(recs, rw, kh, kl)
        assert rec.shape == (c.n, rw)
        lead = gc.leaders(recs)
        rows = [p for p in range(c.n) if lead[p] or p < 2 * gc.TILE or len(recs[p].segs) <= gc.INL[rw]]      # (of a long run of one long list: two tiles and the leaders)
        got = gc.decode(rec, pool, rw, kh, kl, rows)
        at = None
        for g, r in zip(got, (recs[p] for p in rows)):
            assert g.fields(rw == 16) == r.fields(rw == 16), (name, kh, kl, r.p)
            assert (g.block is not None) == (len(r.segs) > gc.INL[rw]), (name, kh, kl, r.p)
            if g.block:
                assert g.block[0] >= (at or 1) and g.block_nseg == len(r.segs)
                at = g.block[1]
        assert (at or 1) <= pool.shape[0]


# ---- the reference against the sequential oracle ------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_reference_is_the_sequential_oracle(name):
    c = gc.case(name)
    iv = oracle.IndexView(c.ix)
    qs, rd = c.sorted
    for kh, kl in c.windows:
        p = oracle.params(kh, kl, 3, K=c.letters)
        a, b = oracle.ranges(iv, p, qs)
        res = oracle.compare(iv, p, qs, rd, a, b, c.n_reads, True, closed_form=False)
        M, ca, cu = _replay(c, gc.ref(name, kh, kl), kh, kl)
        assert np.array_equal(M.view(np.uint32), res.M.view(np.uint32)), (name, kh, kl, "score bits", int(np.flatnonzero((M != res.M).any(axis=1))[0]))
        assert np.array_equal(cu, res.count_unique), (name, kh, kl, "countUnique")
        np.testing.assert_allclose(ca, res.count_all, rtol=1e-12, atol=0, err_msg="%s k %d..%d countAll" % (name, kh, kl))


# ---- walk ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_walk_lengths_sides_and_places(K):
    """Per tile three leaders -- positions 0 and 1 (one wavefront) and 1021 (the tile's last wavefront) -- whose lists visit the
    tile's N entries beyond the representative, on the side(s) the case names; every N of WALK_N; the representative at entry 0
    and at the last entry; 63, 64 and 65 entries on one side (a chunk of coop_walk less one, whole, and one more)."""
    for mode in gc.WALK_MODES:
        c, recs = _primary("walk%d %s" % (gc._w(K), mode))
        assert sorted(c.claim["walks"]) == gc.WALK_N
        for t, n in enumerate(c.claim["walks"]):
            for at in (0, 1, gc.TILE - 3):
                r = recs[t * gc.TILE + at]
                assert r.d == c.windows[0][0] and sum(r.walk) == n == len(r.segs) - 1, (c.name, t, at, r.walk)
                assert {"left": r.walk[1] == 0, "right": r.walk[0] == 0, "both": r.walk == (n // 2, n - n // 2)}[mode], (c.name, t, r.walk)
            assert sum(1 for r in recs[t * gc.TILE:(t + 1) * gc.TILE] if r.d) == 3
        if mode == "right":
            assert recs[0].rep == 0 and recs[0].walk == (0, 200)
        if mode == "left":
            last = [r for r in recs if r.d][-1]
            assert last.rep == c.ix.n - 1 and last.walk == (200, 0)
    facts = gc.tile_facts(recs, c.ix.n)
    assert sorted(f["walk"] for f in facts[:len(gc.WALK_N)]) == gc.WALK_N


@pytest.mark.parametrize("K", KS)
def test_walk_over_the_whole_index(K):
    seen = set()
    for nl, nr in gc.WALK_WHOLE:
        c, recs = _primary("walk%d whole %d+%d" % (gc._w(K), nl, nr))
        r = [x for x in recs if x.d][0]
        assert r.walk == (nl, nr) and r.rep - nl == 0 and r.rep + nr == c.ix.n - 1, (c.name, r.walk, r.rep)
        seen.add(r.walk)
    assert {(64, 64), (63, 66), (65, 63), (0, 129), (129, 0)} <= seen


# ---- count --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_count_lists_levels_and_inline_edges(K):
    w = gc._w(K)
    c, recs = _primary("count%d lists" % w)
    assert {len(r.segs) for r in recs if r.d} == set(gc.COUNT_LISTS)
    assert not c.never_coop
    for kh, kl in gc.WINDOWS[K]:
        if gc.rec_words(kh, kl) == 8 and kh - kl >= 2 and kl <= 7:
            recs = gc.ref("count%d level" % w, kh, kl)
            tops = {r.sizes[-1] for r in recs if r.d == kh and set(r.sizes[:kh - max(kl, 7)]) == {1} and r.walk[0]}
            assert tops >= set(gc.COUNT_LEVEL), (kh, kl, tops)
    c, recs = _primary("count%d inl" % w)
    assert {len(r.segs) for r in recs if r.d} == {gc.INL[8], gc.INL[8] + 1, gc.INL[16], gc.INL[16] + 1}


# ---- split --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_split_every_dup_and_entries_without_segment(K):
    name = "split%d" % gc._w(K)
    c = gc.case(name)
    idx, tax = lc.key_ints(c.ix.kmer), c.ix.tax.tolist()
    dup = gc.dup_letters(idx, tax, K)
    assert any(idx[i] == idx[i + 1] and tax[i] != tax[i + 1] for i in range(len(idx) - 1)), "equal keys, different taxa"
    for kh, kl in c.windows:
        recs = gc.ref(name, kh, kl)
        seen, no_segment, rep_none, twice = set(), 0, 0, 0
        for r in recs:
            if not r.d:
                continue
            for i in _group_entries(r):
                seen |= {what for what, v in (("5", 5), ("6", 6), ("kLow - 1", kl - 1), ("kLow", kl), ("d - 1", r.d - 1), ("d", r.d)) if dup[i] == v}
            no_segment += len(r.segs) < sum(r.walk) + 1
            rep_none += dup[r.rep] >= gc.RANGE_LETTERS and dup[r.rep] + 1 > r.d
            taxa = [t for t, _, _ in r.segs]
            twice += len(taxa) > len(set(taxa))
            assert r.split == any(kf > kl for _, kf, _ in r.segs)
        want = {"5", "6", "d - 1"} | ({"d"} if kh < K else set()) | ({"kLow - 1", "kLow"} if kl > 6 and kl < K else set())      # (dup < K: a k-mer is in the index once per taxon)
        assert seen >= want, (name, kh, kl, seen)
        assert no_segment or kl == K, (name, kh, kl)           # (kLow = K: the group is one key)
        assert twice or kh == kl, (name, kh, kl)               # (one level: a taxon is in it once)
        assert rep_none or kh == K, (name, kh, kl, "a representative whose dup is its depth needs a depth the window cuts")


# ---- order --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_order_ties_and_event_counts(K):
    name = "order%d" % gc._w(K)
    c = gc.case(name)
    idx = lc.key_ints(c.ix.kmer)
    qs = lc.key_ints(c.sorted[0])
    events = set()
    for kh, kl in c.windows:
        recs = gc.ref(name, kh, kl)
        up = down = ties = both_sides = 0
        for r in recs:
            if not r.d:
                continue
            events.add((gc.rec_words(kh, kl), len(r.order)))
            steps = [b - a for a, b in zip(r.F, r.F[1:])]
            up += any(s > 0 for s in steps)
            down += any(s < 0 for s in steps)
            ties += any(s == 0 for s in steps) and r.order != tuple(sorted(r.order, reverse=True))
            if r.walk[0] >= 2 and r.walk[1] >= 2:
                sh = [min(r.d, gc.shared_letters(qs[r.p], idx[r.rep + o], K)) for o in (-2, -1, 1, 2)]
                both_sides += len(set(sh)) == 1
        if kh > kl:
            assert up and down and ties, (name, kh, kl, up, down, ties)
            assert both_sides, (name, kh, kl)
    assert {12: {(8, 8), (16, 10)}, 25: {(16, 19), (16, 8)}}[K] <= events, events


# ---- flush --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_flush_places(K):
    """the leader at the first position of every place is matched to kHigh, and the groups of its levels above 6 close at the
    second position: one query on in its lane pair, in a later lane, in the next wavefront, the next tile, nowhere"""
    c, recs = _primary("flush%d" % gc._w(K))
    kh, kl = c.windows[0]
    for place, (p, closer) in c.claim["places"].items():
        r = recs[p]
        assert r.d == kh and set(r.F[max(kl, 7) - kl:]) == {c.n if closer is None else closer}, (place, r.F)
    P = c.claim["places"]
    assert P["lane pair"][0] // 2 == P["lane pair"][1] // 2 and P["later lane"][0] // gc.WAVE == P["later lane"][1] // gc.WAVE
    assert P["next wavefront"] == (gc.WAVE - 1, gc.WAVE) and P["next tile"] == (gc.TILE - 1, gc.TILE)
    assert P["tile behind"][1] // gc.TILE - P["tile behind"][0] // gc.TILE >= 2


# ---- followers, hits ----------------------------------------------------------------------------
def _runs(recs):
    """(start, length, rep, d) of every maximal run of matched queries with one (representative, depth)"""
    out, p = [], 0
    while p < len(recs):
        e = p + 1
        if recs[p].d:
            while e < len(recs) and (recs[e].rep, recs[e].d) == (recs[p].rep, recs[p].d):
                e += 1
            out.append((p, e - p, recs[p].rep, recs[p].d))
        p = e
    return out


@pytest.mark.parametrize("K", KS)
def test_follower_runs(K):
    seen, cut = set(), 0
    for phase in (0, 1):
        c, recs = _primary("followers%d phase %d" % (gc._w(K), phase))
        rw = gc.rec_words(*c.windows[0])
        runs = _runs(recs)
        for (p, n, rep, d), nxt in zip(runs, runs[1:] + [None]):
            if len(recs[p].segs) > gc.INL[rw]:
                seen.add((n, p % 2))
            cut += nxt is not None and nxt[0] == p + n and nxt[2] == rep and nxt[3] != d
        long = [r for r in runs if r[1] == 1025][0]
        assert long[0] // gc.TILE != (long[0] + 1024) // gc.TILE
    assert seen >= {(n, par) for n in gc.FOLLOWER_RUNS for par in (0, 1)}, seen
    assert cut >= 4, "the same representative at a depth cut by a '^'"


def test_hit_groups():
    for K in KS:
        c, recs = _primary("hits%d phase 0" % gc._w(K))
        assert {n for _, n, _, _ in _runs(recs)} >= set(gc.HIT_GROUPS)
    c, recs = _primary(gc.LARGE)
    assert max(n for _, n, _, _ in _runs(recs)) == gc.HITS_LARGE > 0xFFFF and c.large


# ---- span, park, pool ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_spans(K):
    """the tile's span with its margins is what the case names; the lists at its two ends are as long as named, on the outer
    sides; only the case built for it walks out of group2_kernel's staged window"""
    outside = {}
    for limit, delta, walk in gc.SPANS:
        c, recs = _primary("span%d %d%+d walk %d" % (gc._w(K), limit, delta, walk))
        f = gc.tile_facts(recs, c.ix.n)[0]
        m = [r for r in recs if r.d]
        assert f["span"] == limit + delta and m[0].walk == (walk, 0) and m[-1].walk == (0, walk), (c.name, f, m[0].walk, m[-1].walk)
        assert m[0].rep - walk >= gc.GMARGIN and m[-1].rep + walk + gc.GMARGIN < c.ix.n
        outside[(limit, delta, walk)] = f["outside"]
    assert outside[(gc.G2_SPAN, 60, 40)] and not outside[(gc.G2_SPAN, 50, 40)] and not outside[(gc.G2_SPAN, 1, 8)]


@pytest.mark.parametrize("K", KS)
def test_parked_totals_and_the_routes_they_take(K):
    w = gc._w(K)
    for total in gc.PARK_EDGES:
        c, recs = _primary("park%d g2 %d" % (w, total))
        facts = gc.tile_facts(recs, c.ix.n)
        assert facts[0]["parked2"] == total and facts[0]["walk"] == gc.G2_STEPS and not facts[0]["outside"], (c.name, facts[0])
        assert len(facts) >= 5 and all(f["leaders"] == 0 for f in facts[1:])
        listed = gc.listed_tiles(facts, 6, K == 25)
        ovf = gc.g2_ovf(6, K == 25)
        assert listed == (int(total > ovf), int(total > (4 * ovf if K == 12 else ovf))), (c.name, listed)
        if K == 12:
            facts5 = gc.tile_facts(gc.ref(c.name, 12, 5), c.ix.n)
            assert facts5[0]["parked2"] == total and gc.listed_tiles(facts5, 8, False) == (int(total > 512),) * 2
    for total in gc.PARK_EDGES[:3]:
        c, recs = _primary("park%d g %d" % (w, total))
        f = gc.tile_facts(recs, c.ix.n)[0]
        assert f["parked"] == total and f["walk"] == gc.G2_STEPS, (c.name, f)


@pytest.mark.parametrize("K", KS)
def test_walks_listed_from_41_entries_on(K):
    c = gc.case("walk%d both" % gc._w(K))
    kh, kl = (12, 7)
    facts = gc.tile_facts(gc.ref(c.name, kh, kl), c.ix.n)
    assert gc.listed_tiles(facts, 6, K == 25)[0] == sum(1 for n in gc.WALK_N if n > gc.G2_STEPS) == 11
    assert [f["walk"] > gc.G2_STEPS for f in facts[:21]] == [n > 40 for n in sorted(gc.WALK_N)]


@pytest.mark.parametrize("K", KS)
def test_pool_outgrows_its_first_size(K):
    c, recs = _primary("pool%d" % gc._w(K))
    rw = gc.rec_words(*c.windows[0])
    lead = gc.leaders(recs)
    words = sum(len(r.segs) - (gc.INL[rw] - 1) + 1 for r, l in zip(recs, lead) if l)
    assert sum(lead) == gc.POOL_LEADERS and c.n < 65536 < words, (sum(lead), c.n, words)
    assert {len(r.segs) for r in recs} == {gc.POOL_LIST}


# ---- ends ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_ends(K):
    cases = [gc.case(n) for n in _names("ends", K)]
    assert {c.n for c in cases} >= {1, 2, 127, 128, 129, 1023, 1024, 1025, 2049}
    assert {c.ix.n for c in cases} >= {1, 2, 3}
    c, recs = _primary("ends%d nothing matches" % gc._w(K))
    assert c.n > gc.TILE and not any(r.d for r in recs)
