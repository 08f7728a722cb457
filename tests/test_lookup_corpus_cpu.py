"""The corpus of hand-made indices and query batches for the lookup stage (tests/lookup_corpus.py) is what it claims to be --
one assertion per category, so that an edit of the corpus cannot silently drop one -- and its plain reference agrees with the
oracle.  No device here: tests/test_gpu_lookup_corpus.py feeds the same cases to kasa_batch_sort_and_range."""
import time

import numpy as np
import pytest

from oracle import oracle
from tests import lookup_corpus as lc

SMALL = lc.case_names(large=False)
KS = (12, 25)


def _cases(family=None, K=None, large=False):
    return [c for c in map(lc.case, lc.case_names(large=large)) if (family is None or c.family == family) and (K is None or c.letters == K)]


def _ref(c, window=None):
    kh, kl = window or c.windows[0]
    return lc.reference(c.name, kh, kl)


def _uncut(c):
    """the reference under the window that cuts nothing: depth = L wherever L >= 6 and no '^' ends the query"""
    return lc.reference(c.name, c.letters, 1)


# ---- span -------------------------------------------------------------------------------------
def test_span_edge_every_span_and_parity():
    """A tile whose span is exactly 1535, 1536, 1537 and 1538 records: 64-bit keys with the span's start even and odd,
    128-bit keys (whose staging has no shift) once each; as designed, tile by tile."""
    for K in KS:
        seen = set()
        for c in _cases("span", K):
            assert [int(s) for s in c.spans[:, 0]] == [s for s, _ in c.runs], c.name
            if K == 12:
                assert [int(p) for p in c.spans[:, 1]] == [p for _, p in c.runs], c.name
            seen |= {(int(s), int(p) if K == 12 else 0) for s, p in c.spans[:, :2]}
        assert seen >= {(s, p) for s in lc.SPAN_EDGE for p in ((0, 1) if K == 12 else (0,))}, (K, seen)


def test_span_edge_queries_stay_in_one_bucket():
    """... with the run inside one prefix-table bucket and all the tile's queries inside that bucket"""
    for c in _cases("span"):
        bits, tb = 5 * c.letters, lc.table_bits(c.ix.n)
        qb = lc.formats.key_shr(c.sorted[0], bits - tb)
        for t in range(c.spans.shape[0]):
            assert np.unique(qb[t * lc.TILE:(t + 1) * lc.TILE]).shape[0] == 1, (c.name, t)


def test_span_edge_last_record_of_odd_and_even_index():
    """A staged span that reaches the last record of an index of odd size (the staging loop's branch for the single last record)
    and of even size."""
    seen = {(c.ix.n % 2) for c in _cases("span", 12) if c.spans[-1, 2] and c.spans[-1, 0] <= lc.LSPAN}
    assert seen == {0, 1}


def test_tiles_of_both_kinds_in_one_batch():
    """staged tiles, an unstaged tile, staged tiles again"""
    for K in KS:
        n = 0
        for c in _cases(K=K):
            staged = (c.spans[:, 0] <= lc.LSPAN).tolist()
            n += any(staged[t] and not staged[t + 1] and staged[t + 2] for t in range(len(staged) - 2))
        assert n >= 2, K


# ---- index ends ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_index_ends(K):
    """Queries below the first and above the last index key, on the first and on the last; indices of 1, 2 and 3 entries; a
    tile whose first bucket is bucket 0 and one whose last bucket is the top bucket."""
    seen = set()
    top = (1 << (5 * K)) - 1
    for c in _cases("ends", K):
        r, n = _ref(c), c.ix.n
        q = lc.key_ints(c.sorted[0])
        idx = lc.key_ints(c.ix.kmer)
        seen |= {("index of", n)} if n <= 3 else set()
        seen |= {"below"} if (r.lo == 0).any() and q[0] < idx[0] else set()
        seen |= {"above"} if (r.lo == n).any() else set()
        seen |= {"on the first"} if idx[0] in q else set()
        seen |= {"on the last"} if idx[-1] in q else set()
        seen |= {"bucket 0"} if q[0] == 0 and c.spans[0, 3] else set()
        seen |= {"top bucket"} if q[-1] == top and c.spans[-1, 2] else set()
        seen |= {"matched above the last"} if ((r.lo == n) & (r.depth > 0)).any() else set()
        seen |= {"matched below the first"} if ((r.lo == 0) & (r.depth > 0) & (r.la < K)).any() else set()
    want = {("index of", 1), ("index of", 2), ("index of", 3), "below", "above", "on the first", "on the last", "bucket 0", "top bucket",
            "matched above the last", "matched below the first"}
    assert want <= seen, want - seen


def test_batch_sizes():
    """full and partial last tiles, threads with one to four queries"""
    for K in KS:
        assert {c.n for c in _cases("ends", K)} >= set(lc.BATCH_SIZES)


# ---- neighbour geometry ---------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_neighbour_geometry_at_every_length(K):
    """la > lb, la < lb and la == lb at every L -- L == 0 leaves only la == lb (both 0), L == K only la > lb (idx[lo - 1] < q)."""
    c = lc.case("main%d" % (64 if K == 12 else 128))
    r = _uncut(c)
    seen = set(zip(r.L.tolist(), np.sign(r.la - r.lb).tolist()))
    want = {(0, 0), (K, 1)} | {(L, s) for L in range(1, K) for s in (-1, 0, 1)}
    assert want <= seen, sorted(want - seen)


@pytest.mark.parametrize("K", KS)
def test_equal_keys_and_repeated_queries(K):
    """exact matches on a k-mer under 1, 2 and 40 or more taxa (equal keys in a row: the representative is the first of them,
    and the last of them for the query just above); queries 1, 2, 5 and 300 or more times"""
    c = lc.case("main%d" % (64 if K == 12 else 128))
    r = _uncut(c)
    idx = c.ix.kmer
    exact = np.flatnonzero(r.la == K)
    taxa = {int(np.searchsorted(idx, idx[lo], side="right") - lo) for lo in r.lo[exact]} if K == 12 else \
        {lc.key_ints(idx).count(lc.key_ints(idx[lo:lo + 1])[0]) for lo in set(r.lo[exact].tolist())}
    assert {1, 2} <= taxa and max(taxa) >= 40
    above = (r.lb > r.la) & (r.lo > 0)
    prev = np.maximum(r.lo - 2, 0)                                    # the entry before the representative lo - 1 equals it
    assert any(idx[a] == idx[b] for a, b in zip(prev[above], (r.lo - 1)[above]))
    q = c.sorted[0]
    _, counts = np.unique(q, return_counts=True)
    assert {1, 2, 5} <= set(counts.tolist()) and counts.max() >= 300


def test_gallop_steps():
    """In staged tiles, behind the first of a thread's four queries: the lower bound stays (step 0), moves on by one, and by more
    than 64 records."""
    for K in KS:
        seen = set()
        for c in _cases(K=K):
            r = _ref(c)
            p = np.arange(1, c.n)
            ok = (p % lc.ITEMS != 0) & (c.spans[p // lc.TILE, 0] <= lc.LSPAN)
            step = (r.lo[1:] - r.lo[:-1])[ok]
            seen |= {"0"} if (step == 0).any() else set()
            seen |= {"1"} if (step == 1).any() else set()
            seen |= {"far"} if (step > 64).any() else set()
        assert seen == {"0", "1", "far"}, (K, seen)


@pytest.mark.parametrize("K", KS)
def test_thread_and_tile_positions(K):
    """Every kind of query as each of a thread's four (p % 4) -- the main batch comes four times, moved up by 0 .. 3 places -- and
    matched queries of both representatives, and unmatched ones, as a tile's first, second and last query."""
    kinds = {m: set() for m in range(4)}
    edge = {m: set() for m in (0, 1, lc.TILE - 1)}
    for c in _cases(K=K):
        r, u = _ref(c), _uncut(c)
        p = np.arange(c.n)
        hat_cut = (r.depth > 0) & (r.depth < np.minimum(u.L, c.windows[0][0]))
        for m in range(4):
            at = p % 4 == m
            for name, mask in (("la > lb", (r.la > r.lb) & (r.depth > 0)), ("la < lb", (r.la < r.lb) & (r.depth > 0)),
                               ("la == lb", (r.la == r.lb) & (r.depth > 0)), ("exact", r.la == K), ("cut by ^", hat_cut),
                               ("range but no match", (u.L >= lc.RANGE_LETTERS) & (r.depth == 0)), ("no range", u.L < lc.RANGE_LETTERS)):
                if (at & mask).any():
                    kinds[m].add(name)
        for m in edge:
            at = p % lc.TILE == m
            for name, mask in (("rep lo", (r.depth > 0) & (r.la >= r.lb)), ("rep lo - 1", (r.depth > 0) & (r.la < r.lb)), ("unmatched", r.depth == 0)):
                if (at & mask).any():
                    edge[m].add(name)
    first = []                                                          # per phase: where every different query of the main batch comes first
    for phase in range(4):
        q = lc.case("main%d%s" % (64 if K == 12 else 128, " phase %d" % phase if phase else "")).sorted[0]
        keys, at = np.unique(q[phase:], return_index=True)
        first.append((keys, at + phase))
    assert all(np.array_equal(first[0][0], k) for k, _ in first)
    assert (np.sort(np.stack([at % 4 for _, at in first]), axis=0) == np.arange(4)[:, None]).all()     # each of them as each of a thread's four
    for m, got in kinds.items():
        assert len(got) == 7, (K, m, got)
    for m, got in edge.items():
        assert len(got) == 3, (K, m, got)


# ---- '^' ----------------------------------------------------------------------------------------
def _hat_pairs(c):
    """(L, the first '^' of the query) over the case's queries"""
    u = _uncut(c)
    q = lc.key_ints(c.sorted[0])
    return {(int(L), lc.first_hat(x, c.letters)) for L, x in zip(u.L.tolist(), q)}


@pytest.mark.parametrize("K", KS)
def test_hat_at_every_position_of_every_match(K):
    """A first '^' at every letter 1 .. K against a match of every length 6 .. K -- so, under every window, at k_low - 1, k_low,
    the depth, the depth + 1 and k_high + 1."""
    c = lc.case("main%d" % (64 if K == 12 else 128))
    pairs = _hat_pairs(c)
    want = {(L, h) for L in range(lc.RANGE_LETTERS, K + 1) for h in range(1, K + 1)}
    assert want <= pairs, sorted(want - pairs)[:10]
    for kh, kl in lc.WINDOWS[K]:                                       # (spelled out: what the line above implies)
        for L in range(lc.RANGE_LETTERS, K + 1):
            d = min(L, kh)
            for h in (kl - 1, kl, d, d + 1, kh + 1):
                assert not 1 <= h <= K or (L, h) in pairs, (kh, kl, L, h)


@pytest.mark.parametrize("K", KS)
def test_hat_twice_at_the_parting_letter_and_in_the_index(K):
    """two '^' in one query; '^' as the letter at which the query leaves its neighbour; index entries that hold a '^' and are the
    representative of a match that goes beyond it"""
    c = lc.case("main%d" % (64 if K == 12 else 128))
    u = _uncut(c)
    q, idx = lc.key_ints(c.sorted[0]), lc.key_ints(c.ix.kmer)
    letter = lambda x, k: (x >> (5 * (K - k))) & 31
    twice = [x for x in q if sum(letter(x, k) == lc.HAT for k in range(1, K + 1)) >= 2]
    assert len(twice) >= 4
    parting = {int(L) for L, x in zip(u.L.tolist(), q) if lc.RANGE_LETTERS <= L < K and letter(x, L + 1) == lc.HAT}
    assert parting == set(range(lc.RANGE_LETTERS, K)), parting
    inside = {lc.first_hat(idx[int(rep)], K) for rep, L in zip(u.rep.tolist(), u.L.tolist()) if L >= lc.RANGE_LETTERS and 0 < lc.first_hat(idx[int(rep)], K) <= L}
    assert inside == set(range(1, K + 1)), inside


# ---- level windows ------------------------------------------------------------------------------
def test_level_windows():
    """The windows of both key widths (12 .. 3: ten levels, 64-byte records); under each of them a match longer than k_high (the
    cap) and one of 6 letters or more but fewer than k_low (no match in an existing range), where the window leaves room."""
    assert lc.WINDOWS[12] == [(12, 7), (12, 12), (9, 7), (7, 7), (12, 5), (12, 3)] and lc.WINDOWS[25] == [(25, 7), (25, 18), (25, 25), (12, 7)]
    for K in KS:
        for name in ("main%d" % (64 if K == 12 else 128), "main%d+filler" % (64 if K == 12 else 128)):
            c = lc.case(name)
            assert c.windows == lc.WINDOWS[K]
            L = _uncut(c).L
            for kh, kl in c.windows:
                r = _ref(c, (kh, kl))
                assert kh == K or ((L > kh) & (r.depth == kh)).any(), (name, kh, kl)
                assert kl <= lc.RANGE_LETTERS or ((L >= lc.RANGE_LETTERS) & (L < kl) & (r.depth == 0)).any(), (name, kh, kl)
                assert set(range(kl, kh + 1)) <= set(r.depth.tolist()), (name, kh, kl)                  # every level is some query's depth


# ---- 128-bit keys ---------------------------------------------------------------------------
def test_wide_keys_words_and_seam():
    """Matched queries that differ from their representative only in the low word, only in the high word, only in the high
    word's lowest bit (the top bit of letter 13), and first at letter 13 in both words."""
    c = lc.case("main128")
    u = _uncut(c)
    q, idx = c.sorted[0], c.ix.kmer
    seen = set()
    for p in np.flatnonzero((u.L >= lc.RANGE_LETTERS) & (u.L < 25)):
        e = idx[int(u.rep[p])]
        lo, hi = int(q["lo"][p]) ^ int(e["lo"]), int(q["hi"][p]) ^ int(e["hi"])
        seen |= {"low word"} if hi == 0 else set()
        seen |= {"high word"} if lo == 0 else set()
        seen |= {"bit 64"} if (lo, hi) == (0, 1) else set()
        seen |= {"letter 13, both words"} if hi == 1 and lo >> 60 else set()
    assert seen == {"low word", "high word", "bit 64", "letter 13, both words"}, seen


# ---- open groups ------------------------------------------------------------------------------
def _open_blocks(c):
    """positions of the matched queries and the tileNext of the case"""
    r = _ref(c)
    return r, np.flatnonzero(r.depth > 0), lc.tile_next_reference(c.sorted[0], r.depth, 12, 7)


@pytest.mark.parametrize("name", list(lc.OPEN_LAYOUTS))
def test_open_groups_over_tiles(name):
    """Matched queries of reads 0 .. 5 in the first tile, under two or more taxa per k-mer and at every depth 7 .. 12; then tiles
    of queries of the same 6-letter range that match nothing (L == 6 < k_low) -- no special position at any level; then matched
    queries of the same reads.  The groups of levels 10 .. 12 of the first tile close later than those of levels 7 .. 9, and
    later than the groups the middle block opens."""
    c = lc.case(name)
    r, m, nxt = _open_blocks(c)
    q, rd = c.sorted
    assert ((r.depth == 0) == (r.L == lc.RANGE_LETTERS)).all()                                       # a stretch query: the range and nothing more
    assert (np.diff(q.astype(np.uint64) >> np.uint64(30)) == 0).all()                                  # one range
    first = m[m < lc.TILE]
    assert set(r.depth[first].tolist()) == set(range(7, 13)) and set(rd[first].tolist()) == set(range(lc.OPEN_MATCHED_READS))
    idx = c.ix.kmer
    assert all(np.searchsorted(idx, idx[int(j)], side="right") - np.searchsorted(idx, idx[int(j)], side="left") >= 2 for j in set(r.rep[m].tolist()))
    gaps = np.diff(m)
    wide = np.flatnonzero(gaps > lc.TILE)                                                            # the stretches
    assert wide.shape[0] >= 2 and gaps[wide[0]] > 2 * lc.TILE - 40
    middle = m[(m > m[wide[0]]) & (m <= m[wide[1]])]
    later = m[m > m[wide[1]]]
    assert set(rd[middle].tolist()) == set(rd[later][:len(lc.OPEN_DEEP) * 3 + 3].tolist()) == set(range(lc.OPEN_MATCHED_READS))
    assert int(r.depth[middle].max()) == 9
    for lv, k in enumerate(range(12, 6, -1)):
        at = int(nxt[lv, 0])
        assert at in (middle if k <= 9 else later), (k, at)                                            # levels 10 .. 12 stay open over the middle block
        assert all(int(nxt[lv, t]) == at for t in range(1, at // lc.TILE)), k                          # ... and every tile of the stretch says so
    assert int(nxt[5, middle[0] // lc.TILE]) == int(later[0])                                          # the middle block's 7-letter group closes before ...
    assert int(nxt[0, 0]) > int(later[0])                                                              # ... the first tile's 12-letter group does


def test_open_groups_next_special_position_layouts():
    """The next special position of a tile is the first position of the following tile, is the last position of the batch, does
    not exist (the number of queries stands for it) -- the last one also for a tile that is not the batch's last."""
    c = lc.case("open6 edges")
    r, m, nxt = _open_blocks(c)
    assert any(int(nxt[lv, t]) == (t + 1) * lc.TILE for lv in range(6) for t in range(nxt.shape[1] - 1))
    assert int(m[-1]) == c.n - 1 and any(int(nxt[lv, t]) == c.n - 1 for lv in range(6) for t in range(nxt.shape[1] - 1))
    c = lc.case("open6")
    r, m, nxt = _open_blocks(c)
    assert (nxt[:, -2:] == c.n).all() and int(m[-1]) // lc.TILE == nxt.shape[1] - 2


def test_open_groups_over_a_chunk_of_tiles():
    """More than 1024 tiles, 1 049 000 to 1 060 000 queries: the first tile's groups close in the second chunk of 1024 tiles, so
    every tile of the first chunk gets its next position from the chunks' combination."""
    c = lc.case(lc.LARGE)
    assert 1_049_000 <= c.n <= 1_060_000 and not c.wide
    r, m, nxt = _open_blocks(c)
    assert nxt.shape[1] > lc.CHUNK_TILES
    assert (nxt[:, :lc.CHUNK_TILES] >= lc.CHUNK_TILES * lc.TILE).all() and (nxt[:, :lc.CHUNK_TILES] < c.n).all()
    assert len({int(nxt[lv, 0]) for lv in range(6)}) >= 4                                              # the levels differ


def test_scored_cases():
    """The cases compared through scores: every open-group case, and per key width of the other families staged and unstaged
    tiles."""
    assert lc.SCORED == [n for n in lc.case_names() if lc.case(n).score_windows]
    assert set(lc.OPEN_LAYOUTS) <= set(lc.SCORED)
    for K in KS:
        spans = np.concatenate([c.spans[:, 0] for c in _cases(K=K) if c.name in lc.SCORED and c.family != "open"])
        assert (spans <= lc.LSPAN).any() and (spans > lc.LSPAN).any()


# ---- the reference ----------------------------------------------------------------------------
def _oracle_depth(c, kh, kl):
    qs = c.sorted[0]
    p = oracle.params(kh, kl, 3, K=c.letters)
    iv = oracle.IndexView(c.ix)
    a, b = oracle.ranges(iv, p, qs)
    _, ml = oracle.compare_ml(iv, p, qs, np.zeros(c.n, dtype=np.uint32), a, b, 1, closed_form=True)   # (the depth does not ask whose query it is)
    return ml


@pytest.mark.parametrize("name", SMALL)
def test_reference_equals_oracle(name):
    """lookup_reference's depth = the deepest matched level of the oracle's closed form, on every query of every case under every
    window of the case: no query had to be left out, the two definitions agree everywhere."""
    c = lc.case(name)
    for kh, kl in c.windows:
        ref = lc.reference(name, kh, kl)
        ml = _oracle_depth(c, kh, kl)
        bad = np.flatnonzero(ref.depth != ml)
        assert bad.shape[0] == 0, (name, kh, kl, int(bad[0]), int(ref.depth[bad[0]]), int(ml[bad[0]]))


@pytest.mark.parametrize("name", [n for n in SMALL if not lc.case(n).wide])
def test_vectorised_reference_equals_loop(name):
    c = lc.case(name)
    for kh, kl in c.windows:
        a, b = lc.reference(name, kh, kl), lc.lookup_reference_vectorised(c.ix.kmer, c.sorted[0], kh, kl)
        for f in ("depth", "rep", "lo", "la", "lb"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), (name, kh, kl, f)


def test_large_case_reference_and_oracle_in_seconds():
    """The batch of a million queries: the vectorised reference = the oracle, and = the loop on a sample; each in seconds."""
    t0 = time.perf_counter()
    c = lc.open_case(lc.LARGE)                                          # (not the cached one: the times are this test's)
    c.sorted
    t1 = time.perf_counter()
    ref = lc.lookup_reference_vectorised(c.ix.kmer, c.sorted[0], 12, 7)
    t2 = time.perf_counter()
    ml = _oracle_depth(c, 12, 7)
    t3 = time.perf_counter()
    print("\nlarge case: %d queries; built and sorted in %.2f s, vectorised reference %.2f s, oracle %.2f s" % (c.n, t1 - t0, t2 - t1, t3 - t2))
    assert np.array_equal(ref.depth, ml)
    at = np.unique(np.concatenate((np.flatnonzero(ref.depth > 0), np.arange(0, c.n, 997))))
    loop = lc.lookup_reference(c.ix.kmer, c.sorted[0][at], 12, 7, 12)
    assert np.array_equal(loop.depth, ref.depth[at]) and np.array_equal(loop.rep, ref.rep[at])
    assert max(t1 - t0, t2 - t1, t3 - t2) < 10.0


def test_census():
    """The numbers of the corpus (printed with -s): queries per family and key width, tiles on the staged and on the unstaged
    path, counted once per case and window."""
    total = {}
    for c in _cases(large=True):
        key = (c.family, 64 if c.letters == 12 else 128)
        t = total.setdefault(key, [0, 0, 0, 0])
        w = len(c.windows)
        staged = int((c.spans[:, 0] <= lc.LSPAN).sum())
        t[0] += 1; t[1] += c.n * w; t[2] += staged * w; t[3] += (c.spans.shape[0] - staged) * w
    for (family, width), (n, nq, st, un) in sorted(total.items()):
        print("\ncorpus %-5s %3d-bit: %2d cases, %8d queries looked up per flag, %5d staged tiles, %3d unstaged" % (family, width, n, nq, st, un), end="")
    print()
    assert sum(t[3] for t in total.values()) > 0 and sum(t[2] for t in total.values()) > 0
