"""The corpus of hand-made batches for the query sort (tests/sort_corpus.py) is what it claims to be -- one assertion per
category, on the digits in the order in which the named pass reads them (sort_corpus.pass_model), so that an edit of the corpus
cannot silently drop one -- and its plain reference agrees with the oracle on every case, the large ones included.  No device
here: tests/test_gpu_sort_corpus.py feeds the same cases to the device's sort."""
import os
import re

import numpy as np
import pytest

from oracle import oracle
from tests import sort_corpus as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases(family, width=None, variant=None, exact=False):
    """the family's small cases, of the variants that begin with `variant` (or, exact, are it)"""
    out = [c for c in map(sc.case, sc.case_names(family, width))
           if variant is None or (c.meta["variant"] == variant if exact else c.meta["variant"].startswith(variant))]
    assert out, (family, width, variant)
    return out


def _view(c):
    """pass j of the product path as it reads the case's pairs"""
    views, _ = sc.pass_model(c.keys, sc.SHIFTS[c.width])
    return views[c.meta["j"]]


def _every_pass(family, variant):
    """the family's cases of that variant, with one for every pass of the product path in both widths"""
    cs = _cases(family, variant=variant, exact=True)
    assert {(c.width, c.meta["j"]) for c in cs} == {(w, j) for w in sc.WIDTHS for j in range(len(sc.SHIFTS[w]))}, (family, variant)
    return [(c, _view(c)) for c in cs]


# ---- the constants ------------------------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    radix = open(os.path.join(ROOT, "kasa_amd", "csrc", "kasa_radix.h")).read()
    hip = open(os.path.join(ROOT, "kasa_amd", "csrc", "kasa_hip.hip")).read()
    assert "THREADS = 1024, WAVES = THREADS / 64, RADIX = 256" in radix and "ITEMS = sizeof(Key) == 8 ? 8 : 4, SIZE = THREADS * ITEMS" in radix
    assert sc.T == {64: 1024 * 8, 128: 1024 * 4} and sc.STRIPE_ROWS == {64: 8, 128: 4} and sc.STRIPES == 1024 // 64
    assert all(sc.T[w] == sc.STRIPES * sc.STRIPE_ROWS[w] * sc.ROW for w in sc.WIDTHS)
    assert "SORT_TOP = 32, SORT_TOP_OLD = 40" in hip and "SORT_BUCKET_LIMIT = 1024" in hip and "SORT_BIG_LONGEST = 1u << 20" in hip
    assert "RANK_TILE = 2048, RANK_HALO = 128" in hip
    assert re.search(r"\(sizeof\(Key\) == 8\) != \(\(c->debugFlags & 2097152\) != 0\)\) \? SORT_TOP : SORT_TOP_OLD", hip)
    for w, top, other in ((64, 32, 40), (128, 40, 32)):
        bits = sc.KEY_BITS[w]
        assert sc.SHIFTS[w] == tuple(range(bits - top, bits, 8)) and sc.SHIFTS_OTHER[w] == tuple(range(bits - other, bits, 8))
        assert sc.LOW[w] == bits - top and sc.LOW_OTHER[w] == bits - other
    # two workgroups of pass_kernel per CU by their LDS (64 KiB + tables of 160 KiB), 256 CUs
    assert sc.RESIDENT == 2 * 256 and sc.CHAIN_TILES > sc.RESIDENT


def test_every_case_is_a_batch_of_the_stated_ranges():
    """keys in [1, 2^60) or [1, 2^125), payloads a permutation of 0 .. n - 1, the flags of the width"""
    for name in sc.case_names():
        c = sc.case(name)
        bits = sc.KEY_BITS[c.width]
        top = c.keys if c.width == 64 else c.keys["hi"]
        assert not (top >> np.uint64(bits - (0 if c.width == 64 else 64))).any(), name
        assert (c.keys != 0).all() if c.width == 64 else ((c.keys["lo"] | c.keys["hi"]) != 0).all(), name
        assert np.array_equal(np.sort(c.payload), np.arange(c.n, dtype=np.uint32)), name
        assert c.flags == sc.FLAGS[c.width] and sc.PRODUCT in c.flags and {sc.LIB_PASSES, sc.LIBRARY} < set(c.flags), name
    assert sc.GENERIC in sc.FLAGS[64] and sc.GENERIC not in sc.FLAGS[128]


# ---- families for the passes ------------------------------------------------------------------------------------------------------
def test_pass_families_arrive_as_written():
    """The digits below pass j are constant, so pass j reads the pairs in batch order; n = 2T + 37 unless the family says
    otherwise."""
    for family in ("one_digit", "ends", "rows", "tile_runs", "descending"):
        for c in _cases(family):
            v = _view(c)
            assert np.array_equal(v.order, np.arange(c.n)), c.name
            assert family == "tile_runs" or c.n == 2 * sc.T[c.width] + 37, c.name


def test_one_digit():
    """every tile of pass j holds one digit only; one variant has every pass constant: the batch is one long bucket"""
    for c, v in _every_pass("one_digit", "one pass"):
        assert ((v.hist > 0).sum(axis=1) == 1).all() and np.unique(v.digits).shape[0] == 1, c.name
    for w in sc.WIDTHS:
        (c,) = _cases("one_digit", w, "all passes")
        views, _ = sc.pass_model(c.keys, sc.SHIFTS[w])
        assert all(np.unique(v.digits).shape[0] == 1 for v in views), c.name
        starts, sizes = sc.bucket_runs(sc.reference(c.keys, c.payload)[0], sc.LOW[w])
        assert sizes.tolist() == [c.n] and sc.LIMIT < c.n <= sc.BIG_LONGEST, c.name


def test_ends():
    """only the first and the last digit of the scan over digits: alternating, all 0 then all 255, all 255 then all 0"""
    for variant in ("alternating", "0 then 255", "255 then 0"):
        for c, v in _every_pass("ends", variant):
            d = v.digits
            assert set(np.unique(d).tolist()) == {0, 255}, c.name
            if variant == "alternating":
                assert np.array_equal(d, np.arange(c.n) % 2 * 255), c.name
            else:
                step = np.flatnonzero(np.diff(d))
                assert step.tolist() == [c.n // 2 - 1] and d[0] == (0 if variant == "0 then 255" else 255), c.name


def _full_rows(v):
    n = v.digits.shape[0] // sc.ROW * sc.ROW
    return v.digits[:n].reshape(-1, sc.ROW), v.digits[n:]


def test_rows_of_64_distinct_digits():
    for c, v in _every_pass("rows", "a"):
        rows, rest = _full_rows(v)
        assert (np.diff(np.sort(rows, axis=1), axis=1) > 0).all() and np.unique(rest).shape[0] == rest.shape[0] > 0, c.name


def test_rows_of_one_digit_each():
    for c, v in _every_pass("rows", "b"):
        rows, rest = _full_rows(v)
        assert (rows == rows[:, :1]).all() and (np.diff(rows[:, 0]) != 0).all(), c.name
        assert (rest == rest[0]).all() and rest[0] != rows[-1, 0], c.name


def test_wave_stripes_of_one_digit_each():
    """every wave stripe holds one digit, the 16 stripes of a tile are all different"""
    for c, v in _every_pass("rows", "c"):
        stripe = sc.ROW * sc.STRIPE_ROWS[c.width]
        for t in range(v.hist.shape[0]):
            d = v.tile(t, c.width)
            per = [np.unique(d[s:s + stripe]) for s in range(0, d.shape[0], stripe)]
            assert all(p.shape[0] == 1 for p in per) and len({int(p[0]) for p in per}) == len(per), (c.name, t)
            assert len(per) == (sc.STRIPES if t < 2 else 1), (c.name, t)


def test_rows_whose_first_and_last_lane_share_a_digit():
    """lanes 0 and 63 of every full row share a digit that no other lane of the row has"""
    for c, v in _every_pass("rows", "d"):
        rows, rest = _full_rows(v)
        assert (rows[:, 0] == rows[:, -1]).all() and ((rows == rows[:, :1]).sum(axis=1) == 2).all(), c.name
        assert (rest[1:] != rest[0]).all(), c.name


def test_a_digit_fills_a_tiles_worth_of_positions():
    """exactly T consecutive positions, starting at a tile's first position - 1, + 0 and + 1; n = 4T"""
    for off in (-1, 0, 1):
        for c, v in _every_pass("tile_runs", "a tile's worth at %+d" % off):
            Tw, x = sc.T[c.width], c.meta["x"]
            at = np.flatnonzero(v.digits == x)
            assert c.n == 4 * Tw and at.shape[0] == Tw and at[0] == Tw + off and at[-1] == 2 * Tw + off - 1, c.name
            assert v.hist[:, x].tolist() == {-1: [1, Tw - 1, 0, 0], 0: [0, Tw, 0, 0], 1: [0, Tw - 1, 1, 0]}[off], c.name


def test_a_digit_only_in_a_partial_last_tile():
    for r in sc.TAILS:
        for c, v in _every_pass("tile_runs", "only in a last tile of %d" % r):
            x = c.meta["x"]
            assert c.n == 3 * sc.T[c.width] + r and v.hist[:, x].tolist() == [0, 0, 0, r] and v.hist[3].sum() == r, c.name
    assert sc.TAILS == (1, 63, 64, 65)


def test_a_digit_in_the_first_and_the_last_tile_only():
    """the look-back adds zero counts for it over every tile between"""
    for c, v in _every_pass("tile_runs", "first and last tile only"):
        h = v.hist[:, c.meta["x"]]
        assert c.n == 4 * sc.T[c.width] and h[0] > 0 and h[3] > 0 and h[1:3].tolist() == [0, 0], c.name


def test_descending():
    """the digit falls from 255 to 0 over the batch"""
    for c, v in _every_pass("descending", "falling"):
        assert v.digits[0] == 255 and v.digits[-1] == 0 and (np.diff(v.digits) <= 0).all() and np.unique(v.digits).shape[0] == 256, c.name


def test_descending_stairs():
    """equal-digit runs of 1, 64, 65, 1023, 1024, 1025 and T pairs, each a digit below the one before (255 after 0): every run moves"""
    for run in sc.STAIRS:
        for c, v in _every_pass("descending", "stairs of %s" % run):
            r = sc.T[c.width] if run == "T" else run
            edge = np.flatnonzero(np.diff(v.digits)) + 1
            lengths = np.diff(np.concatenate(([0], edge, [c.n])))
            assert (lengths[:-1] == r).all() and 0 < lengths[-1] <= r and lengths.shape[0] >= 3, c.name
            heads = v.digits[np.concatenate(([0], edge))]
            assert heads[0] == 255 and ((heads[:-1] - heads[1:]) % 256 == 1).all(), c.name
    assert sc.STAIRS == (1, 64, 65, 1023, 1024, 1025, "T")


# ---- bucket families ------------------------------------------------------------------------------------------------------------
def _layout(c):
    """the buckets of the sorted batch are the builder's"""
    starts, sizes = sc.bucket_runs(sc.reference(c.keys, c.payload)[0], c.meta["low_bits"])
    assert np.array_equal(starts, c.meta["starts"]) and np.array_equal(sizes, c.meta["sizes"]), c.name
    return starts, sizes


def _holds(c, starts, sizes):
    """the case's buckets of meta["m"] members at the positions meta["at"]"""
    for at in c.meta["at"]:
        b = np.flatnonzero(starts == at)
        assert b.shape[0] == 1 and sizes[b[0]] == c.meta["m"], (c.name, at)


LOWS128 = (sc.LOW[128], sc.LOW_OTHER[128])


def _b128(low_bits, variant, exact=False):
    return [c for c in _cases("buckets128", 128, variant, exact) if c.meta["low_bits"] == low_bits]


@pytest.mark.parametrize("low_bits", LOWS128)
def test_wide_buckets_are_where_the_builder_put_them(low_bits):
    """every bucket case, with its buckets' low part of 85 and of 93 bits"""
    names = [n for n in sc.case_names("buckets128") if n.endswith("low %d" % low_bits)]
    assert len(names) == len(sc.case_names("buckets128")) // 2
    for n in names:
        _layout(sc.case(n))


@pytest.mark.parametrize("low_bits", LOWS128)
def test_wide_batch_sizes(low_bits):
    assert sorted(c.n for c in _b128(low_bits, "batch of")) == sorted(sc.BATCH_SIZES)


@pytest.mark.parametrize("low_bits", LOWS128)
def test_wide_short_buckets_at_every_alignment_and_buckets_longer_than_a_row(low_bits):
    seen = set()
    for c in _b128(low_bits, "short buckets") + _b128(low_bits, "buckets of"):
        if "aligned" not in c.meta:
            continue
        starts, sizes = _layout(c)
        for b, mod, r in c.meta["aligned"]:
            assert starts[b] % mod == r and sizes[b] == c.meta["m"], c.name
            seen.add((c.meta["m"], mod, r))
    assert {(m, 4, r) for m in (1, 2, 3, 4, 5, 7, 8, 9) for r in range(4)} <= seen
    assert {(m, 64, r) for m in (63, 64, 65, 127, 128, 129, 200) for r in (0, 1, 2, 3, 31, 62, 63)} <= seen


@pytest.mark.parametrize("low_bits", LOWS128)
def test_wide_buckets_at_the_limit(low_bits):
    """LIMIT - 1, LIMIT and LIMIT + 1 members inside the first tile, over a tile boundary and inside the second tile"""
    seen = set()
    for c in _b128(low_bits, "bucket of"):
        if "e" in c.meta:
            continue
        starts, sizes = _layout(c)
        _holds(c, starts, sizes)
        a, m = c.meta["at"][0], c.meta["m"]
        seen.add((m - sc.LIMIT, a // sc.RANK_TILE, (a + m - 1) // sc.RANK_TILE))
    assert seen == {(d, *where) for d in (-1, 0, 1) for where in ((0, 0), (0, 1), (1, 1))}


@pytest.mark.parametrize("low_bits", LOWS128)
def test_wide_buckets_over_a_tile_boundary(low_bits):
    """ending e positions behind a boundary, with e and the reach before it below, at and above RANK_HALO; at two boundaries"""
    reach, behind = set(), set()
    for c in _b128(low_bits, "bucket of"):
        if "e" not in c.meta:
            continue
        starts, sizes = _layout(c)
        _holds(c, starts, sizes)
        m, e = c.meta["m"], c.meta["e"]
        assert [a + m - k * sc.RANK_TILE for k, a in zip((1, 2), c.meta["at"])] == [e, e] and c.n == 3 * sc.RANK_TILE + 5, c.name
        reach.add(int(np.sign(m - e - sc.RANK_HALO))); behind.add(int(np.sign(e - sc.RANK_HALO)))
    assert reach == behind == {-1, 0, 1}


@pytest.mark.parametrize("low_bits", LOWS128)
def test_wide_buckets_at_both_ends_singletons_and_one_bucket(low_bits):
    tails = set()
    for c in _b128(low_bits, "buckets of"):
        if "tail" not in c.name:
            continue
        starts, sizes = _layout(c)
        assert c.meta["at"] == [0, c.n - c.meta["m"]] and c.n == c.meta["n"], c.name
        _holds(c, starts, sizes)
        tails.add(c.n - 2 * sc.RANK_TILE)
    assert tails == {1, sc.RANK_HALO, sc.RANK_HALO + 1, sc.RANK_TILE}
    (c,) = _b128(low_bits, "all singletons")
    assert (_layout(c)[1] == 1).all() and c.n == 2 * sc.RANK_TILE + 77
    assert sorted(_layout(c)[1].tolist() for c in _b128(low_bits, "one bucket")) == [[1000], [5000]]


def _tops(c):
    return np.unique(sc.formats.key_shr(c.keys, c.meta["low_bits"]))


@pytest.mark.parametrize("low_bits", LOWS128)
def test_wide_neighbouring_buckets_differ_in_the_lowest_top_bit(low_bits):
    for c in _b128(low_bits, "neighbouring"):
        _layout(c)
        tops = _tops(c)
        pairs = np.flatnonzero(np.diff(tops) == 1)
        assert pairs.shape[0] == 4 and (tops[pairs] % 2 == 0).all(), c.name                 # (x, x + 1) with x even: bit 0 of the top only
    assert sorted(c.meta["m"] for c in _b128(low_bits, "neighbouring")) == [1, 3, 8, 70]


def _members(c, at):
    """the low parts (Python ints) of the bucket that starts at `at` after the passes, in input order"""
    low = c.meta["low_bits"]
    ks, _ = sc.reference(c.keys, c.payload)
    top = sc.key_ints(ks[at:at + 1])[0] >> low
    return [x & ((1 << low) - 1) for x in sc.key_ints(c.keys) if x >> low == top]


@pytest.mark.parametrize("low_bits", LOWS128)
@pytest.mark.parametrize("pattern", sc.PATTERNS)
def test_wide_value_patterns(low_bits, pattern):
    """what only a right 128-bit compare orders: in buckets of 2 to 150 members at every residue mod 4 and one over a tile boundary"""
    (c,) = _b128(low_bits, "values: " + pattern, exact=True)
    starts, sizes = _layout(c)
    _holds(c, starts, sizes)
    assert {int(s) % 4 for s, m in zip(starts, sizes) if m in (6, 9, 16, 37, 64, 150, 11, 21)} == {0, 1, 2, 3}
    v = _members(c, c.meta["at"][0])
    lo, hi = [x & (2**64 - 1) for x in v], [x >> 64 for x in v]
    assert len(v) == 40
    one_bit = {"lo bit 0": 0, "lo bit 63": 63, "bit 64": 64, "highest low bit": low_bits - 1}
    if pattern in one_bit:
        assert {x ^ v[0] for x in v} == {0, 1 << one_bit[pattern]}
        assert v != sorted(v)
    elif pattern == "equal hi, lo descends":
        assert len(set(hi)) == 1 and all(a > b for a, b in zip(lo, lo[1:])) and lo[0] >> 63
    elif pattern == "equal lo, hi descends":
        assert len(set(lo)) == 1 and all(a > b for a, b in zip(hi, hi[1:])) and lo[0] >> 63
    elif pattern == "crossed":
        by_hi = sorted(range(40), key=lambda i: hi[i])
        assert len(set(hi)) == 40 and all(lo[a] > lo[b] for a, b in zip(by_hi, by_hi[1:])) and by_hi != list(range(40))
    elif pattern == "extremes":
        assert set(v) == {0, (1 << low_bits) - 1}
    else:
        assert pattern == "equal" and len(set(v)) == 1
    if pattern == "lo bit 63":
        assert (c.keys["lo"] >> np.uint64(63)).any()


# ---- long buckets -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", sc.WIDTHS)
def test_long_buckets(width):
    """LIMIT + 1, 1500 and 5000 members at position 0, over a RANK_TILE boundary and ending at n; two side by side with
    neighbouring top bits; three in one batch with short ones between"""
    where = set()
    for c in _cases("long", width):
        starts, sizes = _layout(c)
        long_ = np.flatnonzero(sizes > sc.LIMIT)
        assert sizes[long_].tolist() == c.meta["long"], c.name
        if "at" in c.meta:
            _holds(c, starts, sizes)
            a, m = c.meta["at"][0], c.meta["m"]
            where.add((m, "first" if a == 0 else "last" if a + m == c.n else "over" if a // sc.RANK_TILE != (a + m - 1) // sc.RANK_TILE else "?"))
        elif "neighbours" in c.meta:
            tops = _tops(c)
            assert long_[1] == long_[0] + 1 and np.flatnonzero(np.diff(tops) == 1).tolist() == [long_[0]], c.name
        else:
            assert len(long_) == 3 and (np.diff(long_) > 1).all() and long_[0] > 0 and long_[-1] < sizes.shape[0] - 1, c.name
    assert where == {(m, w) for m in sc.LONG_SIZES for w in ("first", "over", "last")}
    assert sc.LONG_SIZES[0] == sc.LIMIT + 1


# ---- the reference, the mirror ----------------------------------------------------------------------------------------------------
FAMILIES = ("one_digit", "ends", "rows", "tile_runs", "descending", "buckets128", "long")


def _equals_oracle(c):
    ks, ps = sc.reference(c.keys, c.payload)
    ko, po = oracle.sort_queries(c.keys, c.payload)
    assert sc.first_difference(ks, ko) is None and sc.first_difference(ps, po) is None, c.name
    return ks, ps


@pytest.mark.parametrize("family", FAMILIES)
def test_reference_equals_oracle(family):
    """numpy's stable sort = oracle.sort_queries, keys and payloads, on every small case"""
    assert set(FAMILIES) == {sc._BUILDERS[n][0] for n in sc.case_names()}
    for c in _cases(family):
        _equals_oracle(c)


@pytest.mark.parametrize("family", FAMILIES)
def test_mirror_equals_reference(family):
    """The CPU mirror of the device's way -- stripe counts, running sums, look-back, digit starts, bucket order -- gives the
    reference's result under both splits of passes and buckets: what a broken copy of it gets wrong, it gets wrong by the break."""
    for c in _cases(family):
        ks, ps = sc.reference(c.keys, c.payload)
        for other in (False, True):
            km, pm = sc.mirror_sort(c.keys, c.payload, other)
            assert sc.first_difference(km, ks) is None and sc.first_difference(pm, ps) is None, (c.name, other)


@pytest.mark.parametrize("name", sc.case_names(large=True))
def test_large_cases(name):
    """chain: 530 tiles -- more than the 512 workgroups the chip holds at once -- of random digits, or of one digit in pass j,
    for every pass j of both widths; long: one bucket of exactly SORT_BIG_LONGEST members, and of one more.  Reference = oracle."""
    c = sc.case(name)
    ks, _ = _equals_oracle(c)
    if c.family == "chain":
        Tw = sc.T[c.width]
        assert c.n == sc.CHAIN_TILES * Tw and c.n // Tw > sc.RESIDENT and c.flags == sc.CHAIN_FLAGS
        views, _ = sc.pass_model(c.keys, sc.SHIFTS[c.width])
        if c.meta["variant"] == "random":
            assert all(((v.hist > 0).sum(axis=1) >= 250).all() for v in views)
        else:
            v = views[c.meta["j"]]
            assert np.array_equal(v.order, np.arange(c.n)) and ((v.hist > 0).sum(axis=1) == 1).all()
    else:
        starts, sizes = sc.bucket_runs(ks, c.meta["low_bits"])
        assert c.width == 64 and sizes.max() == c.meta["m"] and c.meta["m"] in (sc.BIG_LONGEST, sc.BIG_LONGEST + 1) and c.flags == sc.BIGGEST_FLAGS
        assert c.n == c.meta["m"] + 3000 and np.count_nonzero(sizes > sc.LIMIT) == 1


def test_large_cases_are_all_there():
    names = sc.case_names(large=True)
    assert {n for n in names if n.startswith("chain/one digit")} == {"chain/one digit/%d/pass %d" % (w, j) for w in sc.WIDTHS for j in range(len(sc.SHIFTS[w]))}
    assert {"chain/random/64", "chain/random/128"} < set(names) and len(names) == 13


def test_census():
    """the numbers of the corpus (printed with -s): cases and pairs per family and key width, per flag"""
    total = {}
    for n in sc.case_names():
        c = sc.case(n)
        t = total.setdefault((c.family, c.width), [0, 0])
        t[0] += 1; t[1] += c.n
    for (family, width), (cases, pairs) in sorted(total.items()):
        print("\ncorpus %-10s %3d-bit: %3d cases, %8d pairs sorted per flag" % (family, width, cases, pairs), end="")
    print()
    assert len(total) == 5 * 2 + 1 + 2
