"""Hand-made batches for the query sort (kasa_radix.h: hist_kernel, starts_kernel, pass_kernel; then the bucket kernels and the
long-bucket path of sort_and_range_impl), for 64-bit and 128-bit keys, with a plain reference.  No device code here:
tests/test_sort_corpus_cpu.py shows that every case holds what its family claims, tests/test_gpu_sort_corpus.py feeds the same
cases to Context.set_queries -> sort_and_range -> queries.

Three groups of families:
  * pass families -- a digit pattern in ONE radix pass j of the product path, in the order in which that pass reads the pairs.
    The digits of the passes below j are constant over the batch, so those passes (stable) keep the batch order and the
    pattern arrives as it was written; pass_model() shows that it does.  The digits above j are drawn from a few values (or
    held constant), the bits below the passes at random with ties, so that the bucket stage has work.
  * bucket families -- built from the passes' output backwards, as tests/test_gpu_bucket_rank.py does for 64-bit keys: a list
    of buckets with ascending top bits, each with its member count and its low bits in input order; the batch is a random
    interleaving that keeps every bucket's members in order.  Here for 128-bit keys, whose low part (85 or 93 bits) straddles
    the two 64-bit words, with value patterns that only a 128-bit compare can get wrong.
  * long buckets -- more than SORT_BUCKET_LIMIT members: at both ends of the batch, over a tile boundary, side by side, several
    in one batch, and exactly SORT_BIG_LONGEST members and one more.

The reference is numpy: np.argsort(kind="stable") for uint64 keys, np.lexsort((lo, hi)) for KEY128_DTYPE.  Payloads are a
permutation of 0 .. n - 1, so a member out of place among equal keys shows.

mirror_sort() is a CPU mirror of the device's way to the same result -- per wave stripe counts, running sums over a tile's
waves, the look-back over the tiles before, the digit starts, then the order inside the buckets -- in small functions
(wave_counts, look_back, bucket_rank_order), so that a deliberately broken copy of one of them shows which families notice."""
import functools
import zlib
from dataclasses import dataclass, field

import numpy as np

from kasa_amd import formats
from kasa_amd.formats import KEY128_DTYPE

# ---- the constants of the code under test, restated once -----------------------------------------------------------------
WIDTHS = (64, 128)
LETTERS = {64: 12, 128: 25}
KEY_BITS = {64: 60, 128: 125}                       # KeyTraits<Key>::BITS: 5 bits per letter
T = {64: 8192, 128: 4096}                           # kasa_radix::Tile<Key>::SIZE: the pairs of one pass_kernel workgroup
ROW = 64                                            # a wave row: 64 consecutive pairs
STRIPE_ROWS = {64: 8, 128: 4}                       # Tile<Key>::ITEMS: the rows of one wave's stripe
STRIPES = 16                                        # kasa_radix::WAVES: stripes per tile
SHIFTS = {64: (28, 36, 44, 52), 128: (85, 93, 101, 109, 117)}           # the passes of the product path
SHIFTS_OTHER = {64: (20, 28, 36, 44, 52), 128: (93, 101, 109, 117)}     # ... under flag 2097152
LOW = {64: 28, 128: 85}                             # key bits below a bucket's, product path
LOW_OTHER = {64: 20, 128: 93}
RANK_TILE, RANK_HALO, LIMIT, BIG_LONGEST = 2048, 128, 1024, 1 << 20     # RANK_TILE, RANK_HALO, SORT_BUCKET_LIMIT, SORT_BIG_LONGEST
RESIDENT = 512                                      # pass_kernel workgroups on the chip at once: 256 CUs, two per CU by LDS
CHAIN_TILES = 530

PRODUCT, FIRST, OTHER, GENERIC, LIB_PASSES, LIBRARY, LAST_RESORT = 0, 524288, 2097152, 4194304, 512, 64, 128
FLAGS = {64: (PRODUCT, FIRST, OTHER, GENERIC, LIB_PASSES, LIBRARY), 128: (PRODUCT, FIRST, OTHER, LIB_PASSES, LIBRARY)}
CHAIN_FLAGS = (PRODUCT, FIRST, LIBRARY)
BIGGEST_FLAGS = (PRODUCT, LAST_RESORT)

BATCH_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, RANK_TILE - 1, RANK_TILE, RANK_TILE + 1, RANK_TILE + RANK_HALO - 1, RANK_TILE + RANK_HALO,
               RANK_TILE + RANK_HALO + 1, 3 * RANK_TILE + 5)
STAIRS = (1, 64, 65, 1023, 1024, 1025, "T")
TAILS = (1, 63, 64, 65)
LONG_SIZES = (LIMIT + 1, 1500, 5000)
PATTERNS = ("lo bit 0", "lo bit 63", "bit 64", "highest low bit", "equal hi, lo descends", "equal lo, hi descends", "crossed", "extremes", "equal")


# ---- keys of both widths ---------------------------------------------------------------------------------------------------
def zeros(n, width):
    return np.zeros(n, dtype=np.uint64 if width == 64 else KEY128_DTYPE)


def width_of(keys):
    return 128 if keys.dtype == KEY128_DTYPE else 64


def put(keys, shift, values):
    """keys |= values << shift, in place; values: uint64, a scalar or one per key, over the seam of the two words if need be."""
    v = np.asarray(values, dtype=np.uint64)
    if width_of(keys) == 64:
        keys |= v << np.uint64(shift)
    elif shift >= 64:
        keys["hi"] |= v << np.uint64(shift - 64)
    else:
        keys["lo"] |= v << np.uint64(shift)
        if shift:
            keys["hi"] |= v >> np.uint64(64 - shift)
    return keys


def digit(keys, shift):
    return (formats.key_shr(keys, shift) & np.uint64(255)).astype(np.int64)


def key_ints(keys):
    if width_of(keys) == 64:
        return [int(x) for x in keys]
    return [(int(h) << 64) | int(l) for l, h in zip(keys["lo"], keys["hi"])]


def random_low(rng, n, width, nbits):
    """n keys with random bits below `nbits`"""
    k = zeros(n, width)
    if width == 64:
        k |= rng.integers(0, 1 << nbits, size=n, dtype=np.uint64)
    else:
        k["lo"] = rng.integers(0, 1 << min(nbits, 64), size=n, dtype=np.uint64)
        if nbits > 64:
            k["hi"] = rng.integers(0, 1 << (nbits - 64), size=n, dtype=np.uint64)
    return k


def mixed_low(rng, n, width, nbits):
    """... half of them drawn from four values, so that ties are common"""
    k = random_low(rng, n, width, nbits)
    few = random_low(rng, 4, width, nbits)
    tie = rng.random(n) < 0.5
    k[tie] = few[rng.integers(0, 4, size=n)][tie]
    return k


def not_zero(keys):
    """keys lie in [1, 2^BITS)"""
    if width_of(keys) == 64:
        keys[keys == 0] = 1
    else:
        keys["lo"][(keys["lo"] == 0) & (keys["hi"] == 0)] = 1
    return keys


# ---- the plain reference ---------------------------------------------------------------------------------------------------
def order_of(keys):
    """the stable ascending order of the keys"""
    if width_of(keys) == 128:
        return np.lexsort((keys["lo"], keys["hi"]))
    return np.argsort(keys, kind="stable")


def reference(keys, payload):
    o = order_of(keys)
    return keys[o], payload[o]


def first_difference(a, b):
    """position of the first difference of two arrays of one length, or None"""
    bad = np.flatnonzero(a != b)
    return int(bad[0]) if bad.shape[0] else None


def bucket_runs(sorted_keys, low_bits):
    """(start, members) of every run of equal bits above `low_bits`"""
    n = sorted_keys.shape[0]
    if width_of(sorted_keys) == 64:
        top = sorted_keys >> np.uint64(low_bits)
        new = top[1:] != top[:-1]
    else:
        a, b = formats.key_shr(sorted_keys, low_bits), sorted_keys["hi"] >> np.uint64(max(low_bits, 64) - 64)
        new = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
    starts = np.flatnonzero(np.concatenate(([True], new)))
    return starts, np.diff(np.concatenate((starts, [n])))


# ---- a model of what each pass sees ----------------------------------------------------------------------------------------
@dataclass
class PassView:
    shift: int
    order: np.ndarray       # order[i] = the batch position of the pair the pass reads as its i-th
    digits: np.ndarray      # the pass's digit of that pair
    hist: np.ndarray        # [tiles, 256]: the digit counts of every tile

    def tile(self, t, width):
        return self.digits[t * T[width]:(t + 1) * T[width]]


def pass_model(keys, shifts):
    """For each pass the order in which it reads the pairs -- numpy's stable sort by the digits of the passes before -- with the
    digits in that order and the digit histogram of every tile; and the order the last pass leaves."""
    width, n = width_of(keys), keys.shape[0]
    tiles = (n + T[width] - 1) // T[width]
    tile_of = np.arange(n) // T[width]
    order = np.arange(n)
    views = []
    for s in shifts:
        d = digit(keys, s)[order]
        hist = np.bincount(tile_of * 256 + d, minlength=tiles * 256).reshape(tiles, 256)
        views.append(PassView(s, order, d, hist))
        order = order[np.argsort(d.astype(np.uint8), kind="stable")]
    return views, order


# ---- a CPU mirror of the device's way ------------------------------------------------------------------------------------------
def wave_counts(d, width):
    """[stripes of the batch, 256]: how often a wave's stripe holds each digit (pass_kernel's sCnt, before the running sums)"""
    stripe = np.arange(d.shape[0]) // (ROW * STRIPE_ROWS[width])
    tiles = (d.shape[0] + T[width] - 1) // T[width]
    return np.bincount(stripe * 256 + d, minlength=tiles * STRIPES * 256).reshape(tiles * STRIPES, 256)


def look_back(total):
    """[tiles, 256] -> the pairs with the digit in all earlier tiles"""
    return np.cumsum(total, axis=0) - total


def bucket_rank_order(keys):
    """the order inside the buckets, the buckets staying where the passes put them: what counting the members that order
    before one's own comes to -- a stable sort of the passes' output by the whole key"""
    return order_of(keys)


def mirror_pass(keys, payload, shift):
    width, n = width_of(keys), keys.shape[0]
    d = digit(keys, shift)
    cnt = wave_counts(d, width).reshape(-1, STRIPES, 256)
    wave_base = np.cumsum(cnt, axis=1) - cnt                        # the waves' counts become running sums
    total = cnt.sum(axis=1)                                         # the tile's count of the digit: what it publishes
    hist = np.bincount(d, minlength=256)                            # hist_kernel, starts_kernel
    start = np.cumsum(hist) - hist
    prev = look_back(total)
    stripe = np.arange(n) // (ROW * STRIPE_ROWS[width])
    g = stripe * 256 + d                                            # rank inside the wave: among its pairs with the digit, in row and lane order
    o = np.argsort(g, kind="stable")
    gs = g[o]
    first = np.flatnonzero(np.concatenate(([True], gs[1:] != gs[:-1])))
    within = np.empty(n, dtype=np.int64)
    within[o] = np.arange(n) - np.repeat(first, np.diff(np.concatenate((first, [n]))))
    tile = stripe // STRIPES
    dest = start[d] + prev[tile, d] + wave_base[tile, stripe % STRIPES, d] + within
    ko, vo = np.zeros_like(keys), np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    ko[dest] = keys
    vo[dest] = payload
    return ko, vo


def mirror_sort(keys, payload, other=False):
    k, v = keys, payload
    for s in (SHIFTS_OTHER if other else SHIFTS)[width_of(keys)]:
        k, v = mirror_pass(k, v, s)
    o = bucket_rank_order(k)
    return k[o], v[o]


# ---- cases -----------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    family: str
    width: int
    keys: np.ndarray
    payload: np.ndarray
    flags: tuple
    meta: dict = field(default_factory=dict)

    @property
    def n(self):
        return self.keys.shape[0]


_BUILDERS = {}          # name -> (family, width, large, build(rng) -> (keys, flags, meta))


def _add(name, family, width, build, large=False):
    assert name not in _BUILDERS, name
    _BUILDERS[name] = (family, width, large, build)


def _seed(name):
    return zlib.crc32(name.encode())


def build_case(name):
    family, width, _, build = _BUILDERS[name]
    rng = np.random.default_rng(_seed(name))
    keys, flags, meta = build(rng)
    keys = not_zero(keys)
    payload = rng.permutation(keys.shape[0]).astype(np.uint32)
    return Case(name, family, width, keys, payload, flags, meta)


@functools.lru_cache(maxsize=None)
def _small(name):
    return build_case(name)


def case(name):
    """the case of that name; the small ones are kept"""
    return build_case(name) if _BUILDERS[name][2] else _small(name)


def case_names(family=None, width=None, large=False):
    return [n for n, (f, w, big, _) in _BUILDERS.items() if big == large and family in (None, f) and width in (None, w)]


# ---- families for the passes ---------------------------------------------------------------------------------------------------
def pass_keys(rng, width, j, dj, above="few"):
    """Keys whose digit in pass j of the product path is dj, one per pair: the digits of the passes below j are one value each,
    those above come from three values each ("few") or are one value each ("const"), the bits below the passes are random."""
    n, shifts = dj.shape[0], SHIFTS[width]
    k = mixed_low(rng, n, width, shifts[0])
    for p, s in enumerate(shifts):
        if p == j:
            put(k, s, dj)
        elif p < j or above == "const":
            put(k, s, int(rng.integers(0, 256)))
        else:
            put(k, s, rng.integers(0, 256, size=3)[rng.integers(0, 3, size=n)])
    return k


def _others(rng, n, x):
    """n random digits, none of them x"""
    r = rng.integers(0, 255, size=n)
    return r + (r >= x)


def _n_default(width):
    return 2 * T[width] + 37


def _one_digit(rng, width):
    return np.full(_n_default(width), int(rng.integers(0, 256)), dtype=np.int64), {}


def _ends(which):
    def make(rng, width):
        n = _n_default(width)
        i = np.arange(n)
        half = (i >= n // 2).astype(np.int64)
        return {"alternating": i % 2, "0 then 255": half, "255 then 0": 1 - half}[which] * 255, {}
    return make


def _rows(which):
    def make(rng, width):
        n = _n_default(width)
        rows = (n + ROW - 1) // ROW
        if which == "a":                                                 # 64 distinct digits in every row
            d = np.concatenate([rng.choice(256, size=ROW, replace=False) for _ in range(rows)])[:n]
        elif which == "b":                                               # one digit per row, neighbouring rows differ
            d = np.repeat(np.cumsum(rng.integers(1, 256, size=rows)) % 256, ROW)[:n]
        elif which == "c":                                               # one digit per wave stripe, a tile's 16 stripes all different
            tiles = (n + T[width] - 1) // T[width]
            per = np.concatenate([rng.choice(256, size=STRIPES, replace=False) for _ in range(tiles)])
            d = np.repeat(per, ROW * STRIPE_ROWS[width])[:n]
        else:                                                            # lanes 0 and 63 share a digit that no other lane has
            d = np.empty(rows * ROW, dtype=np.int64)
            for r in range(rows):
                x = int(rng.integers(0, 256))
                d[r * ROW:(r + 1) * ROW] = _others(rng, ROW, x)
                d[r * ROW] = d[r * ROW + ROW - 1] = x
            d = d[:n]
        return d.astype(np.int64), {}
    return make


def _run_of_a_tile(offset):
    def make(rng, width):
        n, x = 4 * T[width], int(rng.integers(0, 256))
        d = _others(rng, n, x)
        d[T[width] + offset:2 * T[width] + offset] = x
        return d, {"x": x, "start": T[width] + offset}
    return make


def _partial_last_tile(r):
    def make(rng, width):
        n, x = 3 * T[width] + r, int(rng.integers(0, 256))
        d = _others(rng, n, x)
        d[3 * T[width]:] = x
        return d, {"x": x, "pairs": r}
    return make


def _first_and_last_tile(rng, width):
    n, x = 4 * T[width], int(rng.integers(0, 256))
    d = _others(rng, n, x)
    d[rng.choice(T[width], size=40, replace=False)] = x
    d[3 * T[width] + rng.choice(T[width], size=40, replace=False)] = x
    return d, {"x": x}


def _falling(rng, width):
    n = _n_default(width)
    return 255 - np.arange(n) * 256 // n, {}


def _stairs(run):
    def make(rng, width):
        n, r = _n_default(width), T[width] if run == "T" else run
        return (255 - np.arange(n) // r) % 256, {"run": r}
    return make


def _pass_family(family, variant, make, above="few", passes=None):
    for width in WIDTHS:
        for j in (range(len(SHIFTS[width])) if passes is None else passes):
            def build(rng, width=width, j=j):
                d, meta = make(rng, width)
                return pass_keys(rng, width, j, d, above), FLAGS[width], dict(meta, j=j, variant=variant)
            _add("%s/%s/%d/pass %d" % (family, variant, width, j), family, width, build)


_pass_family("one_digit", "one pass", _one_digit)
_pass_family("one_digit", "all passes", _one_digit, above="const", passes=(0,))
for _w in ("alternating", "0 then 255", "255 then 0"):
    _pass_family("ends", _w, _ends(_w))
for _w in "abcd":
    _pass_family("rows", _w, _rows(_w))
for _o in (-1, 0, 1):
    _pass_family("tile_runs", "a tile's worth at %+d" % _o, _run_of_a_tile(_o))
for _r in TAILS:
    _pass_family("tile_runs", "only in a last tile of %d" % _r, _partial_last_tile(_r))
_pass_family("tile_runs", "first and last tile only", _first_and_last_tile)
_pass_family("descending", "falling", _falling)
for _r in STAIRS:
    _pass_family("descending", "stairs of %s" % _r, _stairs(_r))


def _chain_random(width):
    def build(rng):
        n = CHAIN_TILES * T[width]
        return random_low(rng, n, width, KEY_BITS[width]), CHAIN_FLAGS, {"variant": "random"}
    return build


def _chain_one_digit(width, j):
    def build(rng):
        n = CHAIN_TILES * T[width]
        d = np.full(n, int(rng.integers(0, 256)), dtype=np.int64)
        return pass_keys(rng, width, j, d), CHAIN_FLAGS, {"variant": "one digit", "j": j}
    return build


for _wd in WIDTHS:
    _add("chain/random/%d" % _wd, "chain", _wd, _chain_random(_wd), large=True)
    for _j in range(len(SHIFTS[_wd])):
        _add("chain/one digit/%d/pass %d" % (_wd, _j), "chain", _wd, _chain_one_digit(_wd, _j), large=True)


# ---- bucket families: from the passes' output backwards ------------------------------------------------------------------------
def filler(rng, total):
    """bucket sizes 1 .. 5 that add up to `total`"""
    sizes = []
    while total > 0:
        m = min(int(rng.integers(1, 6)), total)
        sizes.append(m)
        total -= m
    return sizes


def plain(sizes):
    return [(m, None, False) for m in sizes]


def make_batch(rng, buckets, width, low_bits):
    """buckets: (members, low parts or None, neighbour) in the order of the passes' output.  Top bits ascend by an even step from
    an even start; a `neighbour` bucket's top bits are its predecessor's + 1, so the two differ in the lowest top bit only.  The
    low parts are keys of the batch's width with nothing set at `low_bits` and above.  -> keys, and the start and size of
    every bucket after the passes."""
    sizes = np.asarray([m for m, _, _ in buckets], dtype=np.int64)
    starts = np.cumsum(sizes) - sizes
    steps, tops, top = rng.integers(0, 500, size=sizes.shape[0]), [], 2
    for (m, lows, neighbour), s in zip(buckets, steps):
        top = top + 1 if neighbour else (top | 1) + 3 + 2 * int(s)
        tops.append(top)
    assert top < 1 << 32
    drawn = np.repeat(np.asarray([lows is None for _, lows, _ in buckets]), sizes)
    keys = zeros(int(sizes.sum()), width)
    keys[drawn] = mixed_low(rng, int(drawn.sum()), width, low_bits)
    for (m, lows, _), at in zip(buckets, starts):
        if lows is not None:
            assert lows.shape[0] == m and lows.dtype == keys.dtype
            keys[at:at + m] = lows
    assert not formats.key_shr(keys, low_bits).any() and (width == 64 or low_bits >= 64 or not keys["hi"].any())
    put(keys, low_bits, np.repeat(np.asarray(tops, dtype=np.uint64), sizes))
    label = np.repeat(np.arange(sizes.shape[0]), sizes)
    rng.shuffle(label)                                   # which bucket sits at each place of the batch ...
    q = np.empty_like(keys)
    q[np.argsort(label, kind="stable")] = keys           # ... its members in their order
    return q, starts, sizes


def _bucket_case(family, variant, width, low_bits, layout, flags=None, large=False):
    """layout(rng) -> (buckets, meta)"""
    def build(rng):
        buckets, meta = layout(rng)
        q, starts, sizes = make_batch(rng, buckets, width, low_bits)
        return q, flags or FLAGS[width], dict(meta, variant=variant, low_bits=low_bits, starts=starts, sizes=sizes)
    _add("%s/%s/%d/low %d" % (family, variant, width, low_bits), family, width, build, large)


def wide(hi, lo):
    k = np.zeros(np.broadcast(hi, lo).shape[0], dtype=KEY128_DTYPE)
    k["hi"], k["lo"] = hi, lo
    return k


def patterns(m, low_bits):
    """The low parts of a 128-bit bucket's m members, in input order, by name: what only a right 128-bit compare orders."""
    u, d = np.uint64, np.arange(m, dtype=np.uint64)
    hb = low_bits - 64                                                  # low bits that lie in `hi`
    flip = (d * u(7) // u(3)) & u(1)                                    # 0 0 1 1 1 0 0 1 ...
    full = u((1 << hb) - 1)
    perm = np.random.default_rng(m).permutation(m).astype(np.uint64)
    return {
        "lo bit 0": wide(u(0x155), u(0x123456789ABCDE0) | flip),
        "lo bit 63": wide(u(0x155), u(0x123456789ABCDEF) | (flip << u(63))),      # needs an unsigned compare of `lo`
        "bit 64": wide(u(0x154) | flip, u(0xF23456789ABCDEF0)),
        "highest low bit": wide(u(0x55) | (flip << u(hb - 1)), u(0x8000000000000001)),
        "equal hi, lo descends": wide(u(0x1234), u(0xFFFFFFFFFFFFFFFF) - d * u(3)),
        "equal lo, hi descends": wide(full - d * u(3), u(0x8000000000000000)),
        "crossed": wide(perm, u(0xFFFFFFFFFFFFFFFF) - perm * u(0x10000000001)),      # hi ascends where lo descends: the order follows hi
        "extremes": wide(np.where(flip == 0, u(0), full), np.where(flip == 0, u(0), u(0xFFFFFFFFFFFFFFFF))),
        "equal": wide(u(0x5A5A5), np.full(m, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)),
    }


def _boundary_ends(m):
    e = {1, 2, m - 1, m}
    if m > RANK_HALO + 1:
        e |= {m - (RANK_HALO - 1), m - RANK_HALO, m - (RANK_HALO + 1), RANK_HALO - 1, RANK_HALO, RANK_HALO + 1}
    return sorted(x for x in e if 1 <= x <= m)


def _wide_bucket_families(low_bits):
    W, TILE, HALO = 128, RANK_TILE, RANK_HALO
    add = lambda variant, layout: _bucket_case("buckets128", variant, W, low_bits, layout)
    for n in BATCH_SIZES:
        add("batch of %d" % n, lambda rng, n=n: (plain(filler(rng, n)), {"n": n}))
    for m in (1, 2, 3, 4, 5, 7, 8, 9):
        def short(rng, m=m):
            buckets, at, want = [], 0, []
            for rep in range(20):
                for r in range(4):
                    for s in filler(rng, int(rng.integers(0, 9))):
                        buckets.append((s, None, False)); at += s
                    while at % 4 != r:
                        buckets.append((1, None, False)); at += 1
                    want.append((len(buckets), 4, r))
                    buckets.append((m, None, False)); at += m
            return buckets, {"m": m, "aligned": want}
        add("short buckets of %d at every alignment" % m, short)
    for m in (63, 64, 65, 127, 128, 129, 200):
        def longer(rng, m=m):
            buckets, at, want = [], 0, []
            for r in (0, 1, 2, 3, 31, 62, 63, 64, 65):
                for s in filler(rng, int(rng.integers(1, 40))):
                    buckets.append((s, None, False)); at += s
                while at % 64 != r % 64:
                    buckets.append((1, None, False)); at += 1
                want.append((len(buckets), 64, r % 64))
                buckets.append((m, None, False)); at += m
            return buckets + plain(filler(rng, 77)), {"m": m, "aligned": want}
        add("buckets of %d, longer than a row" % m, longer)
    for m in (LIMIT - 1, LIMIT, LIMIT + 1):
        for start in (37, TILE - 300, TILE + 100):
            add("bucket of %d at %d" % (m, start),
                lambda rng, m=m, start=start: (plain(filler(rng, start)) + [(m, None, False)] + plain(filler(rng, 450)), {"m": m, "at": [start]}))
    for m in (2, 5, 130, 300):
        for e in _boundary_ends(m):
            def over(rng, m=m, e=e):
                n = 3 * TILE + 5
                first, second = TILE + e - m, 2 * TILE + e - m
                buckets = plain(filler(rng, first)) + [(m, None, False)] + plain(filler(rng, second - first - m)) + [(m, None, False)]
                return buckets + plain(filler(rng, n - second - m)), {"m": m, "e": e, "at": [first, second], "n": n}
            add("bucket of %d ends %d behind a boundary" % (m, e), over)
    for m in (2, 5, 130, 300):
        for tail in (1, HALO, HALO + 1, TILE):
            def ends(rng, m=m, tail=tail):
                n = 2 * TILE + tail
                return [(m, None, False)] + plain(filler(rng, n - 2 * m)) + [(m, None, False)], {"m": m, "at": [0, n - m], "n": n}
            add("buckets of %d at both ends, tail %d" % (m, tail), ends)
    add("all singletons", lambda rng: (plain([1] * (2 * TILE + 77)), {"n": 2 * TILE + 77}))
    for n in (1000, 5000):
        add("one bucket of %d is the batch" % n, lambda rng, n=n: ([(n, None, False)], {"n": n, "m": n, "at": [0]}))
    for m in (1, 3, 8, 70):
        def neighbours(rng, m=m):
            buckets = []
            for r in range(4):
                low = mixed_low(rng, m, W, low_bits)
                buckets += plain(filler(rng, 13 + r)) + [(m, low, False), (m, low[::-1].copy(), True)]
            return buckets + plain(filler(rng, 50)), {"m": m, "neighbours": 4}
        add("neighbouring buckets of %d" % m, neighbours)
    for pattern in PATTERNS:
        def values(rng, pattern=pattern):
            buckets, at = [], 0
            for r, m in enumerate([2, 3, 4, 5, 6, 9, 16, 37, 64, 150, 11, 21]):
                for s in filler(rng, int(rng.integers(1, 30))):
                    buckets.append((s, None, False)); at += s
                while at % 4 != r % 4:
                    buckets.append((1, None, False)); at += 1
                buckets.append((m, patterns(m, low_bits)[pattern], False)); at += m
            buckets += plain(filler(rng, TILE - 20 - at)) + [(40, patterns(40, low_bits)[pattern], False)] + plain(filler(rng, 100))
            return buckets, {"pattern": pattern, "at": [TILE - 20], "m": 40}
        add("values: " + pattern, values)


_wide_bucket_families(LOW[128])
_wide_bucket_families(LOW_OTHER[128])


def _long_bucket_families(width):
    low_bits = LOW[width]
    add = lambda variant, layout, **kw: _bucket_case("long", variant, width, low_bits, layout, **kw)
    for m in LONG_SIZES:
        mid = 2 * RANK_TILE - m // 2
        add("%d at position 0" % m, lambda rng, m=m: ([(m, None, False)] + plain(filler(rng, 3000)), {"long": [m], "at": [0], "m": m}))
        add("%d over a tile boundary" % m,
            lambda rng, m=m, mid=mid: (plain(filler(rng, mid)) + [(m, None, False)] + plain(filler(rng, 1500)), {"long": [m], "at": [mid], "m": m}))
        add("%d ending at n" % m, lambda rng, m=m: (plain(filler(rng, 3000)) + [(m, None, False)], {"long": [m], "at": [3000], "m": m, "n": 3000 + m}))
    add("two side by side", lambda rng: (plain(filler(rng, 500)) + [(1500, None, False), (1300, None, True)] + plain(filler(rng, 500)),
                                         {"long": [1500, 1300], "neighbours": 1}))
    add("three with short ones between", lambda rng: (plain(filler(rng, 300)) + [(1100, None, False)] + plain(filler(rng, 40)) + [(3000, None, False)] +
                                                      plain(filler(rng, 7)) + [(LIMIT + 1, None, False)] + plain(filler(rng, 300)),
                                                      {"long": [1100, 3000, LIMIT + 1]}))
    if width == 64:
        for m in (BIG_LONGEST, BIG_LONGEST + 1):
            add("%d members" % m, lambda rng, m=m: (plain(filler(rng, 1500)) + [(m, None, False)] + plain(filler(rng, 1500)), {"long": [m], "at": [1500], "m": m}),
                flags=BIGGEST_FLAGS, large=True)


for _wd in WIDTHS:
    _long_bucket_families(_wd)
