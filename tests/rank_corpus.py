"""Hand-made score rows for the rank and text stages (kasa_batch_rank, kasa_batch_text): the inputs of
tests/test_rank_corpus_cpu.py (which checks that the corpus is what it claims) and tests/test_gpu_rank_corpus.py (which
feeds it to the device through kasa_batch_set_scores).  Pure numpy and kasa_amd/report.py: no device, no reference tree.

A case is one batch: a CSR of (taxon index, k-mer score) cells, the denominators of the relative score per read class
(rel = float64(score) / den, the IEEE division the kernels do), the perfect score per class, what a writer prints about a
read (specifier, length), the threshold and the values of -b (`beasts`) to run.  Mostly den = 1, so that rel = score and a
tie lies exactly where the layout puts it.

The constants below restate kasa_hip.hip's (RANK_FIRST, RANK_CAP, RANK_ROWS, the slab geometry of rank_kernel, the LDS
staging of text_write_kernel): the corpus is cut to their seams.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from kasa_amd import report

N_TAXA = 1100                   # entries of the content file (index 0 = non_unique, never in a row)
RANK_FIRST, RANK_CAP, RANK_ROWS = 12, 64, 256
SLAB_STRIDE = 4 * 256 * 32      # reads between two reads of one wavefront of rank_kernel
TEXT_LDS = 48 * 1024
COUNTS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1000]
ADVERSARY_N = [40, 64, 65, 128, 129, 256, 257, 300]
TEXT_BEASTS = [1, 2, 3, 12, 13, 64, 65, 100]
F32 = np.float32


def taxa():
    """(taxon ids, names) of the content: ids up to 2^32 - 1, names empty, short, long, with the separators of the formats."""
    ids = (np.arange(N_TAXA, dtype=np.uint64) * 7 + 10).astype(np.uint32)
    ids[0] = 0
    ids[5], ids[6], ids[7], ids[8] = 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 1
    ids[999], ids[1000] = 999999999, 1000000000
    names = []
    for t in range(N_TAXA):
        if t == 0:
            names.append("non_unique")
        elif t % 97 == 3 or t in (1, 2):
            names.append("")
        elif t % 89 == 7:
            names.append("semi;colon\tand \"quote\" " + "y" * (t % 40))
        else:
            names.append("T%d" % t)
    return ids, names


EMPTY_NAME_TAXA = [t for t in range(1, N_TAXA) if t % 97 == 3 or t in (1, 2)]


@dataclass
class Case:
    name: str
    off: np.ndarray                 # uint64[nReads + 1]
    tax: np.ndarray                 # uint32[nnz], strictly ascending within a row
    score: np.ndarray               # float32[nnz]
    den: np.ndarray                 # float64[nClasses, N_TAXA]
    rclass: np.ndarray              # uint32[nReads]
    best: np.ndarray                # float32[nClasses]
    names: list
    lengths: np.ndarray             # uint32[nReads]
    threshold: float = 0.0
    beasts: list = field(default_factory=lambda: list(TEXT_BEASTS))
    first_reads: list = field(default_factory=lambda: [0])
    formats: list = field(default_factory=lambda: ["json", "jsonl", "tsv", "kraken"])
    labels: dict = field(default_factory=dict)      # read -> what the row was made for (for the counts in the summary)
    staging: dict = field(default_factory=dict)     # text-staging cases: (format, first read) -> {group: (m, bytes)} as designed

    @property
    def n(self) -> int:
        return int(self.off.shape[0] - 1)


class _Rows:
    def __init__(self):
        self.off, self.tax, self.score, self.labels, self.names, self.lengths, self.rclass = [0], [], [], {}, [], [], []

    def add(self, tax, score, label=None, name=None, length=100, cls=0):
        tax = np.asarray(tax, dtype=np.uint32)
        score = np.asarray(score, dtype=np.float32)
        assert tax.shape == score.shape and (tax.shape[0] < 2 or (np.diff(tax.astype(np.int64)) > 0).all()) and (tax.shape[0] == 0 or (tax.min() >= 1 and tax.max() < N_TAXA))
        r = len(self.off) - 1
        self.tax.append(tax); self.score.append(score)
        self.off.append(self.off[-1] + tax.shape[0])
        if label is not None:
            self.labels[r] = label
        self.names.append(("r%d " % r) if name is None else name)
        self.lengths.append(length)
        self.rclass.append(cls)
        return r

    def case(self, name, den=None, best=None, **kw):
        den = np.ones((1, N_TAXA), dtype=np.float64) if den is None else np.asarray(den, dtype=np.float64)
        best = np.full(den.shape[0], 1500.0, dtype=np.float32) if best is None else np.asarray(best, dtype=np.float32)
        cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
        return Case(name, np.asarray(self.off, dtype=np.uint64), cat(self.tax, np.uint32), cat(self.score, np.float32), den,
                    np.asarray(self.rclass, dtype=np.uint32), best, self.names, np.asarray(self.lengths, dtype=np.uint32), labels=self.labels, **kw)


def _pick_taxa(rng, n):
    return np.sort(rng.choice(np.arange(1, N_TAXA), size=n, replace=False)).astype(np.uint32)


def _by_rank(rng, values_by_rank):
    """values_by_rank[k] = the value of the hit a stable descending sort puts at place k; spread over the taxa at random."""
    v = np.asarray(values_by_rank, dtype=np.float32)
    return v[rng.permutation(v.shape[0])]


def _tie_at(n, p, width):
    """n distinct descending values, except that the places p .. p + width - 1 (as far as there are that many) share one."""
    v = np.arange(n, 0, -1, dtype=np.float32) + F32(2000.0)      # (within 0.8 of the largest: all of them can be top hits)
    v[p:p + width] = v[p] if p < n else 0
    return v


def layouts(n):
    """name -> scores by taxon position (den = 1: the relative scores, too)."""
    rng = np.random.default_rng(1000 + n)
    i = np.arange(n)
    out = {
        "all equal": np.full(n, 3.0),
        "2 values": 1.0 + rng.integers(0, 2, n),
        "3 values": 1.0 + rng.integers(0, 3, n),
        "5 values": 10.0 + rng.integers(0, 5, n),
        "ascending": 1.0 + i,
        "descending": 1.0 + (n - 1 - i),
        "organ pipe": 1.0 + np.minimum(i, n - 1 - i),
        # fourteen distinct leaders, the rest tied: the tie is beyond the print for a small -b and inside it for a large one
        "tie beyond": _by_rank(rng, np.concatenate((3000.0 - np.arange(min(n, 14)), np.full(max(0, n - 14), 5.0)))),
        "tie across 12": _by_rank(rng, _tie_at(n, 10, 4)),
        "tie 11|12": _by_rank(rng, _tie_at(n, 11, 2)),
        "tie 12|13": _by_rank(rng, _tie_at(n, 12, 2)),
    }
    for b in (1, 2, 3, 12, 13, 64, 65):
        # the b-th distinct score is shared by three hits: a writer with -b = b prints the first of them only
        out["straddle %d" % b] = _by_rank(rng, _tie_at(n, b - 1, 3))
    return {k: np.asarray(v, dtype=np.float32) for k, v in out.items()}


def case_counts(organ_pipe=False):
    """Every hit count with every layout.  The organ pipes are a batch of their own: std::sort heap-sorts those of 300 and
    1000 hits, and a batch with a read left to the host gets no text from the device."""
    R = _Rows()
    rng = np.random.default_rng(3)
    for n in COUNTS:
        for lay, sc in layouts(n).items():
            if (lay == "organ pipe") != organ_pipe:
                continue
            R.add(_pick_taxa(np.random.default_rng(n * 31 + len(lay)), n), sc, label=("count", n, lay), length=[0, 10, 255, 256, 70000, 151][len(R.names) % 6])
        if organ_pipe:
            k = int(rng.integers(1, 12))
            R.add(_pick_taxa(rng, k), 1.0 + rng.integers(0, 50, k), label=("filler",))
            R.add(_pick_taxa(rng, k), 1.0 + rng.integers(0, 2, k), label=("filler",))
    return R.case("organ pipes" if organ_pipe else "counts", first_reads=[0, 7, (1 << 32) + 5])


def adversary(n, tie=1):
    """McIlroy's adversary against report._stdsort_order: relative scores on which libstdc++'s introsort uses up its
    2 log2(n) levels (values never compared stay `gas`: they tie at the low end).  tie = 2: neighbours tied in pairs."""
    gas = n - 1
    val = [gas] * n
    state = {"solid": 0, "cand": 0}

    def less(x, y):
        if val[x] == gas and val[y] == gas:
            z = x if x == state["cand"] else y
            val[z] = state["solid"]; state["solid"] += 1
        if val[x] == gas:
            state["cand"] = x
        elif val[y] == gas:
            state["cand"] = y
        return val[x] < val[y]
    report._stdsort_order(n, less)
    return np.asarray([F32(n - v // tie) for v in val], dtype=np.float32)


def case_adversary():
    """Rows on which std::sort leaves introsort; -b 1 prints one hit (the prefix-only sort finishes), -b 100 needs the whole
    sort.  320 plain reads around them keep such reads below 5 % of the batch."""
    R = _Rows()
    rng = np.random.default_rng(77)
    for n in ADVERSARY_N:
        for tie in (1, 2):
            for _ in range(10):
                k = int(rng.integers(1, 12))
                R.add(_pick_taxa(rng, k), 1.0 + rng.integers(0, 50, k), label=("filler",))
            R.add(np.arange(1, n + 1) * (1099 // n), adversary(n, tie), label=("adversary", n, tie))
    for _ in range(160):
        k = int(rng.integers(0, 30))
        R.add(_pick_taxa(rng, k), 1.0 + rng.integers(0, 4, k), label=("filler",))
    return R.case("adversary", beasts=[1, 100])


def _ulps(x, k):
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf) if k > 0 else F32(-np.inf))
    return x


def case_arith():
    """Three read classes with their own denominators and perfect scores: the 0.8f top-hit rule at its float neighbours with
    the largest k-mer score NOT on the first hit, equal relative scores from different k-mer scores, denominators of
    -inf / +inf / 0 / NaN, cells that are not hits (0, -1, NaN, -0.0) on both sides of 256, the contamination rule at its limit."""
    den = np.ones((3, N_TAXA), dtype=np.float64)
    den[1, 2::2] = 2.0                                              # class 1: even taxa count double
    den[2] = 1.0 + np.log2(np.arange(N_TAXA) % 13 + 2.0)           # class 2: thirteen different denominators
    den[0, 20], den[0, 21], den[0, 22], den[0, 23] = -np.inf, np.nan, np.inf, 0.0
    den[0, 30], den[0, 40], den[0, 41] = 0.001, 20.0, 0.5
    best = np.array([2.0, 1500.0, 97.5], dtype=np.float32)
    R = _Rows()
    # 0.8f: taxon 30 leads (rel 1000 x), taxon 40 holds the largest k-mer score at rel = score / 20, taxon 35 is the candidate
    for mx in (100.0, 3.0, 7.0, 0.3, 1e-3, 12345.0):
        for k in range(-2, 3):
            cand = _ulps(F32(0.8) * F32(mx), k)
            R.add([30, 35, 40, 41], [F32(mx) * F32(0.5), cand, F32(mx), F32(mx) * F32(1e-3)], label=("0.8f", float(mx), k), length=300, cls=0)
    # equal relative scores from different k-mer scores (2/2 and 1/1), among few and many hits
    rng = np.random.default_rng(9)
    for n in (2, 5, 16, 17, 40, 129, 300):
        t = _pick_taxa(rng, n)
        base = 1.0 + rng.integers(0, 3, n)
        R.add(t, np.where(t % 2 == 0, 2.0 * base, base), label=("rel tie, scores differ", n), length=151, cls=1)
        R.add(t, (1.0 + rng.integers(0, 6, n)) * 0.25, label=("thirteen denominators", n), length=40, cls=2)
    # special denominators: rel = -0.0 (kept at threshold 0, printed "0.0"), NaN (dropped), +0.0, inf
    R.add([20], [1.5], label=("den -inf",), cls=0)
    R.add([21], [1.5], label=("den nan",), cls=0)
    R.add([20, 21, 22, 23], [1.5, 2.5, 3.5, 4.5], label=("den specials",), cls=0)
    R.add([10, 20, 21, 22, 23, 50], [1.0, 1.5, 2.5, 3.5, 4.5, 0.25], label=("den specials",), cls=0)
    t = _pick_taxa(rng, 40)
    t = np.unique(np.concatenate((t, [20, 21, 22, 23]))).astype(np.uint32)
    R.add(t, 1.0 + rng.integers(0, 3, t.shape[0]), label=("den specials",), cls=0)
    # cells that are not hits: m != cnt
    for m, cnt in ((5, 0), (5, 2), (40, 16), (40, 17), (300, 255), (300, 256), (300, 257), (257, 256), (257, 64), (600, 300), (1000, 3)):
        t = _pick_taxa(rng, m)
        sc = (1.0 + rng.integers(0, 4, m)).astype(np.float32)
        dead = rng.permutation(m)[:m - cnt]
        sc[dead] = np.asarray([0.0, -1.0, np.nan, -0.0], dtype=np.float32)[np.arange(m - cnt) % 4]
        R.add(t, sc, label=("dead cells", m, cnt), cls=1)
    # --filter: (best - max score) / best < 0.5 in double, at the limit (class 0: best = 2) and around it
    for k in (-1, 0, 1):
        R.add([60, 61], [_ulps(1.0, k), 0.5], label=("error threshold", k), cls=0)
    return R.case("arith", den=den, best=best, beasts=[1, 2, 3, 13, 100], first_reads=[3])


THRESHOLD = float(F32(0.3))


def case_threshold():
    """rel >= thr at equality, one ulp below and above (score 1, denominators around 1 / thr), and with score = thr, den = 1."""
    den = np.ones((1, N_TAXA), dtype=np.float64)
    d = 1.0 / THRESHOLD
    steps = np.arange(-8, 9)
    for i, k in enumerate(steps):
        x = d
        for _ in range(abs(int(k))):
            x = np.nextafter(x, np.inf if k > 0 else -np.inf)
        den[0, 100 + i] = x
    R = _Rows()
    for i in range(steps.shape[0]):
        R.add([100 + i], [1.0], label=("threshold", int(steps[i])))
    R.add(100 + np.arange(steps.shape[0]), np.ones(steps.shape[0]), label=("threshold row",))
    R.add([7], [F32(0.3)], label=("threshold score",))
    R.add([7, 8, 9], [_ulps(0.3, -1), F32(0.3), _ulps(0.3, 1)], label=("threshold score",))
    rng = np.random.default_rng(4)
    for n in (17, 40, 300):                                         # many hits, a third of them below the threshold
        R.add(_pick_taxa(rng, n), rng.integers(1, 4, n) * F32(0.15), label=("threshold many", n))
    return R.case("threshold", den=den, threshold=0.3, beasts=[1, 3, 100])


def case_slab():
    """5 x 32 768 + 3 reads, empty but for those = 0, 1, 32 767 (mod 32 768): a wavefront of rank_kernel meets its second,
    third, ... read, and its fifth does not fit what is left of a slab of 256 entries."""
    n_reads = 5 * SLAB_STRIDE + 3
    rng = np.random.default_rng(12)
    off = np.zeros(n_reads + 1, dtype=np.uint64)
    tax, score, labels = [], [], {}
    for r in range(n_reads):
        if r % SLAB_STRIDE in (0, 1, SLAB_STRIDE - 1):
            n = 60 + (r % 4)
            tax.append(_pick_taxa(rng, n)); score.append(_by_rank(rng, 5000.0 - np.arange(n)))
            labels[r] = ("slab", r % SLAB_STRIDE)
            off[r + 1] = n
    off = np.cumsum(off, dtype=np.uint64)
    return Case("slab", off, np.concatenate(tax).astype(np.uint32), np.concatenate(score).astype(np.float32), np.ones((1, N_TAXA)),
                np.zeros(n_reads, dtype=np.uint32), np.array([6000.0], dtype=np.float32), [""] * n_reads, np.full(n_reads, 9, dtype=np.uint32),
                beasts=[100], labels=labels)


def _piece_len(fmt, number, length):
    """bytes of a read without hits and with an empty specifier"""
    w = report.ReadWriter(fmt, [""], [0], 3)
    return len(w.read(number, "", length, report.Ranked([], 0, F32(1.0))).encode("latin-1"))


def case_staging(fmt="jsonl", first_read=0):
    """Groups of 64 reads without hits whose bytes (in `fmt`, numbered from `first_read`), by the lengths of their
    specifiers, come to TEXT_LDS - m and TEXT_LDS - m + 1 for every misalignment m = 0 .. 15 of the group's first byte;
    a small group before each sets m.  A partial last group closes the batch."""
    names, plan, at = [], {}, 0

    def group(total):
        g = len(names) // 64
        fixed = sum(_piece_len(fmt, first_read + g * 64 + i, 100) for i in range(64))
        assert total >= fixed
        extra = total - fixed
        lens = [extra // 64 + (1 if i < extra % 64 else 0) for i in range(64)]
        names.extend("n" * k for k in lens)
        return g

    for m in range(16):
        for over in (0, 1):
            fixed = sum(_piece_len(fmt, first_read + (len(names) // 64) * 64 + i, 100) for i in range(64))
            pad = fixed + (m - (at + fixed)) % 16                   # the group before: ends where the next one starts at m (mod 16)
            group(pad); at += pad
            assert at % 16 == m
            total = TEXT_LDS - m + over
            g = group(total); at += total
            plan[g] = (m, total)
    names.extend(["tail"] * 7)
    n = len(names)
    return Case("staging " + fmt, np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32), np.ones((1, N_TAXA)),
                np.zeros(n, dtype=np.uint32), np.array([10.0], dtype=np.float32), names, np.full(n, 100, dtype=np.uint32),
                beasts=[3], first_reads=[first_read], staging={(fmt, first_read): plan})


def case_small_groups():
    """TSV prints nothing for a read whose one printed hit has an empty name: groups of 64 reads with 0 bytes, and with the
    11 .. 15 bytes of one read without hits (no format writes fewer about a read); one read alone beyond TEXT_LDS; the raw
    length byte of Kraken's unclassified line (0, 10, 255, 256, 70 000)."""
    R = _Rows()
    quiet = EMPTY_NAME_TAXA
    for g in range(9):                                              # (numbered from 0, the one line of group g has 11, 12, 13, 14, 15, 16, 17 bytes)
        for i in range(64):
            if g <= 6 and i == 5:
                R.add([], [], label=("small group", g), name="x" * max(0, g - 2), length=[0, 10, 255, 256, 70000, 65536 + 10, 1][g])
            elif g == 8 and i == 9:
                R.add([11, 12], [5.0, 4.0], label=("large read",), name="L" * (TEXT_LDS + 100), length=151)
            else:
                R.add([quiet[(g * 64 + i) % len(quiet)]], [2.0], label=("quiet",), name="q%d" % i, length=151)
    for L in (0, 10, 255, 256, 70000):
        R.add([], [], label=("length", L), length=L)
        R.add([30], [1.0], label=("length", L), length=L)
    return R.case("small groups", beasts=[1, 3], first_reads=[0, 100])


def cases():
    return [case_counts(), case_counts(organ_pipe=True), case_adversary(), case_arith(), case_threshold(), case_slab(), case_staging(), case_small_groups()]


# ---- what the reference does with a row, up to the sort ---------------------------------------------------------------------
def kept_hits(case: Case):
    """The hits Compare::scoringFunc keeps (Compare.hpp:1501-1522): score > 0 and rel = double(score) / den >= threshold.
    -> (off uint64[nReads + 1], tax, score, rel) of the kept cells, in row order."""
    thr = float(F32(case.threshold))
    row = np.repeat(np.arange(case.n), np.diff(case.off).astype(np.int64))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = case.score.astype(np.float64) / case.den[case.rclass[row], case.tax] if row.shape[0] else np.zeros(0)
        keep = (case.score > 0) & (rel >= thr) if row.shape[0] else np.zeros(0, dtype=bool)
    off = np.zeros(case.n + 1, dtype=np.uint64)
    np.add.at(off, row[keep] + 1, 1)
    return np.cumsum(off, dtype=np.uint64), case.tax[keep], case.score[keep], rel[keep]


def printed(scores_in_order, max_score, beasts: int):
    """How many leading hits some writer prints (Compare.hpp:1586-1594, 1623-1641, 1721-1754): the TSV list, and top hits +
    further hits of the other formats.  -> (hits of the TSV list, top hits, further hits)."""
    n = len(scores_in_order)
    if n == 0:
        return 0, 0, 0
    tsv, j, before = 0, 0, F32(0.0)
    while tsv < n and j < beasts:
        if before != scores_in_order[tsv]:
            before = scores_in_order[tsv]; j += 1
        tsv += 1
    top = 1
    mx = F32(max_score)
    while top < min(n, beasts) and F32(F32(scores_in_order[top]) / mx) > F32(0.8):
        top += 1
    i, j, before = top, top, F32(0.0)
    while i < n and j < beasts:
        if before != scores_in_order[i]:
            before = scores_in_order[i]; j += 1
        i += 1
    return tsv, top, i - top


def structured_numbers():
    """Values for the number format with structure instead of chance: the float32 neighbours (1 and 2 ulp to either side) of
    10^k, k = -10 .. 10, widened to double as the writers pass k-mer scores and errors; and, for each of 1 .. 16 fractional
    digits, 200 doubles that need that many: decimal strings of that many digits (the last one not 0), parsed."""
    vals = []
    for k in range(-10, 11):
        x = F32(10.0 ** k)
        lo = hi = x
        vals.append(float(x))
        for _ in range(2):
            lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
            vals += [float(lo), float(hi)]
    rs = np.random.default_rng(11)
    for digits in range(1, 17):
        for _ in range(200):
            frac = "".join(str(d) for d in rs.integers(0, 10, digits - 1)) + str(int(rs.integers(1, 10)))
            whole = int(rs.integers(0, 1000 if digits <= 12 else 10 if digits <= 15 else 1))
            vals.append(float("%d.%s" % (whole, frac)))
    return vals
