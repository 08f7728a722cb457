"""The corpus of hand-made score rows (tests/rank_corpus.py) is what it claims to be, and its reference
(tests/rank_reference.cpp: std::sort itself) agrees with the Python restatement wherever that has an answer.  No device here:
tests/test_gpu_rank_corpus.py feeds the same cases to kasa_batch_rank and kasa_batch_text."""
import numpy as np
import pytest

from kasa_amd import report
from tests import rank_corpus as rc, rank_expect as rx


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in rc.cases()}


def _all_beasts(case):
    return sorted(set(case.beasts) | {0})


def test_reference_equals_python_stdsort_order(cases):
    """rank_reference's order = report._stdsort_order's on every row with more than 16 hits where that does not give up (up to
    16 std::sort is an insertion sort: stable); both give up on the same rows."""
    checked = gave_up = 0
    for name in ("counts", "organ pipes", "adversary", "arith", "threshold"):
        case = cases[name]
        ref = rx.reference(case)
        off, tax, score, rel = rc.kept_hits(case)
        for r in range(case.n):
            lo, c = int(off[r]), int(ref.cnt[r])
            rl = rel[lo:lo + c].tolist()
            got = ref.order[lo:lo + c].tolist()
            assert sorted(got) == list(range(c))
            assert all(rl[got[k]] >= rl[got[k + 1]] for k in range(c - 1))
            if c <= 16:
                assert got == sorted(range(c), key=lambda i: -rl[i]) and not ref.heap[r] and not ref.short[r]
                continue
            want = report._stdsort_order(c, lambda x, y: rl[x] > rl[y])
            assert (want is None) == bool(ref.heap[r]), (name, r)
            if want is None:
                gave_up += 1
            else:
                assert got == want, (name, r)
                checked += 1
    assert checked > 200 and gave_up >= 16


def test_counts_and_tie_layouts(cases):
    """Every hit count of the list, each with every layout; per format family a tie inside the print, on its edge (the last
    printed hit and the first one left out) and only beyond it, among more than 16 hits; prints beyond RANK_FIRST and
    RANK_CAP; a tie across the places 11 | 12 that is printed."""
    by_count = {}
    for case in (cases["counts"], cases["organ pipes"]):
        ref = rx.reference(case)
        for r, lab in case.labels.items():
            if lab[0] == "count":
                assert ref.cnt[r] == lab[1]
                by_count.setdefault(lab[1], set()).add(lab[2])
    case = cases["counts"]
    ref = rx.reference(case)
    assert sorted(by_count) == rc.COUNTS and all(len(v) == len(rc.layouts(3)) for v in by_count.values())
    assert {"all equal", "2 values", "3 values", "5 values", "ascending", "descending", "organ pipe", "tie beyond", "tie across 12"} <= by_count[300]
    seen = set()
    for beasts in case.beasts:
        e = rx.expected(case, beasts)
        for r in np.flatnonzero(ref.cnt > 16):
            lo, c = int(ref.off[r]), int(ref.cnt[r])
            tie = ref.rel[lo:lo + c - 1] == ref.rel[lo + 1:lo + c]             # tie[k]: the hits at places k and k + 1
            for family, n in (("tsv", int(e.n_tsv[r])), ("json", int(e.n_top[r] + e.n_further[r]))):
                if n == 0:
                    continue
                if tie[:n - 1].any():
                    seen.add((family, "inside"))
                if n < c and tie[n - 1]:
                    seen.add((family, "edge"))
                if not tie[:n].any() and tie[n:].any():
                    seen.add((family, "beyond"))
            if e.n_print[r] > rc.RANK_FIRST and e.exact[r]:
                seen.add("print over RANK_FIRST")
            if e.n_print[r] > rc.RANK_CAP:
                seen.add("print over RANK_CAP")
            if e.n_print[r] > rc.RANK_FIRST and tie[rc.RANK_FIRST - 1]:
                seen.add("tie across RANK_FIRST")
            if e.whole[r]:
                seen.add("whole sort")
            if e.exact[r] and not e.whole[r]:
                seen.add("first places suffice")
            for cl, (a, b) in enumerate(((17, 32), (33, 64), (65, 128), (129, 256), (257, 1 << 30))):
                if e.exact[r] and a <= c <= b:
                    seen.add(("exact class", cl))
    want = {(f, w) for f in ("tsv", "json") for w in ("inside", "edge", "beyond")} | {("exact class", k) for k in range(5)}
    want |= {"print over RANK_FIRST", "print over RANK_CAP", "tie across RANK_FIRST", "whole sort", "first places suffice"}
    assert want <= seen, want - seen


def test_heap_exit_reads(cases):
    """The adversarial rows are heap-exit rows, the first-places sort finishes on every one of them with -b 1, at least 8 reads
    of the corpus must stay flagged (the print needs the whole sort and std::sort leaves introsort there), and such reads are at
    most 5 % of any batch.  From the reference's output alone."""
    case = cases["adversary"]
    ref = rx.reference(case)
    adv = [r for r, lab in case.labels.items() if lab[0] == "adversary"]
    assert len(adv) == 2 * len(rc.ADVERSARY_N) and all(ref.heap[r] for r in adv) and not ref.short.any()
    assert sorted({(case.labels[r][1], case.labels[r][2]) for r in adv}) == sorted((n, t) for n in rc.ADVERSARY_N for t in (1, 2))
    assert not rx.expected(case, 1).flagged.any()
    total = 0
    for c in cases.values():
        for beasts in _all_beasts(c):
            e = rx.expected(c, beasts)
            k = int(e.flagged.sum())
            assert k * 20 <= c.n, (c.name, beasts, k)
            total += k
            assert not (rx.reference(c).short & (rx.reference(c).cnt > 0)).any()      # (so: flagged = whole sort needed and heap exit)
    assert total >= 8 and int(rx.expected(case, 100).flagged.sum()) >= 8


def test_selection_arithmetic(cases):
    case = cases["arith"]
    ref = rx.reference(case)
    assert set(case.rclass.tolist()) == {0, 1, 2} and len(set(case.best.tolist())) == 3
    e = rx.expected(case, 2)
    tops = {}
    for r, lab in case.labels.items():
        lo, c = int(ref.off[r]), int(ref.cnt[r])
        if lab[0] == "0.8f":
            assert c == 4 and ref.score[lo] != ref.max_score[r] and ref.tax[lo] == 30 and ref.tax[lo + 1] == 35      # the maximum is not on the first hit
            ratio = np.float32(ref.score[lo + 1]) / np.float32(ref.max_score[r])
            assert (e.n_top[r] == 2) == bool(ratio > np.float32(0.8))
            tops.setdefault(lab[1], set()).add((int(e.n_top[r]), bool(ratio == np.float32(0.8))))
        if lab[0] == "den -inf":
            assert c == 1 and ref.rel[lo] == 0.0 and np.signbit(ref.rel[lo])
        if lab[0] == "den nan":
            assert c == 0
        if lab[0] == "dead cells":
            assert c == lab[2] and int(case.off[r + 1] - case.off[r]) == lab[1]
        if lab[0] == "rel tie, scores differ" and c >= 16:
            same = (ref.rel[lo:lo + c - 1] == ref.rel[lo + 1:lo + c]) & (ref.score[lo:lo + c - 1] != ref.score[lo + 1:lo + c])
            assert same.any()
        if lab[0] == "error threshold":
            assert report.is_contaminant(case.best[0], ref.max_score[r]) == (lab[1] > 0)
    for mx, got in tops.items():
        assert {t for t, _ in got} == {1, 2}, mx                               # both sides of the limit
    assert any(eq for got in tops.values() for _, eq in got)                   # ... and the limit itself
    dead = [lab[1:] for lab in case.labels.values() if lab[0] == "dead cells"]
    assert any(c <= 256 < m for m, c in dead) and any(c > 256 for m, c in dead) and any(c == 256 for m, c in dead)
    # the threshold: rel == thr is a hit, one ulp below is none
    case = cases["threshold"]
    ref = rx.reference(case)
    thr = rc.THRESHOLD
    seen = set()
    for r, lab in case.labels.items():
        if lab[0] == "threshold":
            rel = 1.0 / case.den[0, int(case.tax[int(case.off[r])])]
            assert int(ref.cnt[r]) == (1 if rel >= thr else 0)
            seen.add("eq" if rel == thr else "below" if rel == np.nextafter(thr, -np.inf) else "above" if rel == np.nextafter(thr, np.inf) else "far")
    assert {"eq", "below", "above"} <= seen


def test_slab_case(cases):
    case = cases["slab"]
    assert case.n == 5 * rc.SLAB_STRIDE + 3
    ref, e = rx.reference(case), rx.expected(case, 100)
    rows = np.flatnonzero(ref.cnt > 0)
    assert rows.tolist() == [r for r in range(case.n) if r % rc.SLAB_STRIDE in (0, 1, rc.SLAB_STRIDE - 1)]
    assert ((e.n_print[rows] >= 55) & (e.n_print[rows] <= rc.RANK_CAP)).all() and not e.exact.any()
    for first in (0, 1):                                                       # the reads of one wavefront: four fit a slab, the fifth does not
        mine = e.n_print[first::rc.SLAB_STRIDE]
        assert mine.shape[0] == 6 and mine[:4].sum() <= 256 < mine[:5].sum()


def test_text_staging_sizes(cases):
    """Per misalignment m = 0 .. 15 a group of 64 reads whose text fills the LDS buffer exactly and one with a byte more;
    groups of 0 and of 11 .. 15 bytes; a partial last group; a read alone beyond the buffer.  Measured with report.ReadWriter."""
    taxids, names = rc.taxa()
    case = cases["staging jsonl"]
    (fmt, first), plan = next(iter(case.staging.items()))
    size = np.array([len(p) for p in rx.pieces(case, case.beasts[0], fmt, first, taxids, names)], dtype=np.int64)
    start = np.concatenate(([0], np.cumsum(size)))
    got = {(int(start[g * 64] % 16), int(start[g * 64 + 64] - start[g * 64])) for g in plan}
    assert got == {(m, rc.TEXT_LDS - m + over) for m in range(16) for over in (0, 1)}
    assert case.n % 64 != 0
    case = cases["small groups"]
    size = np.array([len(p) for p in rx.pieces(case, 1, "tsv", 0, taxids, names)], dtype=np.int64)
    groups = {int(size[g:g + 64].sum()) for g in range(0, 9 * 64, 64)}
    assert {0, 11, 12, 13, 14, 15} <= groups
    assert (size > rc.TEXT_LDS).sum() == 1
    assert {0, 10, 255, 256, 70000} <= set(case.lengths.tolist())
    assert int(taxids.max()) == 0xFFFFFFFF and "" in names


def test_structured_numbers():
    """1 .. 16 fractional digits each: textnum.dtoa prints that many for (nearly) every value of a class -- Grisu2 is not
    always the shortest, and of 16 significant digits one can be spare"""
    from kasa_amd import textnum
    vals = rc.structured_numbers()
    assert len(vals) == 21 * 5 + 16 * 200
    frac = [len(textnum.dtoa(v).split(".")[1]) for v in vals[21 * 5:]]
    for d in range(1, 17):
        assert sum(1 for f in frac[(d - 1) * 200:d * 200] if f == d) >= 190, d


def test_census(cases):
    """The numbers of the corpus (printed with -s): reads per case and -b, how many go to the exact kernel, need the whole
    sort, stay flagged."""
    total = flagged = 0
    if True:
        for c in cases.values():
            for beasts in _all_beasts(c):
                e = rx.expected(c, beasts)
                total += c.n
                flagged += int(e.flagged.sum())
                print("\ncorpus %-14s -b %3d: %6d reads, %4d with hits, %3d exact, %3d whole sort, %2d flagged" % (
                    c.name, beasts, c.n, int((rx.reference(c).cnt > 0).sum()), int(e.exact.sum()), int(e.whole.sum() if e.exact.any() else 0), int(e.flagged.sum())), end="")
        print("\ncorpus total: %d reads ranked, %d flagged" % (total, flagged))
    assert total > 0
