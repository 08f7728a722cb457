"""What the reference makes of a case of tests/rank_corpus.py: the hits it keeps (numpy), the order std::sort leaves them in
(tests/rank_reference.cpp, compiled here with g++ and run once per case), what the writers print of them (kasa_amd/report.py).
Shared by tests/test_rank_corpus_cpu.py and tests/test_gpu_rank_corpus.py; computed once per case and never changed."""
from __future__ import annotations

import os
import subprocess
import tempfile
from dataclasses import dataclass

import numpy as np

from kasa_amd import report
from tests import rank_corpus as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dir = None
_refs, _exps = {}, {}


def build_reference() -> str:
    """tests/rank_reference.cpp -> a program in a temporary directory of this process (as test_host_cpu.py builds stdsort_check)."""
    global _dir
    if _dir is None:
        _dir = tempfile.TemporaryDirectory(prefix="rank_reference_")
    exe = os.path.join(_dir.name, "rank_reference")
    if not os.path.exists(exe):
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "rank_reference.cpp")], check=True)
    return exe


def run_reference(off, tax, score, rel, need=rc.RANK_FIRST):
    """-> (order within each row, heap exit of the whole sort, give-up of the first-`need`-places sort, places that one made final)"""
    exe = build_reference()
    n_rows, nnz = off.shape[0] - 1, int(off[-1])
    with tempfile.TemporaryDirectory(prefix="rank_rows_") as d:
        with open(os.path.join(d, "in"), "wb") as f:
            f.write(np.uint64(n_rows).tobytes() + off.astype(np.uint64).tobytes() + tax.astype(np.uint32).tobytes()
                    + score.astype(np.float32).tobytes() + rel.astype(np.float64).tobytes())
        r = subprocess.run([exe, os.path.join(d, "in"), os.path.join(d, "out"), str(need)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        raw = open(os.path.join(d, "out"), "rb").read()
    assert len(raw) == nnz * 4 + n_rows * 6
    order = np.frombuffer(raw, dtype=np.uint32, count=nnz)
    heap = np.frombuffer(raw, dtype=np.uint8, count=n_rows, offset=nnz * 4).astype(bool)
    short = np.frombuffer(raw, dtype=np.uint8, count=n_rows, offset=nnz * 4 + n_rows).astype(bool)
    covered = np.frombuffer(raw[nnz * 4 + 2 * n_rows:], dtype=np.uint32, count=n_rows)
    return order, heap, short, covered


@dataclass
class Ref:
    off: np.ndarray         # uint64[nReads + 1] over the kept hits
    cnt: np.ndarray         # hits per read
    tax: np.ndarray         # the kept hits in std::sort's order, row after row
    score: np.ndarray
    rel: np.ndarray
    max_score: np.ndarray   # float32[nReads]: the largest k-mer score among a read's hits (0 without hits)
    heap: np.ndarray        # bool[nReads]: std::sort leaves introsort on this row (stdsort_order.h gives up)
    short: np.ndarray       # ... even when only the first RANK_FIRST places are asked for
    covered: np.ndarray     # places the RANK_FIRST-only sort makes final
    order: np.ndarray       # position within the row (taxon order) of the hit at each place


def reference(case: rc.Case) -> Ref:
    if case.name in _refs:
        return _refs[case.name]
    off, tax, score, rel = rc.kept_hits(case)
    order, heap, short, covered = run_reference(off, tax, score, rel)
    cnt = np.diff(off).astype(np.int64)
    at = np.repeat(off[:-1].astype(np.int64), cnt) + order.astype(np.int64)
    mx = np.zeros(case.n, dtype=np.float32)
    if tax.shape[0]:
        np.maximum.at(mx, np.repeat(np.arange(case.n), cnt), score)
    ref = Ref(off, cnt, tax[at], score[at], rel[at], mx, heap, short, covered.astype(np.int64), order)
    for a in (ref.tax, ref.score, ref.rel, ref.max_score, ref.cnt):
        a.setflags(write=False)
    _refs[case.name] = ref
    return ref


@dataclass
class Exp:
    n_tsv: np.ndarray       # hits of the TSV list
    n_top: np.ndarray       # top hits
    n_further: np.ndarray   # further hits
    n_print: np.ndarray     # the leading hits some writer prints = the entries of the read
    tie_inside: np.ndarray  # a printed hit shares its relative score with the hit behind it
    exact: np.ndarray       # std::sort's own order decides what is printed, or the read is beyond rank_kernel's tables
    whole: np.ndarray       # the print reaches beyond what the RANK_FIRST-only sort makes final
    flagged: np.ndarray     # ... and std::sort heap-sorts: the read stays the host's


def expected(case: rc.Case, beasts: int) -> Exp:
    key = (case.name, beasts)
    if key in _exps:
        return _exps[key]
    ref = reference(case)
    n = case.n
    z = lambda dt=np.int64: np.zeros(n, dtype=dt)
    e = Exp(z(), z(), z(), z(), z(bool), z(bool), z(bool), z(bool))
    for r in np.flatnonzero(ref.cnt > 0):
        lo, c = int(ref.off[r]), int(ref.cnt[r])
        tsv, top, further = rc.printed(ref.score[lo:lo + c], ref.max_score[r], beasts)
        p = max(tsv, top + further)
        e.n_tsv[r], e.n_top[r], e.n_further[r], e.n_print[r] = tsv, top, further, p
        k = min(p, c - 1)
        e.tie_inside[r] = bool(k > 0 and (ref.rel[lo:lo + k] == ref.rel[lo + 1:lo + k + 1]).any())
    e.exact[:] = (ref.cnt > rc.RANK_ROWS) | (e.n_print > rc.RANK_CAP) | ((ref.cnt > 16) & e.tie_inside)
    e.whole[:] = (e.n_print >= ref.covered) & (ref.covered < ref.cnt) & ~ref.short
    e.flagged[:] = e.exact & (ref.short | (e.whole & ref.heap))
    _exps[key] = e
    return e


def ranked(case: rc.Case, beasts: int, r: int) -> report.Ranked:
    """Read r as report.ReadWriter takes it: the hits a writer can print, the top-hit count of report.ranked_from_prefix, the
    perfect score of the read's class."""
    ref, e = reference(case), expected(case, beasts)
    best = np.float32(case.best[case.rclass[r]])
    if ref.cnt[r] == 0:
        return report.Ranked([], 0, best)
    lo, p = int(ref.off[r]), int(e.n_print[r])
    ent = [{"tax": ref.tax[lo + k], "score": ref.score[lo + k], "rel": ref.rel[lo + k]} for k in range(p)]
    rk = report.ranked_from_prefix(ent, ref.max_score[r], int(case.lengths[r]), 12, 7, 3, beasts)
    rk.best = best
    return rk


def pieces(case: rc.Case, beasts: int, fmt: str, first_read: int, taxids, names, coherence=None):
    """The bytes report.ReadWriter writes about every read of the case."""
    w = report.ReadWriter(fmt, names, taxids, beasts, coherence is not None)
    return [w.read(first_read + r, case.names[r], int(case.lengths[r]), ranked(case, beasts, r),
                   None if coherence is None else coherence[r]).encode("latin-1") for r in range(case.n)]
