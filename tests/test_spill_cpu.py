"""CPU-only checks of the spilling index builder: the kasa_build_* symbols of the slab finish are declared, exported and bound;
every case of tests/spill_corpus.py holds what it claims against build_corpus's plain reference; and the slab plan's C++
(kasa_amd/csrc/kasa_spill_plan.h, compiled alone under AddressSanitizer + UBSan as tools/spill_plan_check, an ordinary child
process with nothing preloaded) prints the slabs and slices of the corpus's plain-loop restatement, for 64- and 128-bit keys."""
import os
import re
import subprocess

import pytest

from kasa_amd import build as hipbuild, capi, index_build
from tests import build_corpus as bc, spill_corpus as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kasa_build_set_resident", "kasa_build_finish_begin", "kasa_build_slab", "kasa_build_fetch_slab", "kasa_build_finish_end", "kasa_build_spill_stats"]
# the add-only cases of build_corpus with two bricks or more and eleven distinct prefixes or more: tests/test_gpu_spill.py
# asserts that these, at least, go through two slabs or more
MANY_SLABS = ["bricks/%s/K%d" % (w, K) for w in ("2", "3", "5", "7", "8", "9", "over by one", "single larger") for K in bc.KS] + \
             ["tiny/protein/alone/K%d" % K for K in bc.KS]


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "kasa_hip.h")).read()
    declared = set(re.findall(r"^int\s+(kasa_build_[a-z_]+)\(", header, re.M))
    assert set(SYMBOLS) <= declared
    L = capi.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert s in capi.EXPORTS
    for name in ("set_resident", "spill_stats", "finish_begin", "slab", "fetch_slab", "finish_end", "finish_slabs"):
        assert callable(getattr(capi.Builder, name))
    import inspect
    assert inspect.signature(capi.Builder.__init__).parameters["max_resident_records"].default == 0
    assert inspect.signature(index_build.build_index).parameters["max_resident_records"].default == 0
    # a builder is made of a device; without one the new calls refuse a NULL handle and no more
    assert L.kasa_build_set_resident(None, 5) != 0 and L.kasa_build_spill_stats(None, None) != 0
    # the kernels of the in-core finish are the slab's: the new header launches none of its own
    spill = open(os.path.join(ROOT, "kasa_amd", "csrc", "kasa_spill.h")).read()
    assert "__global__" not in spill and "<<<" not in spill
    assert "hip" not in open(os.path.join(ROOT, "kasa_amd", "csrc", "kasa_spill_plan.h")).read().replace("kasa_hip.hip", "")


def _check_partition(c, sp):
    """the slabs cut the reference's records and trie into consecutive pieces"""
    e = bc.reference(c)
    assert sum(s.records for s in sp.slabs) == len(e.kmers), c.name
    assert sum(s.trie for s in sp.slabs) == len(e.trie[0]), c.name
    at = 0
    for s in sp.slabs:
        keys = e.kmers[at:at + s.records]
        assert keys and sc.prefix_of(keys[0], c.K) == s.first and sc.prefix_of(keys[-1], c.K) == s.last, c.name
        assert s.input <= (c.claim.get("budget") or s.input) and s.records <= s.input
        at += s.records
    for a, b in zip(sp.slabs, sp.slabs[1:]):
        assert a.last < b.first
    assert sp.records_spilled == sum(s.input for s in sp.slabs)
    return e


@pytest.mark.parametrize("name", sc.case_names())
def test_case_holds_its_claim(name):
    c = sc.case(name)
    K, B = c.K, c.claim["budget"]
    runs = sc.runs_of(c)
    assert len(runs) == c.claim["runs"] == bc.reference(c).stats["bricks"]
    sp = sc.spill(c, B)
    assert sp.spilled and sp.refusal is None and sp.runs_spilled == len(runs) and len(sp.slabs) >= 2
    e = _check_partition(c, sp)
    records = list(zip(e.kmers, e.taxids))
    fed = [[r for r, (lo, hi) in enumerate(s.slices) if hi > lo] for s in sp.slabs]
    kind = name.split("/")[0]
    if kind == "adjacent":
        p = c.claim["p"]
        in_run = lambda q: [r for r, run in enumerate(runs) if any(sc.prefix_of(k, K) == q for k, _ in run)]
        assert in_run(p) == [0] and in_run(p + 1) == [1]
        assert (sp.slabs[0].first, sp.slabs[0].last, sp.slabs[0].input) == (p, p, 3) and sp.slabs[1].first == p + 1
    elif kind == "twins":
        assert sum(run.count((c.claim["twin"], 22)) for run in runs) == 3 and records.count((c.claim["twin"], 22)) == 1
        assert [run[-1] for run in runs] == [(c.claim["triple"], t) for t in (33, 22, 11)]
        assert [t for k, t in records if k == c.claim["triple"]] == [11, 22, 33]
        assert fed[0] == [0, 1, 2]
    elif kind == "extremes":
        assert sp.slabs[0].first == 0 and sp.slabs[-1].last == (1 << 30) - 1
        occur = sorted({sc.prefix_of(k, K) for k in e.kmers})         # nothing between [0, '^' x 5] and [31, '^' x 5]: the bisection crosses it
        assert max(b - a for a, b in zip(occur, occur[1:])) > 1 << 29
    elif kind == "gaps":
        assert [0] in fed and [1] in fed                                # a slab fed by one run alone (no merge): the other has no record in it
    elif kind == "alone":
        assert len(runs[0]) > B and all(f == [0] for f in fed)
    elif kind.startswith("odd tree"):
        n = c.claim["meet"]
        assert n % 2 == 1 and [len(f) for f in fed] == [n, n]
        assert sc.spill(c, B + 1).spilled is False                      # one record more and the builder keeps its runs
    elif kind == "tight":
        assert sp.heaviest == c.claim["heaviest"] and B == sp.heaviest[1]
        bad = sc.spill(c, c.claim["refused_budget"])
        assert bad.refusal == "prefix %d alone brings 3 input records to a slab, the resident budget is 2 records" % sp.heaviest[0]
    elif kind == "pads":
        inner = lambda k: any(bc.letter(k, j) == bc.PAD for j in range(K)) and any(bc.letter(k, j) != bc.PAD and any(bc.letter(k, i) == bc.PAD for i in range(j + 1, K)) for j in range(K))
        at, trailing_in, inner_in = 0, set(), set()
        for i, s in enumerate(sp.slabs):
            for k in e.kmers[at:at + s.records]:
                (inner_in if inner(k) else trailing_in).add(i)
            at += s.records
        assert inner_in and trailing_in - inner_in and inner_in - trailing_in


def test_the_cases_that_must_take_many_slabs():
    names = sc.add_only_names()
    assert set(MANY_SLABS) <= set(names) and len(MANY_SLABS) == 18
    for n in MANY_SLABS:
        c = bc.case(n)
        assert bc.reference(c).stats["bricks"] >= 2 and sc.distinct_prefixes(c) >= 11, n
        for B in (sc.heaviest_prefix(c), 4 * sc.heaviest_prefix(c)):
            sp = sc.spill(c, B)
            assert sp.spilled and sp.refusal is None and sp.runs_spilled >= 2 and len(sp.slabs) >= 2, (n, B)
            _check_partition(c, sp)


@pytest.fixture(scope="module")
def plan_check():
    return hipbuild.build_spill_plan_check()


def _budgets(c):
    h = sc.heaviest_prefix(c)
    return [b for b in {c.claim.get("budget"), c.claim.get("refused_budget"), h, 4 * h, max(h - 1, 1), 1 << 40} if b]


def test_plan_program_equals_the_restatement(plan_check, tmp_path):
    """every spill case and every add-only case of build_corpus, at its own budgets: the program under the sanitizers prints what
    the restatement derives -- heaviest prefix, slabs, slices per run, or the refusal"""
    cases = [sc.case(n) for n in sc.case_names()] + [bc.case(n) for n in sc.add_only_names() if "long protein" not in n]
    want, paths, ran = [], [], {12: 0, 25: 0}
    for i, c in enumerate(cases):
        runs = sc.runs_of(c)
        for B in _budgets(c):
            path = tmp_path / ("plan_%d_%d.txt" % (i, B))
            path.write_text(sc.plan_file(runs, B, c.K))
            paths.append(str(path))
            want.append((c.name, B, sc.plan_text(runs, B, c.K)))
            ran[c.K] += 1
    r = subprocess.run([plan_check] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.split("file ")[1:]
    assert len(got) == len(want)
    for g, path, (name, B, text) in zip(got, paths, want):
        assert g == path + "\n" + text, "%s budget %d" % (name, B)
    assert ran[12] == ran[25] and ran[12] > 100 and sum("refused" in t for _, _, t in want) > 10
