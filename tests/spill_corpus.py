"""Hand-made inputs for the spilling index builder (kasa_amd/csrc/kasa_spill.h and kasa_spill_plan.h behind
kasa_build_set_resident / finish_begin / slab / fetch_slab / finish_end), for 12- and 25-letter k-mers, with a plain restatement
of the slab rule.  No device code here: tests/test_spill_cpu.py shows that every case holds what it claims and holds the plan's
C++ (tools/spill_plan_check) to the restatement, tests/test_gpu_spill.py runs the cases through capi.Builder.

It reuses tests/build_corpus.py: a case is a bc.Case of "add" steps (amino-acid bytes give letter-exact k-mers: a sequence of L
letters yields its L suffixes, '^'-padded), bc.reference() is what the index must be.

runs_of(case) restates the brick rule of bc.reference(): the sorted unique (k-mer, tax ID) list of every brick.  spill(case,
budget) restates the rest with plain loops: the builder spills once the runs it holds sum to more records than the budget (every
later run follows); the plan is a Counter of input records per 6-letter prefix and a greedy walk over the prefixes in ascending
order -- a slab takes whole prefixes while its input records stay within the budget, at least one; a single prefix over the
budget is refused."""
import functools
from collections import Counter
from dataclasses import dataclass, field

from tests import build_corpus as bc

KS = bc.KS
PAD = bc.PAD


def prefix_of(key, K):
    return key >> (5 * (K - bc.TRIE_LETTERS))


def runs_of(case):
    """[(k-mer, tax ID)] sorted and unique per brick, in brick order; a brick whose k-mers all hold a '_' (DNA) is an empty run"""
    K = case.K
    runs, cur = [], set()
    staged, staged_protein = 0, None
    limit = case.brick or (1 << 62)
    for step in case.steps:
        assert step[0] == "add", "spilling builders take sequences only"
        _, seqs, taxids, protein = step
        for seq, t in zip(seqs, taxids):
            w = bc.protein_windows(seq, K) if protein else bc.dna_windows(seq, K, case.frames)
            if not w:
                continue
            if staged and (staged + len(w) > limit or staged_protein != protein):
                runs.append(sorted(cur))
                cur, staged = set(), 0
            staged_protein, staged = protein, staged + len(w)
            cur.update((k, t) for k in w if protein or not bc.has_illegal(k, K))
    if staged:
        runs.append(sorted(cur))
    return runs


@dataclass
class Slab:
    first: int                                      # prefixes, both occur
    last: int
    input: int                                      # the sum of the slices
    slices: list                                    # per run (lo, hi)
    records: int = 0                                # unique records out
    trie: int = 0                                   # trie entries = distinct prefixes


@dataclass
class Spill:
    spilled: bool
    runs_spilled: int = 0                           # runs that hold a record
    records_spilled: int = 0
    heaviest: tuple = (0, 0)                        # (prefix, input records), the first of the heaviest in ascending order
    slabs: list = field(default_factory=list)
    refusal: str = None

    @property
    def largest(self):
        return max((s.input for s in self.slabs), default=0)


def plan(runs, budget, K):
    """(heaviest, slabs, refusal) of the runs under the budget"""
    per_prefix = Counter()
    for run in runs:
        for k, _ in run:
            per_prefix[prefix_of(k, K)] += 1
    heaviest = (0, 0)
    for p in sorted(per_prefix):
        if per_prefix[p] > heaviest[1]:
            heaviest = (p, per_prefix[p])
    groups, cur, total = [], [], 0
    for p in sorted(per_prefix):
        c = per_prefix[p]
        if c > budget:
            return heaviest, _slabs(runs, groups, K), "prefix %d alone brings %d input records to a slab, the resident budget is %d records" % (p, c, budget)
        if cur and total + c > budget:
            groups.append(cur)
            cur, total = [], 0
        cur.append(p)
        total += c
    if cur:
        groups.append(cur)
    return heaviest, _slabs(runs, groups, K), None


def _slabs(runs, groups, K):
    out = []
    at = [0] * len(runs)
    for g in groups:
        inside = set(g)
        slices, union = [], set()
        for r, run in enumerate(runs):
            lo = at[r]
            hi = lo
            while hi < len(run) and prefix_of(run[hi][0], K) in inside:
                hi += 1
            union.update(run[lo:hi])
            slices.append((lo, hi))
            at[r] = hi
        out.append(Slab(g[0], g[-1], sum(h - l for l, h in slices), slices, len(union), len({prefix_of(k, K) for k, _ in union})))
    return out


def spill(case, budget):
    runs = runs_of(case)
    held, spilled = 0, False
    for run in runs:
        held += len(run)
        if held > budget:
            spilled = True
            break
    if not spilled:
        return Spill(False)
    heaviest, slabs, refusal = plan(runs, budget, case.K)
    return Spill(True, sum(1 for r in runs if r), sum(len(r) for r in runs), heaviest, slabs, refusal)


def heaviest_prefix(case):
    """the input records of the heaviest prefix: the tightest budget the case's plan accepts"""
    return plan(runs_of(case), 1 << 62, case.K)[0][1]


def distinct_prefixes(case):
    return len({prefix_of(k, case.K) for run in runs_of(case) for k, _ in run})


def plan_file(runs, budget, K):
    """the input of tools/spill_plan_check"""
    lines = ["%d %d %d" % (K, budget, len(runs))]
    for run in runs:
        lines.append(str(len(run)))
        lines.extend("%x" % k for k, _ in run)
    return "\n".join(lines) + "\n"


def plan_text(runs, budget, K):
    """what tools/spill_plan_check prints for that input"""
    heaviest, slabs, refusal = plan(runs, budget, K)
    lines = ["heaviest %d %d" % heaviest]
    if refusal:
        lines.append("refused " + refusal)
    else:
        for i, s in enumerate(slabs):
            lines.append("slab %d %d %d %d " % (i, s.first, s.last, s.input) + " ".join("%d:%d" % sl for sl in s.slices))
        lines.append("largest %d" % max((s.input for s in slabs), default=0))
    return "\n".join(lines) + "\n"


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
_MAKERS = {}
T3 = (11, 22, 33)


def _add(name, make):
    for K in KS:
        _MAKERS["%s/K%d" % (name, K)] = functools.partial(make, K)


def case_names():
    return list(_MAKERS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _MAKERS[name]()
    c.name, c.family = name, "spill"
    return c


def _case(K, seqs, tax, brick, **claim):
    return bc.Case("", "spill", K, bc.Content(bc.CONTENT3), [("add", [bc.prot(s) for s in seqs], list(tax), True)], brick=brick, claim=claim)


def _adjacent(K):
    """1. prefix p only in run A, p + 1 only in run B, three records each: budget 3 cuts exactly between them"""
    a, b = [5, 5, 5, 5, 5, 6], [5, 5, 5, 5, 5, 7]
    p = bc.kmer(a, 6)
    return _case(K, [a] * 3 + [b] * 3, T3 + T3, 18, budget=3, p=p, runs=2)


def _twins(K):
    """2. the pair ([8, 9], 22) in three runs is one record; [12] under 33, 22, 11 in three runs, the highest ID first, is three
    records in tax-ID order"""
    return _case(K, [[8, 9], [12]] * 3, (22, 33, 22, 22, 22, 11), 3, budget=6, runs=3, twin=bc.padded([8, 9], K), triple=bc.padded([12], K))


def _extremes(K):
    """3. prefix 0 (six letters 0) and prefix 2^30 - 1 (six letters 31: amino-acid input keeps '_'), empty prefix space between"""
    return _case(K, [[0] * 6, [31] * 6], (11, 22), 6, budget=4, runs=2)


def _gaps(K):
    """4. run A holds low prefixes only, run B high ones only: slabs fed by one run alone, the other has no record in them"""
    return _case(K, [[1, 2, 3, 4], [2, 2, 9], [20, 21, 22, 23], [21, 23, 23]], (11, 22, 33, 11), 7, budget=3, runs=2)


def _alone(K):
    """4. one spilled run alone, the budget below its length"""
    return _case(K, [[1, 2, 3, 4, 5, 6, 7, 8, 9, 10]], (22,), 0, budget=4, runs=1)


def _odd(n, K):
    """5. n runs that all meet in one slab: an odd merge tree.  Every run holds [3] and [4]; the budget 2n - 1 spills at the last
    run and leaves prefix [3] and prefix [4] a slab each, fed by all n runs"""
    return _case(K, [[3], [4]] * n, [T3[(i // 2) % 3] for i in range(2 * n)], 2, budget=2 * n - 1, runs=n, meet=n)


def _tight(K):
    """6. the heaviest prefix ([3] in three runs) brings 3 input records: budget 3 runs, budget 2 is refused"""
    return _case(K, [[3], [4, 6], [3], [5, 6], [3], [7, 8]], (22, 11, 22, 33, 22, 11), 3, budget=3, refused_budget=2, heaviest=(bc.kmer([3] + [PAD] * 5, 6), 3), runs=3)


def _pads(K):
    """7. records with trailing '^' in one slab and an inner '^' in another: the frequencies accumulate across the slabs"""
    return _case(K, [[2, 3], [2, 4], [25, PAD, 7], [25, PAD, 8, 9]], (11, 22, 33, 11), 4, budget=4, runs=3)


_add("adjacent", _adjacent)
_add("twins", _twins)
_add("extremes", _extremes)
_add("gaps", _gaps)
_add("alone", _alone)
_add("odd tree 3", functools.partial(_odd, 3))
_add("odd tree 5", functools.partial(_odd, 5))
_add("odd tree 21", functools.partial(_odd, 21))   # (more than 16 runs: the plan walks the prefixes with a heap)
_add("tight", _tight)
_add("pads", _pads)


# ---- the add-only cases of tests/build_corpus.py ---------------------------------------------------------------------------------------
def add_only_names():
    """the small cases of build_corpus whose steps are all "add": what a spilling builder accepts"""
    return [n for n in bc.case_names() if all(s[0] == "add" for s in bc.case(n).steps)]
