"""The spilling index builder (kasa_amd/csrc/kasa_spill.h behind kasa_build_set_resident / finish_begin / slab / fetch_slab /
finish_end) through capi.Builder(max_resident_records=B): the runs go to host memory and the index is finished in key-range slabs.

Every add-only case of tests/build_corpus.py runs with B = the input records of its heaviest prefix (the tightest budget the plan
accepts) and with 4 B, against build_corpus's plain reference: k-mers, tax IDs, trie prefixes and counts, frequency rows, pairs_in,
bricks and records_out, all exact; the 18 cases of at least two bricks and eleven prefixes must show two slabs and two spilled
runs or more.  The two `tiny/long protein` cases hold 196 650 records with a prefix nearly each: at B they would take about a hundred
thousand slabs, minutes of launches -- they run at 4096 B and 16384 B instead (some dozens of slabs), everything else compared
alike.  The hand-made cases of tests/spill_corpus.py run through finish() + fetch() and through finish_slabs(): slab count, every
slab's records and trie entries and spill_stats() equal the corpus's restatement of the rule, the concatenation equals the
reference.  Refusals are checked by their text, and a tiny builder per key width and place of the runs is walked through every
state with every entry point called out of order (PROTOCOL: status and text).  A builder with budget 0 gives the same bytes and spill_stats() all zero.  The C++
host builds tests/golden/batches and tests/golden/pairs (--kH 25) in dozens of bricks under a budget of an eighth of the index:
the five files byte for byte."""
import ctypes as C
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from kasa_amd import build as hipbuild, capi, formats
from tests import build_corpus as bc, helpers, spill_corpus as sc
from tests.test_gpu_parity import _gpu_or_fail
from tests.test_spill_cpu import MANY_SLABS

pytestmark = pytest.mark.gpu

RAN = {}                                            # (case, multiple of the tightest budget) -> spill_stats()
LONG = 4096                                         # the long protein cases: this many times the budgets of the others


def _builder(c, budget):
    return capi.Builder(c.content.array(), c.K, c.frames, None, c.brick, 0, budget)


def _add_steps(b, c):
    for step in c.steps:
        seqs = step[1]
        off = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.int64)
        b.add(np.frombuffer(b"".join(seqs), dtype=np.uint8), off, np.asarray(step[2], dtype=np.uint32), protein=step[3])


def _split(rec, K):
    if K == 25:
        km = np.zeros(rec.shape[0], dtype=formats.KEY128_DTYPE)
        km["lo"], km["hi"] = rec["lo"], rec["hi"]
        return km, np.ascontiguousarray(rec["tax"])
    return np.ascontiguousarray(rec["kmer"]), np.ascontiguousarray(rec["tax"])


def _compare(c, e, got, stats):
    km, tid, tp, tc, freq = got
    wkm, wtid, wtp, wtc = bc.arrays(e, c.K)
    assert km.shape[0] == wkm.shape[0] and tp.shape[0] == wtp.shape[0], f"{c.name}: {km.shape[0]} records and {tp.shape[0]} trie entries, expected {wkm.shape[0]} and {wtp.shape[0]}"
    assert np.array_equal(km, wkm), f"{c.name}: k-mers differ"
    assert np.array_equal(tid, wtid), f"{c.name}: tax IDs differ"
    assert np.array_equal(tp, wtp), f"{c.name}: trie prefixes differ"
    assert np.array_equal(tc, wtc), f"{c.name}: trie counts differ"
    rows, vals = bc.freq_sparse(e.freq, c.K)
    assert freq.shape == (c.content.n_rows, c.K), c.name
    assert np.array_equal(freq[rows], vals), f"{c.name}: frequency rows differ"
    assert np.count_nonzero(freq.any(axis=1)) == rows.shape[0], f"{c.name}: frequency rows that must be zero are not"
    for key in ("pairs_in", "bricks", "records_out"):
        assert stats[key] == e.stats[key], f"{c.name}: {key} {stats[key]}, expected {e.stats[key]}"


def _run_finish(c, budget):
    """finish() + fetch(): (what fetch() returns, stats(), spill_stats())"""
    b = _builder(c, budget)
    try:
        _add_steps(b, c)
        n, m = b.finish()
        got = b.fetch()
        assert (n, m) == (got[0].shape[0], got[2].shape[0])
        return got, b.stats(), b.spill_stats()
    finally:
        b.close()


def _run_slabs(c, budget):
    """finish_slabs(): (the concatenation in fetch()'s form, [(records, trie entries)] per slab, stats(), spill_stats())"""
    b = _builder(c, budget)
    try:
        _add_steps(b, c)
        parts = list(b.finish_slabs())
        rec = np.concatenate([p[0] for p in parts])
        tp, tc = np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])
        assert (b.n_records, b.n_trie) == (rec.shape[0], tp.shape[0])
        km, tid = _split(rec, c.K)
        return (km, tid, tp, tc, b.fetch_freq()), [(p[0].shape[0], p[1].shape[0]) for p in parts], b.stats(), b.spill_stats()
    finally:
        b.close()


def _check_stats(c, sp, want):
    assert want.refusal is None
    got = (sp["runs_spilled"], sp["records_spilled"], sp["slabs"], sp["largest_slab_input"], sp["heaviest_prefix_input"])
    exp = (want.runs_spilled, want.records_spilled, len(want.slabs), want.largest, want.heaviest[1]) if want.spilled else (0, 0, 0, 0, 0)
    assert got == exp, f"{c.name}: spill_stats {got}, expected {exp}"


@pytest.mark.parametrize("multiple", [1, 4])
def test_add_only_cases_of_build_corpus(multiple):
    """every add-only case at `multiple` times its tightest budget; a case that differs is reported by name, the others still run"""
    _gpu_or_fail()
    failures = []
    names = sc.add_only_names()
    for name in names:
        c = bc.case(name)
        B = max(1, sc.heaviest_prefix(c)) * multiple * (LONG if "long protein" in name else 1)
        try:
            got, stats, sp = _run_finish(c, B)
            _compare(c, bc.expect(c), got, stats)
            _check_stats(c, sp, sc.spill(c, B))
            RAN[(name, multiple)] = sp
        except AssertionError as ex:
            failures.append(str(ex))
    assert not failures, "%d of %d cases differ:\n%s" % (len(failures), len(names), "\n".join(failures[:20]))


def test_every_add_only_case_ran_and_the_bricked_ones_took_slabs():
    names = sc.add_only_names()
    assert len(names) >= 90 and set(MANY_SLABS) <= set(names)
    assert set(RAN) == {(n, m) for n in names for m in (1, 4)}, "cases skipped"
    for n in MANY_SLABS:
        for m in (1, 4):
            assert RAN[(n, m)]["slabs"] >= 2 and RAN[(n, m)]["runs_spilled"] >= 2, (n, m, RAN[(n, m)])
    assert sum(1 for sp in RAN.values() if sp["slabs"] >= 2) >= 2 * len(MANY_SLABS)


@pytest.mark.parametrize("name", sc.case_names())
def test_spill_case(name):
    _gpu_or_fail()
    c = sc.case(name)
    B = c.claim["budget"]
    e, want = bc.reference(c), sc.spill(c, B)
    got, stats, sp = _run_finish(c, B)
    _compare(c, e, got, stats)
    _check_stats(c, sp, want)
    got, per_slab, stats, sp = _run_slabs(c, B)
    assert per_slab == [(s.records, s.trie) for s in want.slabs], f"{name}: slabs {per_slab}"
    _compare(c, e, got, stats)
    _check_stats(c, sp, want)
    assert sp["upload_us"] > 0 and sp["download_us"] > 0
    # budget 0: the in-core finish, the same bytes, nothing spilled -- through both finishes
    plain, pstats, psp = _run_finish(c, 0)
    _compare(c, e, plain, pstats)
    assert all(v == 0 for v in psp.values()) and pstats["merges"] == e.stats["merges"]
    for a, b in zip(plain, got):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    plain, per_slab, pstats, psp = _run_slabs(c, 0)
    assert per_slab == [(len(e.kmers), len(e.trie[0]))] and all(v == 0 for v in psp.values())
    for a, b in zip(plain, got):
        assert a.tobytes() == b.tobytes()


def _refusal(call, text):
    with pytest.raises(RuntimeError) as ex:
        call()
    assert " failed: " not in str(ex.value) and text in str(ex.value), str(ex.value)


@pytest.mark.parametrize("K", bc.KS)
def test_refusals(K):
    _gpu_or_fail()
    c = sc.case("tight/K%d" % K)
    want = sc.spill(c, c.claim["refused_budget"])
    assert want.refusal and str(c.claim["heaviest"][0]) in want.refusal
    # one record below the heaviest prefix: refused by finish() and by finish_begin(), naming prefix, count and budget
    for how in ("finish", "finish_begin"):
        b = _builder(c, c.claim["refused_budget"])
        try:
            _add_steps(b, c)
            _refusal(getattr(b, how), want.refusal)
        finally:
            b.close()
    # edits need the runs on the device
    b = _builder(c, 5)
    try:
        rec = bc.records_array([bc.urec(i, K) for i in range(4)], K)
        _refusal(lambda: b.add_index(rec), "edits need the runs on the device")
        _refusal(lambda: b.drop_taxa([11]), "edits need the runs on the device")
        _refusal(lambda: b.shrink(3), "edits need the runs on the device")
        _add_steps(b, c)
        _refusal(lambda: b.set_resident(7), "before the first kasa_build_add")
        # the slabs in order, each once
        _refusal(lambda: b.slab(0), "kasa_build_finish_begin first")
        _refusal(b.finish_end, "kasa_build_finish_begin first")
        n = b.finish_begin()
        assert n >= 2
        _refusal(lambda: b.slab(1), "slab 1 asked, slab 0 of %d is next" % n)
        _refusal(b.finish_end, "0 of %d slabs were taken" % n)
        b.slab(0)
        _refusal(lambda: b.slab(0), "slab 0 asked, slab 1 of %d is next" % n)
        _refusal(b.finish_begin, "called twice")
        _refusal(b.finish, "called twice")
        for i in range(1, n):
            b.slab(i)
        _refusal(lambda: b.slab(n), "slab %d asked" % n)
        b.finish_end()
        _refusal(b.finish_end, "called twice")
        _refusal(b.taxa_histogram, "spilled build")
        b.n_records, b.n_trie = 1, 1
        _refusal(b.fetch, "slab by slab")
        assert b.fetch_freq().any()
    finally:
        b.close()
    # after an edit call the budget is refused, and the builder finishes in core as before
    b = _builder(c, 0)
    try:
        b.drop_taxa([33])
        _refusal(lambda: b.set_resident(5), "edits need the runs on the device")
    finally:
        b.close()
    # taxa_histogram after a spilled finish()
    b = _builder(c, c.claim["budget"])
    try:
        _add_steps(b, c)
        b.finish()
        _refusal(b.taxa_histogram, "spilled build")
    finally:
        b.close()


# ---- calls out of order, in every state ------------------------------------------------------------------------------------------------
OK, E_STATE = 0, 4                                  # KASA_OK, KASA_E_STATE of include/kasa_hip.h
FINISHED, TWICE, BEGIN_FIRST, FINISH_FIRST = "the build is finished", "called twice", "kasa_build_finish_begin first", "kasa_build_finish first"
BEFORE_ADD, NO_SLAB, NEED_DEVICE = "before the first kasa_build_add", "no slab is current", "edits need the runs on the device"
BY_SLAB, END_FIRST, NOT_ON_DEVICE = "handed out slab by slab", "kasa_build_finish_end first", "spilled build are not on the device"
# What every entry point answers in every state: None = KASA_OK, a text = KASA_E_STATE with that text; {n} = the slabs.  The rows
# left out of a state are the calls that are in order there.  `slab` is asked for slab 7, which is never next.
AFTER_THE_FINISH = dict(add=FINISHED, add_index=FINISHED, drop_taxa=FINISHED, shrink=FINISHED, set_resident=BEFORE_ADD, finish=TWICE, finish_begin=TWICE)
DONE = dict(AFTER_THE_FINISH, slab=FINISHED, fetch_slab=NO_SLAB, finish_end=TWICE)
NOT_BEGUN = dict(set_resident=BEFORE_ADD, slab=BEGIN_FIRST, fetch_slab=NO_SLAB, finish_end=BEGIN_FIRST, fetch=FINISH_FIRST, fetch_range=FINISH_FIRST,
                 taxa_histogram=FINISH_FIRST)
ON_DEVICE = dict(fetch=None, fetch_range=None, taxa_histogram=None)
PROTOCOL = {
    # the runs on the device: one slab, made by finish_begin; records, trie and histogram are there from then on
    ("device", "adding"): dict(NOT_BEGUN, add=None, add_index=None, drop_taxa=None, shrink=None),
    ("device", "begun"): dict(AFTER_THE_FINISH, **ON_DEVICE, slab="slab 7 asked, slab 0 of 1 is next", fetch_slab=NO_SLAB, finish_end="0 of 1 slabs were taken"),
    ("device", "slab 0"): dict(AFTER_THE_FINISH, **ON_DEVICE, slab="slab 7 asked, slab 1 of 1 is next", fetch_slab=None),
    ("device", "ended"): dict(DONE, **ON_DEVICE),
    ("device", "finish"): dict(DONE, **ON_DEVICE),
    # the runs in host memory (a budget of one record)
    ("host", "adding"): dict(NOT_BEGUN, add=None, add_index=NEED_DEVICE, drop_taxa=NEED_DEVICE, shrink=NEED_DEVICE),
    ("host", "begun"): dict(AFTER_THE_FINISH, slab="slab 7 asked, slab 0 of {n} is next", fetch_slab=NO_SLAB, finish_end="0 of {n} slabs were taken",
                            fetch=END_FIRST, fetch_range=BY_SLAB, taxa_histogram=NOT_ON_DEVICE),
    ("host", "slab 0"): dict(AFTER_THE_FINISH, slab="slab 7 asked, slab 1 of {n} is next", fetch_slab=None, finish_end="1 of {n} slabs were taken",
                             fetch=END_FIRST, fetch_range=BY_SLAB, taxa_histogram=NOT_ON_DEVICE),
    ("host", "ended"): dict(DONE, fetch=BY_SLAB, fetch_range=BY_SLAB, taxa_histogram=NOT_ON_DEVICE),
    ("host", "finish"): dict(DONE, fetch=None, fetch_range=None, taxa_histogram=NOT_ON_DEVICE),
}
ENTRY_POINTS = ("add", "add_index", "drop_taxa", "shrink", "set_resident", "finish", "finish_begin", "slab", "fetch_slab", "finish_end", "fetch", "fetch_range",
                "taxa_histogram")


class _Tiny:
    """two amino-acid sequences whose windows share no 6-letter prefix, one brick; every entry point by name -> (status, message)"""
    TAXIDS = np.array([0, 11, 22, 33], dtype=np.uint32)
    SEQS = (b"ACDEFGHI", b"YWVTSRQP")

    def __init__(self, K, budget):
        self.b = capi.Builder(self.TAXIDS, K, 3, None, 0, 0, budget)
        self.bases = np.frombuffer(b"".join(self.SEQS), dtype=np.uint8)
        self.off = np.array([0, 8, 16], dtype=np.int64)
        self.tax = np.array([11, 22], dtype=np.uint32)
        self.drop = np.array([33], dtype=np.uint32)                   # (no record carries it)
        self.tp, self.tc = np.zeros(4096, dtype=np.uint32), np.zeros(4096, dtype=np.uint64)     # at most 16 trie entries
        self.freq = np.zeros((4, K), dtype=np.uint64)
        self.hist = np.zeros(5, dtype=np.uint64)
        self.n, self.m, self.d = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def call(self, name, slab=7):
        L, h, u64, p = capi.lib(), self.b.h, C.c_uint64, lambda a: a.ctypes.data_as(C.c_void_p)
        rc = {
            "add": lambda: L.kasa_build_add(h, p(self.bases), p(self.off), C.c_int64(2), p(self.tax), C.c_int(1)),
            "add_index": lambda: L.kasa_build_add_index(h, u64(0), u64(0), u64(0), None),
            "drop_taxa": lambda: L.kasa_build_drop_taxa(h, p(self.drop), u64(1)),
            "shrink": lambda: L.kasa_build_shrink(h, C.c_int(1), C.c_float(0)),       # (every n-th with percentage 0: no record goes)
            "set_resident": lambda: L.kasa_build_set_resident(h, u64(5)),
            "finish": lambda: L.kasa_build_finish(h, C.byref(self.n), C.byref(self.m)),
            "finish_begin": lambda: L.kasa_build_finish_begin(h, C.byref(self.n)),
            "slab": lambda: L.kasa_build_slab(h, u64(slab), C.byref(self.d), C.byref(self.m)),
            "fetch_slab": lambda: L.kasa_build_fetch_slab(h, u64(0), u64(0), None, p(self.tp), p(self.tc)),
            "finish_end": lambda: L.kasa_build_finish_end(h, C.byref(self.d), C.byref(self.m)),
            "fetch": lambda: L.kasa_build_fetch(h, None, p(self.tp), p(self.tc), p(self.freq)),
            "fetch_range": lambda: L.kasa_build_fetch_range(h, u64(0), u64(0), None),
            "taxa_histogram": lambda: L.kasa_build_taxa_histogram(h, p(self.hist), u64(5), C.byref(self.d)),
        }[name]()
        return rc, L.kasa_last_error().decode() if rc else ""

    def step(self, name, slab=7):
        rc, text = self.call(name, slab)
        assert rc == OK, f"{name}: {text}"

    def check(self, where, state):
        want = PROTOCOL[(where, state)]
        for name in ENTRY_POINTS:
            if name not in want:
                continue
            rc, text = self.call(name)
            exp = want[name]
            if exp is None:
                assert rc == OK, f"{where}, {state}: {name} refused: {text}"
            else:
                assert rc == E_STATE and exp.format(n=self.n.value) in text, f"{where}, {state}: {name} gave {rc} {text!r}, expected {exp!r}"
        return len(want)


@pytest.mark.parametrize("K", bc.KS)
@pytest.mark.parametrize("where,budget", [("device", 0), ("host", 1)])
def test_calls_out_of_order_in_every_state(where, budget, K):
    """One tiny builder walked through adding -> finish_begin -> slab(0) .. -> finish_end, a second one through finish: at every
    stage every entry point that is not the next step is called once and answers what PROTOCOL says, by status and by text."""
    _gpu_or_fail()
    assert all(set(ENTRY_POINTS) - set(PROTOCOL[(where, s)]) <= {"finish", "finish_begin", "slab", "finish_end"} for s in ("adding", "begun", "slab 0", "ended", "finish"))
    t = _Tiny(K, budget)
    try:
        t.step("add")
        assert t.check(where, "adding") == 11
        t.step("finish_begin")
        n = t.n.value
        assert n == (1 if where == "device" else 16)                 # (host: sixteen records, a prefix each, one to a slab)
        assert t.check(where, "begun") == 13
        t.step("slab", 0)
        assert t.check(where, "slab 0") == (12 if where == "device" else 13)
        for s in range(1, n):
            t.step("slab", s)
        t.step("finish_end")
        assert t.check(where, "ended") == 13
    finally:
        t.b.close()
    t = _Tiny(K, budget)
    try:
        t.step("add")
        t.step("finish")
        assert t.check(where, "finish") == 13
        assert (t.n.value, t.freq.any()) == (16, True)
    finally:
        t.b.close()


# ---- the C++ host ---------------------------------------------------------------------------------------------------------------------
SUFFIXES =("", "_trie", "_trie.txt", "_info.txt", "_f.txt")


def _read(path):
    if not os.path.exists(path) and os.path.exists(path + ".gz"):
        with gzip.open(path + ".gz", "rb") as f:
            return f.read()
    with open(path, "rb") as f:
        return f.read()


def _host_build(args, tmp_path, env):
    exe = hipbuild.build_host()
    return subprocess.run([exe, "build"] + args + ["-m", "4", "-n", "1", "-v"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                          cwd=str(tmp_path), env=dict(os.environ, **env))


@pytest.mark.parametrize("db,stem,extra", [("batches", "idx", []), ("pairs", "idx25", ["--kH", "25"])])
def test_cpp_build_under_a_budget(db, stem, extra, tmp_path):
    _gpu_or_fail()
    d = os.path.join(helpers.GOLDEN, db)
    content, fasta = os.path.join(d, "content.txt"), os.path.join(d, "db.fasta")
    if not os.path.exists(content):
        content = str(tmp_path / "content.txt")
        with gzip.open(os.path.join(d, "content.txt.gz"), "rb") as f, open(content, "wb") as g:
            shutil.copyfileobj(f, g)
    if not os.path.exists(fasta):
        fasta += ".gz"
    n = int(_read(os.path.join(d, stem + "_info.txt")).split()[0])
    r = _host_build(["-i", fasta, "-c", content, "-d", str(tmp_path / "n")] + extra, tmp_path, {"KASA_BUILD_BRICK_PAIRS": "1000", "KASA_BUILD_RESIDENT_RECORDS": str(n // 8)})
    assert r.returncode == 0, r.stdout + r.stderr
    for s in SUFFIXES:
        assert _read(str(tmp_path / "n") + s) == _read(os.path.join(d, stem) + s), s
    m = re.search(r"spilled runs (\d+), slabs (\d+), copy ms up (\S+) down (\S+)", r.stdout)
    assert m and int(m.group(1)) >= 2 and int(m.group(2)) > 1, r.stdout
    # a budget below the heaviest prefix: the library's message as the driver's error, and no _info.txt
    r = _host_build(["-i", fasta, "-c", content, "-d", str(tmp_path / "bad")] + extra, tmp_path, {"KASA_BUILD_BRICK_PAIRS": "1000", "KASA_BUILD_RESIDENT_RECORDS": "1"})
    assert r.returncode == 1 and re.search(r"ERROR: kasa_build_finish: prefix \d+ alone brings \d+ input records to a slab, the resident budget is 1 records", r.stderr), r.stderr
    assert not os.path.exists(str(tmp_path / "bad_info.txt")) and not os.path.exists(str(tmp_path / "bad"))
