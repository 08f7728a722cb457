"""The corpus of hand-made reads for the score stage (tests/score_corpus.py) is what it claims to be -- one assertion per family,
computed from the reference's records and the plain restatement of score_main_kernel's decisions, so that an edit of the
corpus or of a kernel constant cannot silently move a case off its edge --, its records survive encode and decode, the plain
replay of those records is the sequential oracle (score bits, countUnique, countAll), and the reads of the order family really
depend on the flush order.  No device here: tests/test_gpu_score_corpus.py feeds the same cases to kasa_batch_score.

Left out of the comparison with the oracle: score_corpus.NO_ORACLE (lists of 8190, 8191 and 8192 segments on 8200 taxa); the
replay remains their reference.  Every other case is compared under every window."""
import os
import re

import numpy as np
import pytest

from oracle import oracle
from tests import group_corpus as gc, score_corpus as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "kasa_amd", "csrc", "kasa_hip.hip")
REPLAY_H = os.path.join(ROOT, "kasa_amd", "csrc", "kasa_replay.h")
KS = (12, 25)


def _primary(name):
    c = sc.case(name)
    kh, kl = c.windows[0]
    return c, sc.ref(name, kh, kl), sc.facts(name, kh, kl), gc.rec_words(kh, kl)


def _matched(recs, f):
    return [i for i, p in enumerate(f.positions) if recs[p].d]


# ---- the constants ------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    """every restated constant, found by its name in kasa_hip.hip and kasa_replay.h"""
    src, rep = open(HIP).read(), open(REPLAY_H).read()

    def const(name, text=src):
        m = re.search(r"static constexpr (?:int|uint32_t) (?:\w+ = \w+, )*%s = ([^,;]+)[,;]" % name, text)
        assert m, name
        return eval(re.sub(r"(\d+)u", r"\1", m.group(1).strip()))

    for name in ("FTA", "RMAX", "EV_INV", "TLIST", "AGG", "PCAP_SMALL", "DENSE_TAXA", "DQ_SEGS", "SD_WAVES", "BM_WORDS"):
        assert const(name) == getattr(sc, name), name
    assert const("ESR_MIN_KMERS", rep) == sc.ESR_MIN_KMERS
    assert "constexpr uint32_t CNT_FIELDS = RW == 8 ? %du : %du;" % (sc.CNT_FIELDS[8], sc.CNT_FIELDS[16]) in src
    assert "constexpr uint32_t LN = 32u / (uint32_t)RW" in src and sc.LN == {8: 4, 16: 2}
    assert "if (cnt0 > (FB == 16 ? %du : %du))" % (sc.CNT_MAX[16], sc.CNT_MAX[8]) in src and "const bool fb8 = c->maxCnt <= %du" % sc.CNT_MAX[8] in src
    assert "if (live && Q.nseg >= (1u << %d))" % sc.NSEG_BITS in src
    assert "const int kPromote = (nK >= 3) ? A.kLow + 2 : A.kLow;" in src
    assert "base = atomicAdd(A.workCursor, %du);" % sc.TAKE in src
    assert "A.rowPerQuery = (nTaxa <= %du && !(c->debugFlags & 4)" % sc.ROW_PER_QUERY_TAXA in src and "? %du : 0u;" % sc.ROW_PER_QUERY in src
    assert "if ((unsigned long long)A.rowPerQuery * cnt0 >= 2ull * RMAX) rowCap" in src
    assert "R.clsLo[0] = %du; R.clsLo[1] = nTaxa <= %du ? %du : %du; R.clsLo[2] = (uint32_t)RMAX;" % (sc.CLS_LO[0], sc.NARROW_BITMAP_TAXA, sc.CLS_LO[1], sc.CLS_LO[0]) in src
    assert "nTaxa * 5u * SD_WAVES <= 160u * 1024u - 1024u" in src and sc.DENSE_LDS == 160 * 1024 - 1024
    assert "c->stCap = std::max<uint64_t>(1u << 16, (uint64_t)nReads * 8);" in src and sc.FIRST_STAGING == 1 << 16
    assert "R.bitmapMerge = nTaxa <= (uint32_t)BM_WORDS * 32u && !(c->debugFlags & 4);" in src
    assert "return (RW == 8 && pc <= 2u && !saturated) ? (pc ? 1u : 0u) : pc;" in src          # seg_records
    assert "fallback reasons: cnt=%u taxa=%u log=%u big=%u pending=%u" in src and len(sc.WHY) == 5


# ---- decoder and encoder ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.case_names())
def test_decode_reads_what_encode_writes(name):
    c = sc.case(name)
    for kh, kl in c.windows:
        recs, rw = sc.ref(name, kh, kl), gc.rec_words(kh, kl)
        rec, pool = gc.encode(recs, rw, kh, kl)
        assert rec.shape == (c.n, rw)
        for g, r in zip(gc.decode(rec, pool, rw, kh, kl), recs):
            assert g.fields(rw == 16) == r.fields(rw == 16), (name, kh, kl, r.p)


# ---- the replay against the sequential oracle ---------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sc.case_names() if n not in sc.NO_ORACLE])
def test_replay_is_the_sequential_oracle(name):
    c = sc.case(name)
    iv = oracle.IndexView(c.ix)
    qs, rd = c.sorted
    for kh, kl in c.windows:
        p = oracle.params(kh, kl, 3, K=c.letters)
        a, b = oracle.ranges(iv, p, qs)
        res = oracle.compare(iv, p, qs, rd, a, b, c.n_reads, True, closed_form=False)
        M, ca, cu = gc.replay(c, sc.ref(name, kh, kl), kh, kl)
        assert np.array_equal(M.view(np.uint32), res.M.view(np.uint32)), (name, kh, kl, "score bits", int(np.flatnonzero((M != res.M).any(axis=1))[0]))
        assert np.array_equal(cu, res.count_unique), (name, kh, kl, "countUnique")
        np.testing.assert_allclose(ca, res.count_all, rtol=1e-12, atol=0, err_msg="%s k %d..%d countAll" % (name, kh, kl))


# ---- take ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_take_batches_and_empty_reads(K):
    w = gc._w(K)
    assert [sc.case(n).n_reads for n in sc.case_names("take%d" % w) if "tail" not in n] == sc.TAKE_BATCHES
    for name in sc.case_names("take%d" % w):
        c, recs, facts, rw = _primary(name)
        empty = set(c.claim["empty"])
        assert len(facts) == c.n_reads == c.claim["reads"]
        for f in facts:
            assert (f.n == 0) == (f.read in empty), (name, f.read)
            assert f.why is None and (f.row == 0 if f.n == 0 else (len(f.regs) == 2 and f.n_other > 0)), (name, f.read, f.row)
        if c.n_reads >= 63:
            mid = c.n_reads // 2
            assert "tail" in name or ({0, mid - 1, mid + 1, c.n_reads - 1} == empty and facts[mid].row > 0)
    c = sc.case("take%d 129 tail" % w)
    assert c.claim["empty"] == list(range(65, 129))


# ---- phase --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_phase_every_length_at_every_phase(K):
    c, recs, facts, rw = _primary("phase%d" % gc._w(K))
    seen = set()
    for read, ph, n, m in c.claim["plan"]:
        f = facts[read]
        assert (f.first_slot % 4, f.n) == (ph, n) and _matched(recs, f) == [m] and f.why is None and f.row > 0, (read, ph, n, m, f.first_slot, f.n)
        for ln in (4, 2):
            first, last_line = ln - 1 - ph % ln, max(0, ((ph % ln + n - 1) // ln) * ln - ph % ln)      # (of the read's records; one line: its first)
            seen |= {(ln, ph % ln, n, what) for what, at in (("first", 0), ("last", n - 1), ("end of the first line", first), ("start of the last line", last_line)) if at == m}
    for ln in (4, 2):
        for ph in range(ln):
            for n in sc.PHASE_QUERIES:
                assert {(ln, ph, n, "first"), (ln, ph, n, "last")} <= seen
                assert (ln, ph, n, "end of the first line") in seen or ln - 1 - ph >= n
                assert (ln, ph, n, "start of the last line") in seen


# ---- slots --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_slots_reads_on_window_edges(K):
    c, recs, facts, rw = _primary("slots%d reads" % gc._w(K))
    f = facts[c.claim["ends at 63"]]
    assert (f.first_slot, f.n) == (0, 64) and _matched(recs, f) == [0, 63]
    f = facts[c.claim["begins at 64"]]
    assert f.first_slot == 64 and _matched(recs, f) == [0]
    f = facts[c.claim["straddles 127 | 128"]]
    assert f.first_slot < 127 and [f.first_slot + i for i in _matched(recs, f)] == [127, 128]
    f = facts[c.claim["four windows"]]
    assert f.n == 200 and (f.first_slot + f.n - 1) // sc.TAKE - f.first_slot // sc.TAKE >= 3 and len(_matched(recs, f)) == 5
    f = facts[c.claim["long"]]
    assert f.n == sc.SLOT_UNEQUAL[1] and sum(1 for x in facts if x.n == 1) == sc.SLOT_UNEQUAL[0] + sc.SLOT_UNEQUAL[2]
    # read_of_slot's proportional guess misses behind the long read
    rd = c.sorted[1]
    assert sum(1 for s in range(c.n) if min(int(s * (c.n_reads / c.n)), c.n_reads - 1) != rd[s]) > c.n // 2
    assert all(x.why is None for x in facts) and all(x.n_other > 0 for x in facts if x.row)


def _item_boundaries(facts, n):
    """where in a window's items a read begins: at the first item, at the last one, in between"""
    seen = set()
    for w in sc.window_items(facts, n, per_read=True):
        total, at = sum(i for _, i in w), 0
        for _, items in w:
            seen.add("first" if at == 0 else ("last" if at == total - 1 else "middle"))
            at += items
    return seen


def test_slots_item_totals_narrow():
    """items as score_other_flat_kernel counts them: the 64-bit case under its first window (narrow records)"""
    c, recs, facts, rw = _primary("slots64 items")
    assert rw == 8 and sorted({len(r.segs) - 2 for r in recs if r.d}) == sc.SLOT_LISTS == c.claim["lists"]
    assert sc.window_items(facts, c.n) == sc.SLOT_ITEMS == c.claim["items"]
    assert sorted({i for f in facts for i in f.items if i}) == sc.SLOT_LISTS
    assert _item_boundaries(facts, c.n) == {"first", "middle", "last"}
    assert all(f.why is None for f in facts)


@pytest.mark.parametrize("name", ["slots64 items wide", "slots128 items wide"])
def test_slots_item_totals_wide(name):
    """items as the second sweep of score_other_flat16_kernel counts them, under every window of the case (64-byte records on
    both key widths).  Where kLow is below seven the entry of the two-segment list takes the second register slot (kPromote <= 7)
    and the list yields no item: the windows built for 129 and 131 items hold 128 and 130 there."""
    c = sc.case(name)
    assert [w for w in c.windows if w[1] >= 7] or name.startswith("slots64")
    for kh, kl in c.windows:
        facts = sc.facts(name, kh, kl)
        assert gc.rec_words(kh, kl) == 16
        want = sc.SLOT_ITEMS if kl >= 7 else [63, 64, 65, 128, 128, 130]
        assert sc.window_items(facts, c.n) == want, (name, kh, kl, sc.window_items(facts, c.n))
        per_query = sorted({i for f in facts if f.items for i in f.items if i})
        assert per_query == (sc.SLOT_LISTS if kl >= 7 else sc.SLOT_LISTS[1:]), (name, kh, kl, per_query)
        assert _item_boundaries(facts, c.n) >= ({"first", "middle", "last"} if kl >= 7 else {"first", "middle"}), (name, kh, kl)
        assert all(f.why is None for f in facts if f.items and any(f.items))


# ---- register taxa ------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_register_taxa(K):
    c, recs, facts, rw = _primary("registers%d" % gc._w(K))
    kh, kl = c.windows[0]
    kp = sc.k_promote(kh, kl)
    assert kp == 9 and c.claim["reads"] == sc.REGISTER_READS and len(facts) == len(sc.REGISTER_READS)
    F = dict(zip(sc.REGISTER_READS, facts))
    Q = {label: [recs[p] for p in f.positions if recs[p].d] for label, f in F.items()}
    inl = gc.INL[rw]

    def inline(q):
        return [t for t, _, _ in (q.segs if len(q.segs) <= inl else q.segs[:inl - 1])]

    assert all(f.why is None for f in facts)
    f = F["none: depth kPromote - 1"]
    assert f.regs == () and max(q.d for q in Q["none: depth kPromote - 1"]) == kp - 1 and f.row == f.n_other > 0
    assert max(q.d for q in Q["depth kPromote"]) == kp and len(F["depth kPromote"].regs) == 2
    assert len(F["one taxon"].regs) == 1 and F["one taxon"].taxa == 1
    assert len(F["two taxa"].regs) == 2 and F["two taxa"].taxa == 2 and (rw == 16 or F["two taxa"].row == 2)
    assert len(F["four taxa"].regs) == 2 and F["four taxa"].taxa == 4 and all(kl_ >= kp for _, _, kl_ in Q["four taxa"][0].segs)
    q = Q["split first"][0]
    assert q.split and [t for t, _, _ in q.segs].count(F["split first"].regs[0]) == 3 and len(F["split first"].regs) == 2
    f, qs = F["second in a later query"], Q["second in a later query"]
    assert len(f.regs) == 2 and len(qs) == 2 and f.regs[1] not in [t for t, _, _ in qs[0].segs] and f.regs[1] in inline(qs[1])
    for label, sat, many in (("second in the pool", False, False), ("second in the pool, REC_SAT", True, False), ("second in the pool, 255 or more", True, True)):
        f, q = F[label], Q[label][0]
        assert len(f.regs) == 2 and len(Q[label]) == 1
        if rw == 8:
            assert f.regs[1] not in inline(q) and set(inline(q)) == {f.regs[0]} and q.sat == sat and (len(q.segs) >= gc.NSEG_CAP) == many, (label, q.sat, len(q.segs))
    f, qs = F["comes back shallow"], Q["comes back shallow"]
    assert len(f.regs) == 2 and any(t in f.regs and kl_ < kp for t, _, kl_ in qs[1].segs)
    f = F["shallow only"]
    assert f.regs == () and len(Q["shallow only"]) == 2 and f.row == f.n_other > 0


# ---- order --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sc.case_names("order") if n.endswith(("chunks", "pairs"))])
def test_order_reads_depend_on_the_flush_order(name):
    """EVERY read of the case with two or more matched queries -- found here from the reference, not from a list of the
    corpus's -- changes at least one score's bits when its events are replayed query by query instead of in flush order, its
    flush-order chain is the replay's row (which test_replay_is_the_sequential_oracle holds to the oracle), and it breaks the
    order rule.  These reads are the ones the corpus names, with the sizes it names: every size from 2 to 8, and nine in ten of
    the world's matched queries.  A read of one matched query cannot depend on the order across queries; the fast kernels keep it."""
    c, recs, facts, rw = _primary(name)
    kh, kl = c.windows[0]
    M, _, _ = gc.replay(c, recs, kh, kl)
    multi = {}
    for f in facts:
        n = len(_matched(recs, f))
        if n < 2:
            assert f.why is None and f.keeps_rule, (name, f.read)
            continue
        multi[f.read] = n
        ev = sc.read_events(c, recs, f.read)
        flush, by_pos = sc.chain(ev, False), sc.chain(ev, True)
        assert all(M[f.read, t].view(np.uint32) == flush[t].view(np.uint32) for t in flush), (name, f.read)
        assert any(flush[t].view(np.uint32) != by_pos[t].view(np.uint32) for t in flush), (name, f.read, "the same bits query by query")
        assert len({(k, len(taxa)) for _, k, _, taxa in ev}) > 1, (name, f.read, "its scores do not differ in k and |T|")
        assert f.why == 4 and not f.keeps_rule, (name, f.read)
    assert multi == c.claim["sizes"], name
    assert set(multi.values()) == set(sc.ORDER_SIZES), (name, sorted(set(multi.values())))
    assert 10 * sum(multi.values()) >= 9 * sum(1 for r in recs if r.d), (name, sum(multi.values()))


@pytest.mark.parametrize("K", KS)
def test_order_inside_one_query(K):
    """every query its own read: score_main_kernel keeps them all, and under every window of three levels or more some rows
    change their bits when a query's events are taken by level instead of in the record's order field: sums of a register
    taxon (score_main_kernel's chain) under each such window, sums of another taxon (the staging records' order, the row
    merge's chain) under at least one window of wide records"""
    name = "order%d order single" % gc._w(K)
    c = sc.case(name)
    others = {}                                    # by record width: reads with such a sum of another taxon, over the windows
    for kh, kl in c.windows:
        recs, facts = sc.ref(name, kh, kl), sc.facts(name, kh, kl)
        assert all(f.why is None and f.n == 1 for f in facts)
        if kh - kl < 2:
            continue
        reg = other = 0
        for f in facts:
            if f.row:
                a, b = sc.chain_by_query(recs, f.positions, kh, False), sc.chain_by_query(recs, f.positions, kh, True)
                diff = [t for t in a if a[t].view(np.uint32) != b[t].view(np.uint32)]
                reg, other = reg + any(t in f.regs for t in diff), other + any(t not in f.regs for t in diff)
        assert reg, (name, kh, kl)
        others[gc.rec_words(kh, kl)] = others.get(gc.rec_words(kh, kl), 0) + other
    assert others[16], others
    # narrow records: the other taxa of this world have too few events; a read built for it
    c, recs, facts, rw = _primary("order%d other" % gc._w(K))
    kh, kl = c.windows[0]
    for r in c.claim["reads"]:
        f = facts[r]
        a, b = sc.chain_by_query(recs, f.positions, kh, False), sc.chain_by_query(recs, f.positions, kh, True)
        q = recs[f.positions[1]]
        assert f.why is None and f.regs == (290, 291) and q.order == tuple(range(kh - kl + 1)) and q.sizes == tuple(range(1, kh - kl + 2)), (r, f.regs, q.order, q.sizes)
        assert a[1].view(np.uint32) != b[1].view(np.uint32), "taxon 1 of read %d: the same bits in level order" % r


@pytest.mark.parametrize("K", KS)
def test_order_F_up_down_tied_and_closers(K):
    w = gc._w(K)
    c, recs, facts, rw = _primary("order%d order chunks" % w)
    up = down = ties = 0
    for r in recs:
        steps = [b - a for a, b in zip(r.F, r.F[1:])]
        up, down, ties = up + any(s > 0 for s in steps), down + any(s < 0 for s in steps), ties + any(s == 0 for s in steps)
    assert up and down and ties
    rd = c.sorted[1]
    same = other = nowhere = 0
    for name in ("order%d order chunks" % w, "order%d order pairs" % w, "order%d split chunks" % w, "order%d split pairs" % w):
        c, recs, facts, rw = _primary(name)
        rd = c.sorted[1]
        n = (0, 0, 0)
        for r in recs:
            for F in r.F:
                n = (n[0] + (F < c.n and rd[F] == rd[r.p]), n[1] + (F < c.n and rd[F] != rd[r.p]), n[2] + (F == c.n))
        assert n[0] and n[1], (name, n)
        same, other, nowhere = same + n[0], other + n[1], nowhere + n[2]
    assert same and other and nowhere
    c, recs, facts, rw = _primary("order%d split chunks" % w)
    twice = sum(1 for r in recs if len({t for t, _, _ in r.segs}) < len(r.segs))
    again = sum(1 for f in facts if len(_matched(recs, f)) >= 2 and len({t for p in f.positions for t, _, _ in recs[p].segs}) < sum(len({t for t, _, _ in recs[p].segs}) for p in f.positions))
    assert twice and again


def test_order_segment_and_event_records():
    """narrow records (the 64-bit cases; 64-byte records leave an event record per level whatever the shape): among the segments of
    OTHER taxa -- outside the read's register taxa -- in reads score_main_kernel KEEPS, where seg_records decides: one level; two
    levels in ascending and in descending flush order (RK_SEG_DESC); three levels and more (event records); a REC_SPLIT query (one
    record per level); a segment with a level of seven or more taxa"""
    seen = set()
    for name in ["order64 order single", "order64 split single", "order64 other", "sizes64", "registers64", "rows64 classes"]:
        c = sc.case(name)
        for kh, kl in c.windows:
            if gc.rec_words(kh, kl) != 8:
                continue
            recs = sc.ref(name, kh, kl)
            for f in sc.facts(name, kh, kl):
                if f.why is not None:
                    continue
                for r in (recs[p] for p in f.positions if recs[p].d):
                    for t, kf, k_last in r.segs:
                        if t in f.regs:
                            continue
                        n = k_last - kf + 1
                        if r.split:
                            seen.add("split")
                        else:
                            seen.add("%d level%s" % (min(n, 3), "s" if n > 1 else ""))
                            if n == 2:
                                seen.add("two levels, " + ("ascending" if r.order.index(kh - kf) < r.order.index(kh - k_last) else "descending"))
                        if any(r.sizes[kh - k] >= gc.SIZE_CAP for k in range(kf, k_last + 1)):
                            seen.add("seven taxa in a segment record" if n <= 2 and not r.split else "seven taxa in event records")
    assert seen >= {"1 level", "2 levels", "3 levels", "split", "two levels, ascending", "two levels, descending", "seven taxa in a segment record", "seven taxa in event records"}, seen


# ---- sizes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_sizes(K):
    c, recs, facts, rw = _primary("sizes%d" % gc._w(K))
    kh, kl = c.windows[0]
    for f, m in zip(facts, sc.SIZES):
        q = [recs[p] for p in f.positions if recs[p].d]
        assert len(q) == 1 and q[0].sizes[kh - 7] == q[0].sizes[kh - 8] == m and set(q[0].sizes[:kh - 8]) == {1}, (m, q[0].sizes)
    assert {sc.CNT_FIELDS[8], sc.CNT_FIELDS[8] + 1, sc.CNT_FIELDS[16], sc.CNT_FIELDS[16] + 1, 7, 8, sc.EV_INV - 1, sc.EV_INV, sc.EV_INV + 1, 254, 255, 256} <= set(sc.SIZES)
    for n in (255, 256):
        c, recs, facts, rw = _primary("sizes%d fb %d" % (gc._w(K), n))
        assert facts[0].n == n == c.claim["queries"] == len(_matched(recs, facts[0])) and facts[0].regs == (1,) and facts[0].why is None
        assert max(f.n for f in facts) == n and (n > sc.CNT_MAX[8]) == (n == 256)


def test_sizes_counter_bound():
    c, recs, facts, rw = _primary("sizes128 count")
    assert rw == 16 and [f.n for f in facts[:2]] == sc.COUNT_READS == [sc.CNT_MAX[16], sc.CNT_MAX[16] + 1] and [f.why for f in facts] == [None, 0, None]
    assert all(len(_matched(recs, f)) == 1 for f in facts) and sc.COUNT_READS[0] >= sc.ESR_MIN_KMERS


def test_sizes_thirteen_bits():
    c, recs, facts, rw = _primary("sizes64 big")
    assert [len(recs[f.positions[0]].segs) for f in facts] == sc.SIZES_BIG == [(1 << sc.NSEG_BITS) - 2, (1 << sc.NSEG_BITS) - 1, 1 << sc.NSEG_BITS]
    assert [f.why for f in facts] == [2, 2, 3] and c.ix.content.n_taxa == sc.BIG_TAXA > sc.ROW_PER_QUERY_TAXA


# ---- rule ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("long_rows", [False, True])
def test_rule_fmax_at_p_and_one_behind(K, long_rows):
    c, recs, facts, rw = _primary("rule%d%s" % (gc._w(K), " long rows" if long_rows else ""))
    for label, f in zip(sc.RULE_READS, facts):
        q = [recs[p] for p in f.positions if recs[p].d]
        gaps = [a.fmax - b.p for a, b in zip(q, q[1:])]
        at = 3 if label.endswith("last") else 0
        if label.startswith("kept"):
            assert all(g <= 0 for g in gaps) and gaps[at] == 0 and f.keeps_rule and f.why == (2 if long_rows else None), (label, gaps, f.why)
        else:
            assert gaps[at] == 1 and all(g <= 0 for i, g in enumerate(gaps) if i != at) and not f.keeps_rule and f.why == 4, (label, gaps, f.why)
        assert len(q) == 5 + (12 if long_rows else 0)
        assert not long_rows or f.need is None or f.need > sc.RMAX
    assert sc.why_counts(facts) == ((0, 0, 2, 0, 2) if long_rows else (0, 0, 0, 0, 2))


# ---- rows ---------------------------------------------------------------------------------------
def test_rows_lengths():
    c, recs, facts, rw = _primary("rows64 classes")
    assert [f.need for f in facts] == sc.ROW_LENGTHS == c.claim["rows"]
    assert [f.why for f in facts] == [None] * 8 + [2] and all(f.n < 256 for f in facts)
    assert sc.row_classes(facts, c.ix.content.n_taxa) == (2, 3, 3, 0)
    assert {b + d for b in sc.CLS_LO for d in (-1, 0, 1)} == set(sc.ROW_LENGTHS)
    c, recs, facts, rw = _primary("rows64 long")
    assert [(f.n, f.need) for f in facts] == sc.ROW_LONG
    assert [f.why for f in facts] == [2, 2, 2, None, None, 2] and sc.row_classes(facts, c.ix.content.n_taxa) == (0, 0, 0, 2)
    assert sc.row_cap(255, 302) == sc.RMAX and sc.row_cap(256, 302) == 2048 == 2 * sc.RMAX and sc.row_cap(256, 302, True) == sc.RMAX


@pytest.mark.parametrize("total", sc.ROW_BATCH)
def test_rows_staging_demand(total):
    c, recs, facts, rw = _primary("rows64 batch %d" % total)
    assert c.n_reads == sc.ROW_BATCH_READS and max(sc.FIRST_STAGING, 8 * c.n_reads) == sc.FIRST_STAGING
    assert sum(f.row for f in facts) == total and all(f.why is None for f in facts)
    assert sc.ROW_BATCH == [sc.FIRST_STAGING - 1, sc.FIRST_STAGING, sc.FIRST_STAGING + 1]


@pytest.mark.parametrize("total", sc.ROW_BATCH)
def test_rows_key_demand(total):
    """64-byte records: the batch's rows need `total` profile keys (a fresh context has room for as many as staging records)"""
    c, recs, facts, rw = _primary("rows64 keys %d" % total)
    assert rw == 16 and c.n_reads == sc.ROW_BATCH_READS and c.claim["keys"] == total
    assert sum(f.keys for f in facts) == total and all(f.why is None and f.n == 1 for f in facts)


# ---- taxa ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_taxa", sc.TAXA_ROWS)
def test_taxa_tables(n_taxa):
    c, recs, facts, rw = _primary("taxa64 %d" % n_taxa)
    assert c.ix.content.n_taxa == n_taxa
    used = {t for r in recs for t, _, _ in r.segs}
    assert max(used) == n_taxa - 1 and len(used) <= 20
    assert [(f.n if f.n >= 256 else 0, f.need) for f in facts] == sc.TAXA_BATCH
    long_rows = n_taxa <= sc.ROW_PER_QUERY_TAXA
    assert [f.why for f in facts] == [None, None, None, 2, None if long_rows else 2, None]
    assert sc.dense_runs(c, 12, 7, 0) == (n_taxa <= 8140)
    assert sc.TAXA_ROWS == [sc.NARROW_BITMAP_TAXA, sc.NARROW_BITMAP_TAXA + 1, sc.ROW_PER_QUERY_TAXA, sc.ROW_PER_QUERY_TAXA + 1, sc.DENSE_LDS // (5 * sc.SD_WAVES),
                            sc.DENSE_LDS // (5 * sc.SD_WAVES) + 1, sc.BM_WORDS * 32, sc.BM_WORDS * 32 + 1] and sc.DENSE_TAXA == sc.BM_WORDS * 32


# ---- dense, general -----------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_dense_reads(K):
    w = gc._w(K)
    for name in sc.case_names("dense%d" % w):
        c, recs, facts, rw = _primary(name)
        handed = [f for f in facts if f.why is not None]
        assert len(handed) == c.claim["handed"] and all(f.why == 2 and f.keeps_rule and f.need > sc.RMAX for f in handed), (name, [f.why for f in facts])
        assert len(handed) < len(facts)
    c, recs, facts, rw = _primary("dense%d lists" % w)
    assert {len(r.segs) for r in recs if r.d} >= set(sc.DENSE_LISTS)
    if K == 12:
        c, recs, facts, rw = _primary("dense64 split")
        q = recs[facts[0].positions[0]]
        at = [i for i, (t, _, _) in enumerate(q.segs) if t == 300]
        assert q.split and q.sat and len(at) == 2 and at[0] // 64 != at[1] // 64 and facts[0].why == 2
        assert {lv % 2 for lv, n in enumerate(q.sizes) if n >= gc.SIZE_CAP} == {0, 1}
    c, recs, facts, rw = _primary("dense%d queries" % w)
    assert [f.n for f in facts if f.why == 2] == [1, 2, 3]
    assert [sc.case("dense%d reads %d" % (w, n)).claim["handed"] for n in sc.DENSE_READS] == [sc.SD_WAVES - 3, sc.SD_WAVES - 1, sc.SD_WAVES, sc.SD_WAVES + 1]


@pytest.mark.parametrize("K", KS)
def test_general_taxa_and_segments(K):
    c, recs, facts, rw = _primary("general%d taxa" % gc._w(K))
    assert [f.taxa for f in facts] == sc.GENERAL_TAXA == [sc.TLIST - 1, sc.TLIST, sc.TLIST + 1] and sc.AGG == sc.TLIST
    c, recs, facts, rw = _primary("general%d segments" % gc._w(K))
    assert [len(recs[f.positions[0]].segs) for f in facts] == sc.GENERAL_SEGS == [sc.DQ_SEGS - 1, sc.DQ_SEGS, sc.DQ_SEGS + 1]
