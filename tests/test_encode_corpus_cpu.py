"""The corpus of hand-made reads for the encoder (tests/encode_corpus.py) is what it claims to be: its plain reference equals
the oracle's encoder (keys and read ids, both key widths, both codon tables; the slots equal the order the oracle's stable sort
leaves inside a read; the counts equal ko_padded_len / ko_kmer_count), the constants it restates are those of kasa_hip.hip,
every case lands in the encoder form it names under the restated dispatch rule, and every family holds what it says -- one
assertion per claim, computed from the reference alone, so that an edit of the corpus or a retuned constant cannot silently
move a case off its edge.  No device here: tests/test_gpu_encode_corpus.py feeds the same cases to kasa_batch_encode."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle
from tests import encode_corpus as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "kasa_amd", "csrc", "kasa_hip.hip")
ALL = ec.case_names(large=True)


def ints(keys):
    return [ec.key_int(k) for k in keys]


def read_keys(name, r=0):
    """the keys of read r of a case, as Python integers"""
    e = ec.expected(name)
    a = int(e.read_count[:r].sum())
    return ints(e.keys[a:a + int(e.read_count[r])])


# ---- the constants ------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    """every restated constant, found by its name in kasa_hip.hip; the dispatch rule's lines as they stand there"""
    src = open(HIP).read()

    def const(name):
        m = re.search(r"static constexpr (?:int|uint32_t) %s = ([^,;]+);" % name, src)
        assert m, name
        return eval(m.group(1).strip())

    for name in ("ENC_CHUNK", "ENC_WAVES", "ENC_RANK_MAX", "ENC_LONG_MIN", "ENC_GROUP", "ENC_GROUP_RM"):
        assert const(name) == getattr(ec, name), name
    assert "constexpr int ROUNDS = (G * 136 + 63) / 64;" in src and "constexpr int CAPK = ROUNDS * 64;" in src
    assert ec.CAPK == ((ec.ENC_GROUP * 136 + 63) // 64) * 64 and ec.ENC_GROUP_RM <= ec.CAPK
    assert "const unsigned lblocks = 256 * 8;" in src and ec.LONG_BLOCKS == 256 * 8
    assert "for (int64_t w0 = longK ? waveId * chunk : 0; w0 < cnt; w0 += longK ? wavesTotal * chunk : chunk)" in src
    assert ec.LONG_SWEEP == ec.LONG_BLOCKS * ec.ENC_WAVES * ec.ENC_CHUNK
    assert "const int chunk = (mode == ENC_ONE) ? ENC_CHUNK / 3 : ENC_CHUNK;" in src and ec.ONE_CHUNK == ec.ENC_CHUNK // 3
    # the dispatch
    assert "const int rankSlots = (!c->haveSeqRead && c->maxCnt <= (uint32_t)ENC_RANK_MAX && !(c->debugFlags & 8)) ? 1 : 0;" in src
    assert "const uint64_t longMin = (!rankSlots && c->maxCnt >= ENC_LONG_MIN) ? (uint64_t)ENC_LONG_MIN : ~0ull;" in src
    assert "if (c->ix->wide && rankSlots && c->maxCnt <= %du)" % ec.SMALL_RM in src
    assert "else if (rankSlots && c->maxCnt <= (uint32_t)ENC_GROUP_RM && c->enc_mode() == ENC_DNA && c->strands() == 1) {" in src
    assert "} else if (rankSlots && c->maxCnt <= %du)" % ec.SMALL_RM in src
    assert "if (r < nSeq && seqOff[r + 1] - seqOff[r] >= longMin) list[atomicAdd(n, 1u)] = (uint32_t)r;" in src


def test_tables():
    """the built-in table restated is the oracle's; the telling table separates any two triples that differ in one position"""
    assert np.array_equal(ec.table("builtin"), oracle.codon_table())
    t = ec.table("telling")
    assert t.shape == (366,) and int(t.max()) < 32
    triples = [(a, b, c) for a in range(6) for b in range(6) for c in range(6)]
    for x in triples:
        for y in triples:
            if sum(p != q for p, q in zip(x, y)) == 1:
                assert t[x[0] * 64 + x[1] * 8 + x[2]] != t[y[0] * 64 + y[1] * 8 + y[2]], (x, y)
    built = ec.table("builtin")                            # (what the telling table is for: the built-in one does not)
    assert any(built[x[0] * 64 + x[1] * 8 + x[2]] == built[x[0] * 64 + x[1] * 8 + c] for x in triples for c in range(4) if c != x[2] and max(x) < 4)
    assert len(ec.REACHABLE) == 156 and len(ec.UNREACHABLE) == 60
    assert len(ec.codon_of_letter("telling")) == 32        # every letter value from bases alone


# ---- the reference against the oracle -----------------------------------------------------------
def oracle_encode(c, lut):
    bases, off = c.batch()
    p = oracle.params(c.k_high, c.k_low, ec.FRAMES[c.mode], K=c.K, protein=c.mode == "protein")
    km, rd = oracle.encode(bases[c.shift:], off - c.shift, p, np.array(ec.table(lut)))
    if c.seg_read is not None:
        rd = np.ascontiguousarray(np.asarray(c.seg_read, dtype=np.uint32)[rd])
    return km, rd


@pytest.mark.parametrize("name", ALL)
def test_reference_is_the_oracle(name):
    c = ec.case(name)
    for lut in (("telling", "builtin") if c.mode != "protein" and name not in ec.LARGE else (c.lut,)):
        e = ec.expected(c, lut)
        km, rd = oracle_encode(c, lut)
        assert e.keys.dtype == km.dtype and e.keys.shape == km.shape, (name, lut, e.keys.shape, km.shape)
        assert np.array_equal(e.keys, km), (name, lut, ec.describe_difference(c, e.keys, km))
        assert np.array_equal(e.read, rd), (name, lut)
        assert int(e.seq_count.sum()) == km.shape[0] == int(e.read_count.sum())
    if c.ranked:
        e = ec.expected(c)
        n = e.keys.shape[0]
        _, idx = oracle.sort_queries(e.keys, np.arange(n, dtype=np.uint32))           # stable; the payload is the emission index
        by_read = idx[np.argsort(e.read[idx], kind="stable")]                          # read-major, sorted within the read
        slot = np.zeros(n, dtype=np.uint32)
        slot[by_read] = np.arange(n, dtype=np.uint32)
        assert np.array_equal(e.slot, slot), name
        assert np.array_equal(np.sort(e.slot), np.arange(n, dtype=np.uint32))
    else:
        assert ec.expected(c).slot is None


@pytest.mark.parametrize("K,kh,kl", ec.GEOMETRIES)
@pytest.mark.parametrize("mode", ec.MODES)
def test_counts_are_the_oracles(K, kh, kl, mode):
    p = oracle.params(kh, kl, ec.FRAMES[mode], K=K, protein=mode == "protein")
    L = oracle.lib(K)
    for raw in range(0, 3 * K + 9):
        body, padded, cnt = ec.geometry(raw, K, kl, mode)
        lo = int(L.ko_padded_len(C.c_int64(raw), C.byref(p)))
        assert raw == 0 or padded == lo, (raw, padded, lo)
        assert cnt == (int(L.ko_kmer_count(C.c_int64(lo), C.byref(p))) if raw else 0), raw
        assert cnt == 0 or body == raw, "a padded read has a window"                   # padding never reaches a k-mer


# ---- the dispatch -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_case_lands_in_the_form_it_names(name):
    c, e = ec.case(name), ec.expected(name)
    assert c.form in ec.FORMS and c.why
    got = ec.dispatch(c.wide, c.mode, c.seg_read is not None, c.debug, e.seq_count, e.read_count)
    assert got == (c.form, int(c.ranked), c.second_launch), (name, got)
    assert c.k_high <= c.K and (c.K == 25) == c.wide


def test_every_form_is_reached_by_its_families():
    """group: DNA in three frames under 64-bit keys alone; the other four by both key widths; per family the forms the issue lists"""
    have = {(ec.case(n).family, ec.case(n).K, ec.case(n).form) for n in ALL}
    for fam in ("alphabet", "codons", "bounds"):
        for K in (12, 25):
            for form in ("slots192", "slots512", "readid"):
                assert (fam, K, form) in have, (fam, K, form)
        assert (fam, 12, "group") in have
    for K in (12, 25):
        assert ("alphabet", K, "long") in have and ("long", K, "long") in have and ("segments", K, "readid") in have
        assert ("geometry", K, "slots192") in have and ("packing", K, "slots192") in have
        assert ("ranking", K, "slots192") in have and ("ranking", K, "slots512") in have
    assert ("geometry", 12, "group") in have and ("ranking", 12, "group") in have and ("group_parts", 12, "group") in have
    def bare(n):                                                                          # the name without key width and form
        return " ".join(w for w in n.split() if w not in ec.FORMS and w not in ("K12", "K25")).replace("kLow12", "kLowK").replace("kLow25", "kLowK")

    for fam in ("alphabet", "codons", "geometry", "bounds"):                              # every 64-bit case of these has its 128-bit twin
        assert {bare(n) for n in ec.case_names(fam, K=12) if ".." not in n} <= {bare(n) for n in ec.case_names(fam, K=25)}, fam
    assert ec.GEOMETRIES == [(12, 12, 7), (12, 12, 12), (12, 12, 1), (25, 25, 7), (25, 25, 25)]      # (the length sweeps: these five windows)


# ---- alphabet -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in ec.case_names("alphabet") if "protein" not in n])
def test_alphabet_every_value_at_every_position(name):
    c, e = ec.case(name), ec.expected(name)
    inside = [set(), set(), set()]
    last = [set(), set(), set()]
    per = e.seq_count // ec.strands(c.mode)
    for s, cnt in zip(c.seqs[:c.claim["value_reads"]], per[:c.claim["value_reads"]]):
        assert cnt >= 3
        cnt, raw = int(cnt), s.shape[0]
        ws = 3 if c.mode == "one" else 1
        for p in range(raw):
            if p <= (cnt - 2) * ws + 3 * c.K - 1:
                inside[p % 3].add(int(s[p]))
            if p >= (cnt - 1) * ws:
                last[p % 3].add(int(s[p]))
    assert all(len(x) == 256 for x in inside) and all(len(x) == 256 for x in last)
    lower = [i for i, s in enumerate(c.seqs) if set(s.tolist()) <= set(b"acgt") and e.seq_count[i] > 0]
    none = [i for i, s in enumerate(c.seqs) if not set(s.tolist()) & set(b"ACGTacgt") and e.seq_count[i] > 0]
    assert lower and none
    first = int(e.seq_count[:none[0]].sum())
    assert ec.key_int(e.keys[first]) >> 5 * (c.K - 1) == int(ec.table(c.lut)[5 * 64 + 5 * 8 + 5])           # Z Z Z
    if c.form in ("readid", "long"):                                                      # the big read holds every value, too
        big = c.seqs[-1]
        assert all(len({int(v) for v in big[r::3]}) == 256 for r in range(3)) and e.seq_count[-1] == e.seq_count.max()


@pytest.mark.parametrize("name", [n for n in ec.case_names("alphabet") if "protein" in n])
def test_alphabet_protein(name):
    c, e = ec.case(name), ec.expected(name)
    seen = set()
    for s, n in zip(c.seqs, e.seq_count):
        if n:
            seen |= set(s.tolist())
    assert len(seen) == 256
    star = next(i for i, s in enumerate(c.seqs) if set(s.tolist()) == set(b"*[^"))
    ks = read_keys(name, star)
    assert ks and ks[0] >> 5 * (c.K - 3) == ((27 << 10) | (27 << 5) | 30)                 # '*' is '[' (27), '^' is 30
    assert any(set(s.tolist()) <= set(range(97, 123)) and n for s, n in zip(c.seqs, e.seq_count))


# ---- codons -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.case_names("codons"))
def test_codons_every_reachable_triple_at_every_letter(name):
    c, e = ec.case(name), ec.expected(name)
    n_str = ec.strands(c.mode)
    at = [[set() for _ in range(c.K)] for _ in range(n_str)]
    for s, n in zip(c.seqs, e.seq_count):
        cnt = int(n) // n_str
        if not cnt:
            continue
        for st, codes in enumerate(ec.strand_codes(s, c.K, c.k_low, c.mode)):
            t = codes[:-2] * 36 + codes[1:-1] * 6 + codes[2:]
            for j in range(c.K):
                at[st][j] |= set(t[3 * j:3 * j + cnt].tolist())
    plain = {a * 36 + b * 6 + d for a in ec.NON_X for b in ec.NON_X for d in ec.NON_X}
    marker = {a * 36 + b * 6 + d for a, b, d in ec.REACHABLE} - plain
    letters = {0, c.K // 2, c.K - 1} | ({11, 12, 13} if c.K == 25 else set())
    assert len(plain) == 125 and len(marker) == 31
    for st in range(n_str):
        for j in letters:
            assert plain <= at[st][j], (name, st, j, len(plain - at[st][j]))
        seen = set().union(*at[st])
        assert not seen & {a * 36 + b * 6 + d for a, b, d in ec.UNREACHABLE}, "a triple no input produces"
        if c.k_low < c.K:
            assert marker <= at[st][c.k_low], (name, st, sorted(marker - at[st][c.k_low]))
            assert seen == plain | marker
        else:
            assert seen == plain


# ---- geometry -----------------------------------------------------------------------------------
def test_geometry_lengths_and_empty_batches():
    for K, kh, kl in ec.GEOMETRIES:
        for mode in ec.MODES:
            c = ec.case("geometry K%d %d..%d %s" % (K, kh, kl, mode))
            top = (K if mode == "protein" else 3 * K) + 8
            assert [s.shape[0] for s in c.seqs] == list(range(top + 1)) and (c.k_high, c.k_low) == (kh, kl)
            e = ec.expected(c)
            assert e.seq_count[0] == 0 and e.seq_count[-1] > 0 and (e.seq_count == 0).sum() >= 3
    for K in (12, 25):
        for mode in ("dna3", "dna6"):
            e = {w: ec.expected("geometry K%d %s %s without k-mers" % (K, mode, w)) for w in ("first", "last", "none", "one empty")}
            assert e["first"].read_count[0] == 0 and e["first"].read_count[1] == 0 and e["first"].read_count[2] > 0 and e["first"].read_count[-1] == 0
            assert e["last"].read_count[-1] == 0 and e["last"].read_count[-2] == 0 and e["last"].read_count[-3] > 0
            assert e["none"].keys.shape[0] == 0 and e["none"].read_count.shape[0] > 3 and e["one empty"].read_count.tolist() == [0]
        c = ec.case("geometry K%d dna3 offsets from 21" % K)
        off = c.batch()[1]
        assert off[0] == c.shift == 21 and off[0] % 16 and ec.expected(c).keys.shape[0] > 0


def test_no_read_of_one_or_two_kmers_in_three_frames():
    for name in ALL:
        c = ec.case(name)
        if c.mode in ("dna3", "dna6"):
            per = ec.expected(name).seq_count // ec.strands(c.mode)
            assert not np.isin(per, (1, 2)).any(), name
    for K, _, kl in ec.GEOMETRIES:
        assert {ec.geometry(raw, K, kl, "dna3")[2] for raw in range(0, 3 * K + 9)} >= {0, 3, 4} and ec.geometry(3 * K + 2 - 3 * (K - kl), K, kl, "dna3")[2] in (0, 3)


# ---- packing ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.case_names("packing"))
def test_packing_every_value_at_every_letter(name):
    c = ec.case(name)
    K, fill = c.K, c.claim["fill"]
    base = sum(fill << 5 * i for i in range(K))
    for v in range(32):
        ks = read_keys(name, v)
        assert len(ks) == K
        for j in range(K):                                                               # window K - 1 - j has the value at letter j
            sh = 5 * (K - 1 - j)
            assert ks[K - 1 - j] == (base & ~(31 << sh)) | (v << sh), (name, v, j)
    assert K == 12 or any((5 * (K - 1 - j)) < 64 < (5 * (K - 1 - j)) + 5 for j in range(K)), "a letter lies across bit 64"


# ---- bounds -------------------------------------------------------------------------------------
def test_bounds_counts_on_both_sides():
    for K in (12, 25):
        got = {}
        for name in ec.case_names("bounds", K=K):
            c, e = ec.case(name), ec.expected(name)
            n, at = c.claim["k-mers"], c.claim["at"]
            assert int(e.read_count[at]) == n == int(e.read_count.max()) and sorted(e.read_count.tolist())[-2] <= 80, name
            got.setdefault(c.mode, {})[(n, "first" if at == 0 else "last")] = c.form
        short = {m: ec.short_form(K, m) for m in ec.MODES}
        for mode in ("dna3", "one", "protein"):
            g = got[mode]
            assert g[(ec.SMALL_RM, "first")] == short[mode] and g[(ec.SMALL_RM + 1, "first")] == "slots512"
            assert g[(ec.ENC_RANK_MAX, "first")] == "slots512" and g[(ec.ENC_RANK_MAX + 1, "first")] == "readid"
        for mode in ("dna3", "one"):
            assert (ec.SMALL_RM - 1, "first") in got[mode] and (ec.ENC_RANK_MAX - 1, "first") in got[mode]
        assert got["dna3"][(ec.SMALL_RM + 1, "last")] == "slots512" and got["dna3"][(ec.ENC_RANK_MAX + 1, "last")] == "readid"
        six = got["dna6"]
        assert [six[(2 * n, "first")] for n in (95, 96, 97, 255, 256, 257)] == [short["dna6"]] * 2 + ["slots512"] * 3 + ["readid"]
        assert ec.SMALL_RM == 192 and ec.ENC_RANK_MAX == 512, "twice 96 and twice 256 are the bounds"
        for n in ec.CHUNK_COUNTS:
            assert (n, "first") in got["dna3"] and (2 * n, "first") in six
        for n in ec.ONE_CHUNK_COUNTS:
            assert (n, "first") in got["one"]
        assert ec.ONE_CHUNK_COUNTS == (169, 170, 171, 340, 341) and ec.CHUNK_COUNTS == (511, 512, 513, 1024, 1025)


# ---- group_parts --------------------------------------------------------------------------------
def test_group_parts():
    G, RM, CAPK = ec.ENC_GROUP, ec.ENC_GROUP_RM, ec.CAPK
    for name in ec.case_names("group_parts"):
        c, e = ec.case(name), ec.expected(name)
        flat = [n for g in c.claim["groups"] for n in g]
        assert e.read_count.tolist() == flat and max(flat) <= RM, name
        assert all(len(g) == G for g in c.claim["groups"][:-1])
    groups = ec.case("group_parts totals").claim["groups"]
    ends = set()                                                                        # (reads of a group's first part, its k-mers up to and with the next read)
    for g in groups:
        parts = ec.group_parts(g)
        assert all(k <= CAPK for _, _, k in parts) and sum(k for _, _, k in parts) == sum(g)
        first_end = parts[0][1]
        ends.add((first_end, sum(g[:first_end + 1]) if first_end < G else sum(g)))
    for s in range(1, G):
        if (s + 1) * RM > CAPK:                                                         # a part can end behind read s
            assert (s, CAPK + 1) in ends, s
            assert any(sum(g[:s + 1]) == CAPK - 1 and ec.group_parts(g)[0][1] > s for g in groups)
            assert any(sum(g[:s + 1]) == CAPK and ec.group_parts(g)[0][1] > s for g in groups)
    assert any((s + 1) * RM > CAPK for s in range(1, G)), "no group can exceed a part: the family is empty"
    assert [RM] * (G - 1) + [3] in groups and [3] + [RM] * (G - 1) in groups and [RM] * G in groups
    zeros = ec.case("group_parts zeros").claim["groups"]
    assert any(g[0] == 0 and min(g[1:]) > 0 for g in zeros) and any(g[-1] == 0 and min(g[:-1]) > 0 for g in zeros)
    assert any(g[0] > 0 and g[-1] > 0 and 0 in g for g in zeros) and [0] * G in zeros
    for r in range(1, G):
        assert len(ec.case("group_parts tail %d" % r).claim["groups"][-1]) == r and len(ec.case("group_parts only %d" % r).seqs) == r
    assert len(ec.case("group_parts many").claim["groups"]) > 2 * ec.ENC_WAVES


# ---- ranking ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.case_names("ranking"))
def test_ranking_bit_patterns(name):
    c = ec.case(name)
    K, stride, pattern = c.K, c.claim["stride"], c.claim["pattern"]
    keys = read_keys(name, 0)
    frame0 = keys[::stride] if c.mode != "dna6" else keys[:len(keys) // 2]
    letters = sorted(ec.codon_of_letter("telling")) if c.mode in ("dna3", "one") else list(range(32))
    if pattern == "equal":
        assert len(set(frame0)) == 1 and len(keys) in (ec.ENC_GROUP_RM, ec.SMALL_RM, ec.ENC_RANK_MAX)
        if c.mode == "dna6":
            assert len(set(keys)) == 2
    elif pattern == "ascending":
        assert all(a < b for a, b in zip(frame0, frame0[1:])) and len(frame0) >= 32
    elif pattern == "descending":
        assert all(a > b for a, b in zip(frame0, frame0[1:])) and len(frame0) >= 32
    elif pattern == "first":
        assert {k >> 5 * (K - 1) for k in frame0} >= set(letters) and len(letters) == 32
    elif pattern == "pairs":
        assert frame0[:3] == frame0[-3:] and len(frame0) >= K + 3 and len(set(frame0[:3])) == 3
    else:
        kind, places = pattern
        mask = sum(31 << 5 * (K - 1 - p) for p in places)
        ks = frame0[::K][:-1]                                                            # the windows at the blocks' starts
        assert len(ks) >= 4 and len(set(ks)) == len(ks), (name, len(ks))
        assert all((a ^ ks[0]) & ~mask == 0 for a in ks), "they differ in the named letters alone"
        if kind == "bits78":                                                             # top six bits equal, bits 7-8 from the top all different, nothing else
            assert len({k >> (5 * K - 6) for k in ks}) == 1 and len({(k >> (5 * K - 8)) & 3 for k in ks}) == len(ks) == 4
            assert all((a ^ ks[0]) & ~(3 << (5 * K - 8)) == 0 for a in ks)
        if places == [K - 1]:
            assert all(a >> 5 == ks[0] >> 5 for a in ks), "all keys agree in bits >= 5 and differ below"
        if K == 25 and places == [0]:
            assert len({k & ((1 << 64) - 1) for k in ks}) == 1                           # the low halves are equal
        if K == 25 and places == [K - 1]:
            assert len({k >> 64 for k in ks}) == 1                                       # the high halves are equal
        if places == [12, 13]:
            assert len({k >> 64 for k in ks}) > 1 and len({k & ((1 << 64) - 1) for k in ks}) > 1 and mask & (1 << 64) and mask & (1 << 63)


# ---- segments -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in ec.case_names("segments") if "as reads" not in n])
def test_segments_no_kmer_across_a_junction(name):
    c, e = ec.case(name), ec.expected(name)
    per_read = np.bincount(c.seg_read, minlength=c.n_reads).tolist()
    assert {0, 1, 2, 3} <= set(per_read) and any(s.shape[0] == 0 for s in c.seqs)
    assert sorted(c.seg_read) == list(c.seg_read) and e.slot is None
    lut = ec.table(c.lut)
    for r in (c.claim["too short alone"], c.claim["junction"]):
        mates = [i for i, x in enumerate(c.seg_read) if x == r]
        assert len(mates) == 2
        joined = np.concatenate([c.seqs[i] for i in mates])
        jk = ec.sequence_keys(joined, c.K, c.k_low, c.mode, lut)
        mine = set(read_keys(name, r))
        assert int(e.read_count[r]) == sum(int(e.seq_count[i]) for i in mates) < jk.shape[0]
        n1, per = c.seqs[mates[0]].shape[0], jk.shape[0] // ec.strands(c.mode)
        across = [w for w in range(per) if w < n1 < w + 3 * c.K]                           # forward windows with bases of both mates
        assert across and not {ec.key_int(jk[w]) for w in across} & mine
    assert int(e.read_count[c.claim["too short alone"]]) == 0
    plain = ec.case(name + " as reads")
    assert plain.debug == 8 and plain.seg_read is None and np.array_equal(ec.expected(plain).keys, e.keys)


# ---- long ---------------------------------------------------------------------------------------
def test_long_counts():
    M = ec.ENC_LONG_MIN
    for name in ec.case_names("long", large=True):
        c, e = ec.case(name), ec.expected(name)
        assert e.seq_count.tolist() == c.claim["counts"], name
    for d, form, listed in ((-1, "readid", None), (0, "long", 1), (1, "long", 1)):
        c = ec.case("long K12 dna3 %d" % (M + d))
        assert M + d in c.claim["counts"] and (c.form, c.second_launch) == (form, listed)
        c = ec.case("long K12 dna6 2x%d" % (M // 2 + d))
        assert 2 * (M // 2 + d) in c.claim["counts"] and (c.form, c.second_launch) == (form, listed)
    two = ec.case("long K12 dna3 two")
    big = [i for i, n in enumerate(two.claim["counts"]) if n >= M]
    assert len(big) == 2 == two.second_launch and big[0] > 0 and big[1] - big[0] > 1 and big[1] < len(two.seqs) - 1
    pair = ec.case("long K12 dna3 pair of 40000")
    assert pair.claim["counts"] == [40000, 40000] and pair.seg_read == [0, 0] and (pair.form, pair.second_launch) == ("readid", 0) and 80000 >= M > 40000
    mate = ec.case("long K12 dna3 long mate")
    assert mate.seg_read == [0, 0] and (mate.form, mate.second_launch) == ("long", 1)
    sweep = ec.case("long K12 dna3 second sweep")
    assert sweep.claim["counts"][0] == ec.LONG_SWEEP + ec.ENC_CHUNK + 7 and not sweep.wide
    assert {ec.case(n).mode for n in ec.case_names("long")} == set(ec.MODES) and {ec.case(n).K for n in ec.case_names("long")} == {12, 25}
