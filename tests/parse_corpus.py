"""Texts for the device parser (kasa_amd/csrc/kasa_parse.h), built so that every case its kernels tell apart occurs: plain
Python, no device.  `corpus(T)` (T = capi.parse_tile_bytes()) is a deterministic list of members

    (name, text, fasta, expectation, ...)      expectation: "parsable" | every offence in the text as (chunk position, code)

in the groups of DESIGN.md section 8d ("How it is tested"):
  A  gather alignment: every (source start mod 4, destination start mod 16, length 1..16 | 17 and more) of a sequence line
     and of a name entry, behind a prefill that sets the pool's lead to 0..15
  B  runs of one-byte entries, also across an output tile edge
  C  line feeds on lane, step and tile edges; chunks of exactly a tile; tiles without a feed and of nothing but feeds
  D  every byte value
  E  records without letters
  F  refusals, with the position kasa_parse_status must give
  G  `pool_scripts()`: appends, takes and fetches against a list model that knows which branch of pool_compact each
     append takes and when a pool array has to grow with reads in it
What the builder says about a text (`gather_cases`, `Member.claims`, `scan_offences`, the model's counts) is computed from the
text alone and asserted by tests/test_parse_corpus_cpu.py."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from kasa_amd import reads

OK, FASTQ_LINES, FASTQ_HEADER, FASTQ_PLUS, FASTQ_QUALITY, EMPTY_LINE, BLANK, LONG, FASTA_HEADER, FASTQ_SEQ_PLUS = range(10)   # KASA_PARSE_*
CLASSIFY_STAGE = {FASTQ_LINES, FASTQ_HEADER, FASTQ_PLUS, FASTQ_QUALITY, EMPTY_LINE, FASTQ_SEQ_PLUS}    # (and LONG of a FASTQ line)
PARSABLE = "parsable"
GOOD = b"@g0\nACGTACGT\n+\nIIIIIIII\n@g1\nTTTT\n+\nIIII\n"       # the two reads pooled before every refused append: 12 letters, 6 name bytes


class Member(NamedTuple):
    name: str
    text: bytes
    fasta: bool
    expectation: object
    group: str = ""
    prefill: bytes = b""             # appended to the fresh pool first: its letters and name bytes are the gathers' leads
    prefill_fasta: bool = False
    long_sequence: int = 1_000_000
    claims: dict = None              # what the builder says about the text, for the CPU test


# ---------------------------------------------------------------------------------------------------------------- reading a text
def lines_of(text: bytes):
    """(start, length) of every line; only the last one may lack its line feed."""
    if not text:
        return []
    out, pos = [], 0
    for ln in text.split(b"\n"):
        out.append((pos, len(ln)))
        pos += len(ln) + 1
    if text.endswith(b"\n"):
        out.pop()
    return out


def entries(text: bytes, fasta: bool):
    """What the two gathers copy, in order: sequence lines as (chunk position, bytes) and name entries as (position of the
    header's second byte, bytes of the header: the header less its first character plus one space)."""
    seq, names = [], []
    for i, (s, n) in enumerate(lines_of(text)):
        if fasta:
            if n == 0:
                continue
            (names if text[s] == 0x3E else seq).append((s + 1, n) if text[s] == 0x3E else (s, n))
        elif i % 4 == 0:
            names.append((s + 1, n))
        elif i % 4 == 1:
            seq.append((s, n))
    return seq, names


def pooled_bytes(text: bytes, fasta: bool):
    """(letters, name bytes) a chunk adds to the pool: a fresh pool's leads behind it are these mod 16."""
    seq, names = entries(text, fasta)
    return sum(n for _, n in seq), sum(n for _, n in names)


def gather_cases(text: bytes, fasta: bool, base_lead: int, name_lead: int):
    """The (source start mod 4, destination start mod 16, min(length, 17)) of every sequence line and of every name entry of a
    chunk appended behind `base_lead` letters and `name_lead` name bytes."""
    def cases(ents, lead):
        out, d = set(), lead
        for s, n in ents:
            out.add((s % 4, d % 16, min(n, 17)))
            d += n
        return out
    seq, names = entries(text, fasta)
    return cases(seq, base_lead), cases(names, name_lead)


ALL_CASES = frozenset((s, d, c) for s in range(4) for d in range(16) for c in range(1, 18))


def scan_offences(text: bytes, fasta: bool, long_sequence: int = 1_000_000):
    """Every reason the device has to refuse the chunk, as (chunk position, code), sorted: the strict form of DESIGN.md 8d."""
    out, ln = [], lines_of(text)
    blanks = lambda s, n: [(s + k, BLANK) for k in range(n) if text[s + k] in (0x20, 0x09)]
    if fasta:
        hdr, letters = None, 0
        for s, n in ln + [(len(text), -1)]:
            if n == -1 or (n > 0 and text[s] == 0x3E):
                if hdr is not None and letters >= long_sequence:
                    out.append((hdr, LONG))
                hdr, letters = s, 0
            elif n > 0:
                letters += n
                out += blanks(s, n)
        return sorted(out)
    if len(ln) % 4:
        out.append((ln[len(ln) & ~3][0], FASTQ_LINES))
    for i, (s, n) in enumerate(ln):
        m, c0 = i % 4, text[s] if n else 0
        if n == 0:
            out.append((s, EMPTY_LINE))
        elif m == 0 and c0 != 0x40:
            out.append((s, FASTQ_HEADER))
        elif m == 1 and c0 == 0x2B:
            out.append((s, FASTQ_SEQ_PLUS))
        elif m == 1 and n >= long_sequence:
            out.append((s, LONG))
        elif m == 2 and c0 != 0x2B:
            out.append((s, FASTQ_PLUS))
        elif m == 3 and n != ln[i - 2][1]:
            out.append((s, FASTQ_QUALITY))
        if m == 1:
            out += blanks(s, n)
    return sorted(out)


def reported(offences, fasta: bool):
    """The (position, code) kasa_parse_status gives for a chunk with these offences.  The classify stage is read before the
    gathers run: if it found anything, its earliest offence is the answer and blanks are not looked at; otherwise the
    earliest among the blanks and the FASTA long-sequence bound.  Two codes at one position: the smaller code."""
    first = [o for o in offences if o[1] in CLASSIFY_STAGE or (o[1] == LONG and not fasta)]
    return min(first or offences)


def dump_safe(m: Member) -> bool:
    """Can the driver's parse-dump line format carry the member: no tab, CR or byte >= 0x80 in names or letters."""
    data = m.prefill + m.text
    return m.expectation == PARSABLE and not any(b in data for b in (b"\t", b"\r")) and max(data) < 0x80 and min(data) > 0


# ---------------------------------------------------------------------------------------------------------------- letters
_DNA = np.frombuffer(b"ACGTACGTACGTNacgtn", dtype=np.uint8)
_NAME = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789_:/|.>@+ -", dtype=np.uint8)


def _dna(rng, n):
    return _DNA[rng.integers(0, _DNA.shape[0], n)].tobytes()


def _name(rng, n):
    return _NAME[rng.integers(0, _NAME.shape[0], n)].tobytes()


def _qual(rng, n):
    return bytes(rng.integers(33, 74, n).astype(np.uint8))


def _wrap(s: bytes, w: int) -> bytes:
    return b"".join(s[i:i + w] + b"\n" for i in range(0, len(s), w))


def _fastq(name: bytes, seq: bytes, rng=None) -> bytes:
    return b"@" + name + b"\n" + seq + b"\n+\n" + (_qual(rng, len(seq)) if rng is not None else b"I" * len(seq)) + b"\n"


# ---------------------------------------------------------------------------------------------------------------- group A
def lead_prefill(lead: int, fasta: bool) -> bytes:
    """One record of k letters under a name entry of k bytes, k = lead (16 for lead 0)."""
    k = lead or 16
    return (b">" if fasta else b"@") + b"p" * (k - 1) + b"\n" + b"A" * k + (b"\n" if fasta else b"\n+\n" + b"I" * k + b"\n")


def _group_a(fasta: bool, seed: int):
    """A steered draw: every record takes the name length and the line lengths that hit the most cases not yet seen, and
    among equals the ones that leave the pool's ends where cases are still missing."""
    rng = np.random.default_rng(seed)
    todo_n, todo_s = set(ALL_CASES), set(ALL_CASES)
    left_n = np.full((4, 16), 17)                  # cases still missing per (source mod 4, destination mod 16)
    left_s = np.full((4, 16), 17)

    def hit(todo, left, case):
        if case in todo:
            todo.discard(case)
            left[case[0], case[1]] -= 1

    members, total = [], 2 * len(ALL_CASES)
    for part in range(64):
        lead = part % 16
        if part >= 16 and not (todo_n or todo_s):
            break
        goal = total * (15 - lead) // 16 if part < 16 else 0       # cases that may be left to the members after this one
        out, pos, bd, nd = [], 0, lead, lead
        while pos < 7000 and len(todo_n) + len(todo_s) > goal:
            # ---- the name: its entry is the header's length
            src = (pos + 1) % 4
            best, pick = -1.0, 1
            for n in list(range(1, 17)) + list(range(17, 41)):
                c = (src, nd % 16, min(n, 17))
                sc = 100.0 * (c in todo_n) + 40.0 * (left_s[(pos + n + 1) % 4, bd % 16] > 0) + left_n[:, (nd + n) % 16].sum() / 4 + rng.random()
                if sc > best:
                    best, pick = sc, n
            n = pick
            hit(todo_n, left_n, (src, nd % 16, min(n, 17)))
            hdr = (b">" if fasta else b"@") + _name(rng, n - 1)
            spos = pos + n + 1
            if not fasta:                            # ---- one sequence line of 1..40
                best, pick = -1.0, 1
                for L in range(1, 41):
                    c = (spos % 4, bd % 16, min(L, 17))
                    sc = 100.0 * (c in todo_s) + left_s[:, (bd + L) % 16].sum() / 4 + left_n[(pos + n + 2 * L + 6) % 4, (nd + n) % 16] + rng.random()
                    if sc > best:
                        best, pick = sc, L
                L = pick
                hit(todo_s, left_s, (spos % 4, bd % 16, min(L, 17)))
                seq = _dna(rng, L)
                rec = hdr + b"\n" + seq + b"\n+\n" + _qual(rng, L) + b"\n"
                bd += L
            else:                                    # ---- lines wrapped at w in 1..40: m full ones and a last one of r
                best, pick = -1.0, (1, 0, 1)
                for _ in range(24):
                    w = int(rng.integers(1, 41))
                    cand = (w, int(rng.integers(0, 4)), int(rng.integers(1, w + 1)))
                    p, d, new = spos, bd, set()
                    for L in [cand[0]] * cand[1] + [cand[2]]:
                        c = (p % 4, d % 16, min(L, 17))
                        if c in todo_s:
                            new.add(c)
                        p, d = p + L + 1, d + L
                    sc = 100.0 * len(new) + left_s[:, d % 16].sum() / 4 + left_n[(p + 1) % 4, (nd + n) % 16] + rng.random()
                    if sc > best:
                        best, pick = sc, cand
                w, m, r = pick
                seq = _dna(rng, w * m + r)
                p = spos
                for L in [w] * m + [r]:
                    hit(todo_s, left_s, (p % 4, bd % 16, min(L, 17)))
                    p, bd = p + L + 1, bd + L
                rec = hdr + b"\n" + _wrap(seq, w)
            out.append(rec)
            pos += len(rec)
            nd += n
        if out:
            fmt = "fasta" if fasta else "fastq"
            members.append(Member(f"A-{fmt}-lead{lead}" + (f"-more{part // 16}" if part >= 16 else ""), b"".join(out), fasta, PARSABLE, "A",
                                  lead_prefill(lead, fasta), fasta))
    return members


# ---------------------------------------------------------------------------------------------------------------- group B
RUN = 48


def _group_b(T: int):
    rng = np.random.default_rng(202)
    out = []
    for at in (None, T - 24, T - 1, T):            # where in the output the run starts (None: right behind one short record)
        tag = "start" if at is None else f"at{at}"
        fill = 8 if at is None else at
        # one-letter FASTA sequence lines: the letters in front of the run are the output offset
        text = b">filler\n" + _wrap(_dna(rng, fill), 60) + b">run\n" + b"".join(bytes([c]) + b"\n" for c in _dna(rng, RUN)) + b">after\n" + _wrap(_dna(rng, 70), 60)
        out.append(Member(f"B-fasta-lines-{tag}", text, True, PARSABLE, "B", claims={"run": "lines", "offset": fill}))
        # '>'-only headers with one-letter sequences: the name bytes in front of the run are the output offset
        head = b">" + _name(rng, fill - 1) + b"\n" + _dna(rng, 33) + b"\n"
        text = head + b"".join(b">\n" + bytes([c]) + b"\n" for c in _dna(rng, RUN)) + b">after the run\nACGTTGCA\n"
        out.append(Member(f"B-fasta-headers-{tag}", text, True, PARSABLE, "B", claims={"run": "headers", "offset": fill}))
        head = b"@" + _name(rng, fill - 1) + b"\n" + _dna(rng, fill) + b"\n+\n" + _qual(rng, fill) + b"\n"
        text = head + b"".join(b"@\n" + bytes([c]) + b"\n+\n" + bytes([q]) + b"\n" for c, q in zip(_dna(rng, RUN), _qual(rng, RUN))) + _fastq(b"after", b"ACGTTGCA")
        out.append(Member(f"B-fastq-minimal-{tag}", text, False, PARSABLE, "B", claims={"run": "both", "offset": fill}))
    return out


# ---------------------------------------------------------------------------------------------------------------- group C
def _sized(rng, size: int, final_feed: bool, fasta: bool) -> bytes:
    """A chunk of exactly `size` bytes."""
    if fasta:
        head = b">first\n" + _wrap(_dna(rng, 100), 60) + b">sized to the byte\n"
        body = bytearray(_wrap(_dna(rng, size), 61)[:size - len(head)])      # 61 letters and a feed a line, cut to the byte
        for k in ((-2,) if final_feed else (-1,)):                          # no empty last line, no feed where none is wanted
            if body[k] == 0x0A:
                body[k] = 0x41
        if final_feed:
            body[-1] = 0x0A
        return head + bytes(body)
    recs, used = [], 0
    while size - used >= 300:
        recs.append(_fastq(b"r%d x" % len(recs), _dna(rng, int(rng.integers(1, 100))), rng))
        used += len(recs[-1])
    rest = size - used + (0 if final_feed else 1)   # = name + 2 L + 6 with the last feed counted
    name = b"zz" if rest % 2 == 0 else b"zzz"
    last = _fastq(name, _dna(rng, (rest - 6 - len(name)) // 2), rng)
    return b"".join(recs) + (last if final_feed else last[:-1])


def _group_c(T: int):
    rng = np.random.default_rng(303)
    out = []
    for p in (15, 16, 17, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T - 1, 2 * T):
        tail_a, tail_q = b"ACGTTGCATT\n>next\nGG\nTTA\n", _fastq(b"next", b"GGTTA", rng)
        texts = {"fasta-seq": (b">c\n" + _dna(rng, p - 3) + b"\n" + tail_a, True),
                 "fasta-hdr": (b">" + _name(rng, p - 1) + b"\n" + tail_a, True),
                 "fastq-seq": (b"@c\n" + _dna(rng, p - 3) + b"\n+\n" + _qual(rng, p - 3) + b"\n" + tail_q, False)}
        for kind, (text, fasta) in texts.items():
            out.append(Member(f"C-feed{p}-{kind}", text, fasta, PARSABLE, "C", claims={"feed_at": p}))
    for size in (T - 1, T, T + 1, 2 * T):
        for final_feed in (True, False):
            for fasta in (True, False):
                out.append(Member(f"C-size{size}-{'fasta' if fasta else 'fastq'}-{'feed' if final_feed else 'nofeed'}", _sized(rng, size, final_feed, fasta), fasta,
                                  PARSABLE, "C", claims={"size": size, "final_feed": final_feed}))
    out.append(Member("C-line-of-3T+1", b">short\nACGT\n>one line\n" + _dna(rng, 3 * T + 1) + b"\n>last\nTTGA\n", True, PARSABLE, "C", claims={"line": 3 * T + 1}))
    out.append(Member("C-empty-lines", b">e\nACGT\n" + b"\n" * (T + 5) + b"TTGA\n" + b"\n" * 70 + b">f\nCC\n", True, PARSABLE, "C", claims={"feeds": (8, T + 5)}))
    head = _sized(rng, T, True, True)
    out.append(Member("C-tile-of-feeds", head + b"\n" * (T + 5) + b"TTGA\n>f\nCC\n", True, PARSABLE, "C", claims={"feeds": (T, T + 5)}))
    for name in (f"C-feed{T}-fasta-seq", f"C-size{T}-fastq-feed"):
        m = next(x for x in out if x.name == name)
        out.append(Member(name + "-crlf", m.text.replace(b"\n", b"\r\n"), m.fasta, PARSABLE, "C"))
    return out


# ---------------------------------------------------------------------------------------------------------------- group D
def _group_d():
    names = bytes(b for b in range(256) if b != 0x0A)
    letters = bytes(b for b in list(range(0x41, 256)) + list(range(0, 0x41)) if b not in (0x0A, 0x20, 0x09))   # (starts with 'A': no '>' or '+' up front)
    assert len(names) == 255 and len(letters) == 253 and all(b in letters for b in (0x00, 0x89, 0x8A, 0xA0))
    out = []
    for k in range(4):                             # the same bytes at every position of a 32-bit word
        pad = b"n" * k
        out.append(Member(f"D-fasta-names-{k}", b">" + pad + names + b"\nACGT\n>" + names[::-1] + b"\nTT\n", True, PARSABLE, "D"))
        out.append(Member(f"D-fastq-names-{k}", _fastq(pad + names, b"ACGT") + _fastq(names[::-1], b"TT"), False, PARSABLE, "D"))
        w = (7, 8, 9, 11)[k]
        out.append(Member(f"D-fasta-letters-{k}", b">" + pad + b"\n" + letters + b"\n>wrapped\n" + _wrap(letters, w), True, PARSABLE, "D",
                          claims={"lengths": (254, 253 + (253 + w - 1) // w)}))
        out.append(Member(f"D-fastq-letters-{k}", _fastq(pad, letters) + _fastq(b"again", letters[::-1][3:] + b"ACG"), False, PARSABLE, "D", claims={"lengths": (254, 254)}))
    for m in out:                                   # no wrapped line may look like a header
        assert len(entries(m.text, m.fasta)[1]) == 2, m.name
    return out


# ---------------------------------------------------------------------------------------------------------------- group E
def _group_e():
    none = b">a\n>b x\n>\n>d\n\n\n>e\n"
    return [Member("E-no-record-has-letters", none, True, PARSABLE, "E"),
            Member("E-no-letters-no-final-feed", none[:-1], True, PARSABLE, "E"),
            Member("E-first-middle-last", b">e\n>a\nACGT\nTT\n>m\n\n>b\nGG\n>z\n", True, PARSABLE, "E"),
            Member("E-first", b">e\n>a\nACGT\n", True, PARSABLE, "E"),
            Member("E-middle", b">a\nACGT\n>m\n>b\nG\n", True, PARSABLE, "E"),
            Member("E-last", b">a\nACGT\n>z", True, PARSABLE, "E"),
            Member("E-append-behind-no-letters", b">a\nACGTACGTACGTACGTACGT\nTTG\n>b\nC\n", True, PARSABLE, "E", none, True),
            Member("E-no-letters-behind-reads", none, True, PARSABLE, "E", GOOD, False),
            Member("E-fastq-behind-no-letters", GOOD, False, PARSABLE, "E", none, True)]


# ---------------------------------------------------------------------------------------------------------------- group F
def _blank_in_vector(q: int, blank: bytes, hdr: bytes, whole: bool, second: int = None):
    """A blank at byte q (and another at byte `second`) of the output vector at absolute pool offset 32, behind GOOD's 12
    letters: in a line of 48 letters (the whole vector comes from it) or in lines of 5 (the vector spans lines)."""
    idx = [20 + k for k in ((q,) if second is None else (q, second))]      # letter 20 + q lies at pool offset 32 + q
    seq = bytearray(b"ACGTTGCA" * 8)[:48 if whole else 60]
    for i in idx:
        seq[i:i + 1] = blank
    if whole:
        text = b"@" + hdr + b"\n" + bytes(seq) + b"\n+\n" + b"I" * 48 + b"\n"
        return text, [(len(hdr) + 2 + i, BLANK) for i in idx]
    text = b">" + hdr + b"\n" + _wrap(bytes(seq), 5)
    return text, [(len(hdr) + 2 + i // 5 * 6 + i % 5, BLANK) for i in idx]


def _group_f(T: int):
    out = []

    def add(name, text, fasta, offences, long_sequence=1_000_000, claims=None):
        out.append(Member("F-" + name, text, fasta, PARSABLE if offences is None else sorted(offences), "F", GOOD, False, long_sequence, claims))

    for whole in (True, False):
        for blank, bn in ((b" ", "space"), (b"\t", "tab")):
            for hdr in (b"a", b"ab"):
                for q in range(16):
                    text, off = _blank_in_vector(q, blank, hdr, whole)
                    add(f"{'whole' if whole else 'span'}-{bn}-src{len(hdr)}-byte{q}", text, not whole, off, claims={"vector_byte": q, "whole": whole})
        for q, second in ((3, 9), (0, 15), (14, 15)):                        # two in ONE vector: the smaller position
            text, off = _blank_in_vector(q, b" ", b"a", whole, second)
            add(f"{'whole' if whole else 'span'}-two-in-one-vector-{q}-{second}", text, not whole, off, claims={"vector_byte": q, "whole": whole})
    rng = np.random.default_rng(606)
    for first, second in ((100, T + 900), (T - 13, T - 12), (700, 2 * T + 5)):   # two blanks in different output tiles (GOOD's 12 letters lie in front)
        seq = bytearray(_dna(rng, 2 * T + 200))
        seq[first:first + 1], seq[second:second + 1] = b" ", b"\t"
        add(f"two-tiles-fasta-{first}-{second}", b">t\n" + _wrap(bytes(seq), 60), True, [(3 + k // 60 * 61 + k % 60, BLANK) for k in (first, second)],
            claims={"tiles": ((12 + first) // T, (12 + second) // T)})
        add(f"two-tiles-fastq-{first}-{second}", b"@t\n" + bytes(seq) + b"\n+\n" + b"I" * len(seq) + b"\n", False, [(3 + k, BLANK) for k in (first, second)],
            claims={"tiles": ((12 + first) // T, (12 + second) // T)})
    # two classify-stage offences: a short quality early, a header without '@' late
    r = [_fastq(b"r0", b"ACGTAC"), b"@r1\nACGT\n+\nIII\n", _fastq(b"r2", b"GGTT"), b"xr3\nAC\n+\nII\n", _fastq(b"r4", b"T")]
    at = lambda k: sum(len(x) for x in r[:k])
    add("quality-early-header-late", b"".join(r), False, [(at(1) + 11, FASTQ_QUALITY), (at(3), FASTQ_HEADER)])
    r = [_fastq(b"r0", b"ACGTAC"), b"@r1\nAC\n-\nII\n", b"@r2\n\n+\n\n", _fastq(b"r3", b"T")]
    add("plus-then-empty-lines", b"".join(r), False, [(at(1) + 7, FASTQ_PLUS), (at(2) + 4, EMPTY_LINE), (at(2) + 7, EMPTY_LINE)])
    # a classify-stage offence together with an EARLIER blank: the classify stage is read first
    r = [b"@r0\nAC GT\n+\nIIIII\n", _fastq(b"r1", b"GG"), b"@r2\nAC\n*\nII\n"]
    add("blank-early-plus-late", b"".join(r), False, [(6, BLANK), (at(2) + 7, FASTQ_PLUS)])
    r = [b"@r0\nAC\tGT\n+\nIIIII\n", b"@r1\n+CGT\n+\nIIII\n"]
    add("blank-early-seq-plus-late", b"".join(r), False, [(6, BLANK), (at(1) + 4, FASTQ_SEQ_PLUS)])
    # the FASTA bound is a sum over the record's lines; `at` is the start of its header line
    L = 500
    front = b">ok\nACGT\n\n"
    add("fasta-long-minus-1", front + b">long\n" + _wrap(_dna(rng, L - 1), 7) + b"\n>last\nAC\n", True, None, L)
    add("fasta-long-minus-1-last-record", front + b">long\n" + _wrap(_dna(rng, L - 1), 7)[:-1], True, None, L)
    add("fasta-long", front + b">long\n" + _wrap(_dna(rng, L), 7) + b">last\nAC\n", True, [(len(front), LONG)], L)
    add("fasta-long-last-record-one-line", front + b">long\n" + _dna(rng, L), True, [(len(front), LONG)], L)
    seq = bytearray(_dna(rng, L + 30)); seq[40:41] = b" "
    add("fasta-long-with-a-blank-inside", front + b">long\n" + _wrap(bytes(seq), 7), True, [(len(front), LONG), (len(front) + 6 + 40 // 7 * 8 + 40 % 7, BLANK)], L)
    add("fasta-blank-before-long", b">b\nAC GT\n>long\n" + _wrap(_dna(rng, L), 50), True, [(5, BLANK), (9, LONG)], L)
    add("fasta-two-long", front + b">l1\n" + _wrap(_dna(rng, L), 50) + b">l2\n" + _dna(rng, L + 1) + b"\n", True, [(len(front), LONG), (len(front) + 4 + L + L // 50, LONG)], L)
    add("fastq-long-minus-1", _fastq(b"a", _dna(rng, L - 1), rng), False, None, L)
    add("fastq-long", _fastq(b"ok", b"ACGT") + _fastq(b"a", _dna(rng, L), rng), False, [(len(_fastq(b"ok", b"ACGT")) + 3, LONG)], L)
    # the line count: `at` is the start of line (lines & ~3)
    rec = _fastq(b"r0", b"ACGT")
    add("fastq-6-lines", rec + b"@r1\nACGT\n", False, [(len(rec), FASTQ_LINES)])
    add("fastq-7-lines-no-final-feed", rec + b"@r1\nACGT\n+", False, [(len(rec), FASTQ_LINES)])
    add("fastq-3-lines", b"@r0\nACGT\n+\n", False, [(0, FASTQ_LINES)])
    add("fastq-5-lines-bad-header", rec + b"r1\n", False, [(len(rec), FASTQ_LINES), (len(rec), FASTQ_HEADER)])
    add("fastq-9-lines-quality-earlier", b"@r0\nACGT\n+\nIIIII\n" + rec + b"@r2\n", False, [(11, FASTQ_QUALITY), (17 + len(rec), FASTQ_LINES)])
    return out


# ---------------------------------------------------------------------------------------------------------------- the corpus
@functools.lru_cache(maxsize=None)
def corpus(T: int = 4096):
    out = _group_a(False, 101) + _group_a(True, 102) + _group_b(T) + _group_c(T) + _group_d() + _group_e() + _group_f(T)
    assert len({m.name for m in out}) == len(out)
    return tuple(out)


def group(T: int, g: str, fasta=None):
    return [m for m in corpus(T) if m.group == g and (fasta is None or m.fasta == fasta)]


# ---------------------------------------------------------------------------------------------------------------- group G
class Read(NamedTuple):
    name: str        # the name entry: header less its first character plus one space
    letters: bytes
    length: int      # letters + one per sequence line


def as_batch(rs) -> reads.ReadBatch:
    off = np.zeros(len(rs) + 1, dtype=np.int64)
    if rs:
        np.cumsum([len(r.letters) for r in rs], out=off[1:])
    return reads.ReadBatch(np.frombuffer(b"".join(r.letters for r in rs), dtype=np.uint8).copy(), off, [r.name for r in rs],
                           np.asarray([r.length for r in rs], dtype=np.uint32))


NOTHING, RESTART, STAYS, MOVES = range(4)           # what pool_compact does at the start of an append


class PoolModel:
    """The pool as a list.  `reads` is what the current set of arrays holds since it last started over, the first `head` of
    them taken; from the letters in front of and behind the head the model knows the branch pool_compact takes, and from
    the growth rule of the arrays (1.5 x, then 1/16 and 256 bytes on top) when `bases` is reallocated with letters in it."""

    def __init__(self):
        self.reads, self.head = [], 0
        self.cur, self.cap = 0, [0, 0]
        self.branches = [0, 0, 0, 0]
        self.doubling = 0                           # appends of more letters than are pooled, with reads pooled
        self.grown_keeping = 0                      # ... of which the letters' array had to be reallocated and copied

    @staticmethod
    def _letters(rs):
        return sum(len(r.letters) for r in rs)

    @property
    def pooled(self):
        return self.reads[self.head:]

    def sizes(self):
        p = self.pooled
        return len(p), self._letters(p), sum(len(r.name) for r in p)

    def _room(self, s, need, keep):
        if need > self.cap[s]:
            b = max(need, self.cap[s] + self.cap[s] // 2)
            self.cap[s] = b + b // 16 + 256
            return keep > 0
        return False

    def append(self, rs):
        head_base, n = self._letters(self.reads[:self.head]), len(self.reads) - self.head
        nb = self._letters(self.pooled)
        if self.head == 0:
            branch = NOTHING
        elif n == 0:
            branch, self.reads, self.head = RESTART, [], 0
        elif head_base <= nb:
            branch = STAYS
        else:
            branch, self.reads, self.head = MOVES, self.pooled, 0
            self.cur ^= 1
            self._room(self.cur, nb + 64, 0)
        self.branches[branch] += 1
        end_base, add = self._letters(self.reads), self._letters(rs)
        grown = self._room(self.cur, end_base + add + 64, end_base)
        if n > 0 and nb > 0 and add > nb:
            self.doubling += 1
            self.grown_keeping += grown
        self.reads = self.reads + list(rs)
        return branch

    def take(self, k):
        out = self.reads[self.head:self.head + k]
        assert len(out) == k
        self.head += k
        return out

    def fetch(self, first, n):
        return self.pooled[first:first + n]


def _records(rng, count: int, fasta: bool, serial: int):
    text, rs = [], []
    for i in range(count):
        L = int(rng.integers(37, 130))               # (every read has a k-mer at K = 12: no take leaves a batch without queries)
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)].tobytes()
        name = b"s%d" % (serial + i) + (b" len=%d" % L if rng.random() < 0.3 else b"")
        if fasta:
            w = int(rng.integers(10, 71))
            text.append(b">" + name + b"\n" + _wrap(seq, w))
            rs.append(Read(name.decode() + " ", seq, L + (L + w - 1) // w))
        else:
            text.append(_fastq(name, seq, rng))
            rs.append(Read(name.decode() + " ", seq, L + 1))
    return b"".join(text), rs


@functools.lru_cache(maxsize=None)
def pool_script(seed: int, n_ops: int = 170):
    """("append", text, fasta, reads) | ("take", k) | ("fetch", first, n) | ("fetch_all",), ending with the pool empty.
    Appends start small and grow, so that arrays are reallocated while they hold reads."""
    rng = np.random.default_rng(seed)
    model, ops, serial = PoolModel(), [], 0
    while len(ops) < n_ops or model.sizes()[0]:
        pooled, x = model.sizes()[0], rng.random()
        if len(ops) >= n_ops:
            op = ("take", pooled)
        elif pooled == 0 or x < 0.36:
            if pooled == 0 and x > 0.85:
                op = ("fetch", 0, 0)
            else:
                big = 1 + len(ops) * 39 // n_ops
                count = int(rng.integers(1, 4)) if rng.random() < 0.4 else int(rng.integers(max(1, big // 2), big + 1))
                fasta = bool(rng.random() < 0.5)
                text, rs = _records(rng, count, fasta, serial)
                serial += count
                op = ("append", text, fasta, tuple(rs))
        elif x < 0.72:
            how = rng.random()
            k = 1 if how < 0.2 else pooled if how < 0.45 else max(1, pooled - int(rng.integers(1, 3))) if how < 0.75 else int(rng.integers(1, pooled + 1))
            op = ("take", k)
        elif x < 0.86:
            how = rng.random()
            first = 0 if how < 0.2 else pooled if how < 0.4 else int(rng.integers(0, pooled + 1))
            n = 0 if how < 0.4 else int(rng.integers(0, pooled - first + 1))
            op = ("fetch", first, n)
        else:
            op = ("fetch_all",)
        if op[0] == "append":
            model.append(op[3])
        elif op[0] == "take":
            model.take(op[1])
        ops.append(op)
    return tuple(ops)


POOL_SEEDS = (4, 8)          # chosen for the counts tests/test_parse_corpus_cpu.py asserts from the model
