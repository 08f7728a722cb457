"""A deflate WRITER for the tests of the device inflater (tests/inflate_corpus.py: built_cases): RFC 1951 payloads made by
construction -- an LSB-first bit writer, canonical codes from a list of code lengths, the length and distance tables, and
fixed / stored / dynamic blocks whose every choice is the caller's (the code lengths, HLIT / HDIST / HCLEN, the code-length
code, the exact 0-15 / 16 / 17 / 18 sequence of the header).  zlib's compressor uses a narrow part of the format; this one
writes the rest.  No product code imports it.

A token is
    b                          a literal byte (int, 0..255)
    (length, distance)         a match, 3..258 and 1..32768
    (258, distance, AS_284)    length 258 written as symbol 284 with extra bits 31
    ("L", symbol[, extra])     a literal/length symbol by number, as it stands (its extra bits too when it has some)
    ("D", symbol[, extra])     a distance symbol by number
    ("B", value, nbits)        bits as they stand
the last three for members that have to be rejected.  expand(tokens) is the text of the first three.

Payload keeps, per block it wrote, what the block really holds (symbols, code lengths of the symbols used, extra bits at
their ends, the header's sequence, where the block begins, every match with its token index): the record the corpus' own
coverage test walks."""

AS_284 = "as 284+31"

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_L = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
MAX_PAYLOAD = 65536 - 18 - 8                      # what BSIZE can state
assert len(LEN_BASE) == len(LEN_EXTRA) == 29 and len(DIST_BASE) == len(DIST_EXTRA) == 30
assert all(LEN_BASE[i] + (1 << LEN_EXTRA[i]) == LEN_BASE[i + 1] for i in range(27)) and LEN_BASE[27] + 31 == 258
assert all(DIST_BASE[i] + (1 << DIST_EXTRA[i]) == DIST_BASE[i + 1] for i in range(29)) and DIST_BASE[29] + (1 << 13) - 1 == 32768


def length_symbol(length):
    """(index of the length symbol: symbol - 257, value of its extra bits); 258 is symbol 285"""
    assert 3 <= length <= 258
    i = max(k for k in range(29) if LEN_BASE[k] <= length)
    return i, length - LEN_BASE[i]


def distance_symbol(dist):
    assert 1 <= dist <= 32768
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, dist - DIST_BASE[i]


_LEN_SYM = [None] * 3 + [length_symbol(n) for n in range(3, 259)]


def canonical(lengths):
    """the canonical codes (RFC 1951 3.2.2) of a list of code lengths; 0 where the length is 0"""
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for n in lengths:
        out.append(nxt[n] if n else 0)
        if n:
            nxt[n] += 1
    return out


def kraft(lengths):
    """sum of 2^-length in units of 2^-15: 32768 is a complete code"""
    return sum(1 << (15 - n) for n in lengths if n)


def random_code(rng, n, max_len=15):
    """the lengths of a random COMPLETE code of n symbols, none longer than max_len: random leaves of depth below max_len
    are split until there is a leaf per symbol.  (One symbol: the one-bit code, which deflate allows incomplete.)"""
    assert 1 <= n <= 1 << max_len
    if n == 1:
        return [1]
    leaves = [1, 1]
    while len(leaves) < n:
        i = rng.choice([k for k, d in enumerate(leaves) if d < max_len])
        leaves[i] += 1
        leaves.append(leaves[i])
    rng.shuffle(leaves)
    assert kraft(leaves) == 32768
    return leaves


def flat_code(n):
    """the lengths of a complete code of n >= 2 symbols whose lengths differ by at most one"""
    k = n.bit_length() - 1
    short = (2 << k) - n
    return [k] * short + [k + 1] * (n - short) if n > (1 << k) else [k] * n


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif isinstance(t[0], int):
            length, dist = t[0], t[1]
            assert dist <= len(out)
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out)


def text_len(tokens):
    return sum(1 if isinstance(t, int) else t[0] if isinstance(t[0], int) else 0 for t in tokens)


def used_symbols(tokens):
    """(literal/length symbols, distance symbols) the tokens need codes for, 256 among them"""
    ls, ds = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            ls.add(t)
        elif isinstance(t[0], int):
            ls.add(257 + (27 if len(t) > 2 else _LEN_SYM[t[0]][0]))
            ds.add(distance_symbol(t[1])[0])
        elif t[0] == "L":
            ls.add(t[1])
        elif t[0] == "D":
            ds.add(t[1])
    return ls, ds


def rle_items(seq, mode="greedy", rng=None):
    """a dynamic header's sequence for the lengths `seq`: [(symbol, repeat)] with repeat 1 for 0..15.
    "none": no repeats; "greedy": the longest repeat wherever one fits; "random": any legal choice, by rng"""
    items, i, n = [], 0, len(seq)
    while i < n:
        v, run = seq[i], 1
        while i + run < n and seq[i + run] == v:
            run += 1
        options = [(v, 1)]
        if mode != "none":
            if v == 0 and run >= 3:
                options.append((17, min(run, 10)))
            if v == 0 and run >= 11:
                options.append((18, min(run, 138)))
            if i > 0 and seq[i - 1] == v and run >= 3:
                options.append((16, min(run, 6)))
        if mode == "random":
            sym, top = rng.choice(options)
            rep = 1 if sym < 16 else rng.randint({16: 3, 17: 3, 18: 11}[sym], top)
        else:
            sym, rep = max(options, key=lambda o: o[1])
        items.append((sym, rep))
        i += rep
    return items


def items_expand(items):
    out = []
    for sym, rep in items:
        if sym < 16:
            out.append(sym)
        elif sym == 16:
            out += [out[-1]] * rep
        else:
            out += [0] * rep
    return out


class BitWriter:
    """bits in the order deflate packs them: the first bit is the lowest of the first byte"""

    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, n):
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """a Huffman code: its first bit is its HIGHEST"""
        self.bits(int(format(code, "0%db" % n)[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    @property
    def bitpos(self):
        return 8 * len(self.buf) + self.n

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


class Payload:
    """one deflate stream, block after block"""

    def __init__(self):
        self.w = BitWriter()
        self.blocks = []
        self.pos = 0                              # text bytes so far

    def getvalue(self):
        return self.w.getvalue()

    def _begin(self, kind, final):
        rec = dict(kind=kind, final=int(bool(final)), bit=self.w.bitpos, text_at=self.pos, lsyms=set(), dsyms=set(), llens=set(), dlens=set(),
                   lext=set(), dext=set(), matches=[], ntok=0)
        self.blocks.append(rec)
        self.w.bits(rec["final"], 1)
        self.w.bits({"stored": 0, "fixed": 1, "dynamic": 2}[kind], 2)
        return rec

    def stored(self, data, final, length=None):
        """length: the LEN field where it is not to be len(data)"""
        rec = self._begin("stored", final)
        self.w.align()
        n = len(data) if length is None else length
        self.w.bits(n, 16)
        self.w.bits(n ^ 0xFFFF, 16)
        rec["data_at"] = self.w.bitpos // 8
        self.w.buf += data
        self.pos += len(data)
        rec["end_bit"] = self.w.bitpos
        return self

    def fixed(self, tokens, final, eob=True):
        rec = self._begin("fixed", final)
        self._body(rec, tokens, FIXED_L, FIXED_D, eob)
        return self

    def dynamic(self, tokens, litlen_lengths, dist_lengths, final, hclen=None, cl_lengths=None, rle="greedy", rng=None, body=True, eob=True, check=True):
        """rle: "none" / "greedy" / "random" (with rng), or the sequence itself as [(symbol, repeat)] (repeat 1 for 0..15).
        check=False: for headers that are wrong on purpose (the sequence need not give the lengths, nor the counts be legal)"""
        seq = list(litlen_lengths) + list(dist_lengths)
        hlit, hdist = len(litlen_lengths), len(dist_lengths)
        items = rle_items(seq, rle, rng) if isinstance(rle, str) else [tuple(i) for i in rle]
        if cl_lengths is None:
            used = sorted({s for s, _ in items})
            if len(used) == 1:
                used.append(0 if used[0] else 1)                  # the code-length code has to be complete: a second, unused code
            cl_lengths = [0] * 19
            for s, n in zip(used, flat_code(len(used))):
                cl_lengths[s] = n
        if hclen is None:
            hclen = max([4] + [k + 1 for k, s in enumerate(CL_ORDER) if cl_lengths[s]])
        if check:
            assert 257 <= hlit <= 286 and 1 <= hdist <= 30 and items_expand(items) == seq
            assert kraft(cl_lengths) == 32768 and max(cl_lengths) <= 7 and all(cl_lengths[s] == 0 for s in CL_ORDER[hclen:])
        assert 257 <= hlit <= 288 and 1 <= hdist <= 32 and 4 <= hclen <= 19
        rec = self._begin("dynamic", final)
        w = self.w
        w.bits(hlit - 257, 5)
        w.bits(hdist - 1, 5)
        w.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.bits(cl_lengths[s], 3)
        codes = canonical(cl_lengths)
        at, placed = 0, []
        for sym, rep in items:
            assert cl_lengths[sym], "the code-length code has no code for %d" % sym
            w.code(codes[sym], cl_lengths[sym])
            if sym == 16:
                w.bits(rep - 3, 2)
            elif sym == 17:
                w.bits(rep - 3, 3)
            elif sym == 18:
                w.bits(rep - 11, 7)
            placed.append((sym, rep, at))
            at += rep
        rec.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_lengths=list(cl_lengths), items=placed, header_end_bit=w.bitpos)
        if body:
            self._body(rec, tokens, list(litlen_lengths), list(dist_lengths), eob)
        rec["end_bit"] = w.bitpos
        return self

    def _body(self, rec, tokens, llens, dlens, eob):
        w = self.w
        # (the codes bit-reversed once per block: a Huffman code goes out highest bit first)
        lcodes = [int(format(c, "0%db" % n)[::-1], 2) if n else 0 for c, n in zip(canonical(llens), llens)]
        dcodes = [int(format(c, "0%db" % n)[::-1], 2) if n else 0 for c, n in zip(canonical(dlens), dlens)]

        def lsym(s):
            assert s < len(llens) and llens[s], "no code for literal/length symbol %d" % s
            w.bits(lcodes[s] & ((1 << llens[s]) - 1), llens[s])
            rec["lsyms"].add(s)
            rec["llens"].add(llens[s])

        def dsym(s):
            assert s < len(dlens) and dlens[s], "no code for distance symbol %d" % s
            w.bits(dcodes[s] & ((1 << dlens[s]) - 1), dlens[s])
            rec["dsyms"].add(s)
            rec["dlens"].add(dlens[s])

        for k, t in enumerate(tokens):
            if isinstance(t, int):
                lsym(t)
                self.pos += 1
            elif isinstance(t[0], int):
                length, dist = t[0], t[1]
                assert 1 <= dist <= self.pos, "a distance beyond the text so far is written with (\"D\", ...)"
                li, le = (27, 31) if len(t) > 2 else _LEN_SYM[length]
                assert len(t) == 2 or (length == 258 and t[2] == AS_284)
                rec["matches"].append((k, w.bitpos, self.pos, length, dist))
                lsym(257 + li)
                w.bits(le, LEN_EXTRA[li])
                di, de = distance_symbol(dist)
                dsym(di)
                w.bits(de, DIST_EXTRA[di])
                for e, what, ext in ((le, ("L", 257 + li), LEN_EXTRA[li]), (de, ("D", di), DIST_EXTRA[di])):
                    if e == 0:
                        rec["lext" if what[0] == "L" else "dext"].add((what[1], "min"))
                    if e == (1 << ext) - 1:
                        rec["lext" if what[0] == "L" else "dext"].add((what[1], "max"))
                self.pos += length
            elif t[0] == "L":
                lsym(t[1])
                if 257 <= t[1] <= 285:
                    w.bits(t[2] if len(t) > 2 else 0, LEN_EXTRA[t[1] - 257])
            elif t[0] == "D":
                dsym(t[1])
                if t[1] < 30:
                    w.bits(t[2] if len(t) > 2 else 0, DIST_EXTRA[t[1]])
            else:
                assert t[0] == "B"
                w.bits(t[1], t[2])
        rec["ntok"] = len(tokens)
        rec["last_token_end_bit"] = w.bitpos
        if eob:
            lsym(256)
        rec["end_bit"] = w.bitpos


def code_for(rng, symbols, size, max_len=15):
    """code lengths over `size` symbols: a random complete code on `symbols`, 0 elsewhere"""
    symbols = sorted(symbols)
    lens = [0] * size
    for s, n in zip(symbols, random_code(rng, len(symbols), max_len)):
        lens[s] = n
    return lens


def random_dynamic(p, rng, tokens, final, hlit=None, hdist=None):
    """one dynamic block of `tokens` into Payload p with random complete codes (to 15 bits) on exactly the symbols used, a
    random complete code-length code (to 7 bits) and a random legal run-length coding of the header.  hlit / hdist: the
    counts to state (default: the smallest that hold the symbols)"""
    ls, ds = used_symbols(tokens)
    hlit = max(257, max(ls) + 1) if hlit is None else hlit
    hdist = max(1, max(ds) + 1 if ds else 1) if hdist is None else hdist
    llens = code_for(rng, ls, hlit)
    dlens = code_for(rng, ds, hdist) if ds else [0] * hdist
    mode = rng.choice(["none", "greedy", "random", "random"])
    items = rle_items(llens + dlens, mode, rng)
    used = sorted({s for s, _ in items})
    if len(used) == 1:
        used.append(0 if used[0] else 1)
    cl = [0] * 19
    for s, n in zip(used, random_code(rng, len(used), 7)):
        cl[s] = n
    p.dynamic(tokens, llens, dlens, final, cl_lengths=cl, rle=items)
    return p


def random_tokens(rng, size, literals, len_syms, dist_syms, start=0):
    """tokens for `size` bytes of text behind `start` bytes: literals from `literals`, matches whose length and distance
    symbols come from the two subsets, with random extra bits"""
    out, n = [], 0
    while n < size:
        pos = start + n
        ok_d = [d for d in dist_syms if DIST_BASE[d] <= pos]
        ok_l = [s for s in len_syms if LEN_BASE[s] <= size - n]
        if ok_d and ok_l and rng.random() < 0.5:
            li, di = rng.choice(ok_l), rng.choice(ok_d)
            length = min(LEN_BASE[li] + rng.randrange(1 << LEN_EXTRA[li]), size - n, 258)
            dist = min(DIST_BASE[di] + rng.randrange(1 << DIST_EXTRA[di]), pos)
            out.append((length, dist))
            n += length
        else:
            out.append(rng.choice(literals))
            n += 1
    return out


def tokens_of_text(rng, text, p_match=0.5):
    """`text` as literals and random back-references into itself: at a position whose four bytes occurred before, one of
    the earlier places (any of them, not the nearest) is taken with probability p_match, up to a random length"""
    seen, out, i, n = {}, [], 0, len(text)
    while i < n:
        key = text[i:i + 4]
        places = seen.get(key)
        step = 1
        if places and len(key) == 4 and rng.random() < p_match:
            j = rng.choice(places)
            cap, length = rng.choice([3, 8, 40, 258]), 0
            while length < cap and i + length < n and text[j + length] == text[i + length]:
                length += 1
            if length >= 3 and i - j <= 32768:
                out.append((length, i - j))
                step = length
        if step == 1:
            out.append(text[i])
        for k in range(i, i + step):
            seen.setdefault(text[k:k + 4], []).append(k)
        i += step
    assert expand(out) == text
    return out


def split_blocks(rng, tokens, nblocks):
    """the token list cut into nblocks runs (some may be empty)"""
    cuts = sorted(rng.randint(0, len(tokens)) for _ in range(nblocks - 1))
    return [tokens[a:b] for a, b in zip([0] + cuts, cuts + [len(tokens)])]
