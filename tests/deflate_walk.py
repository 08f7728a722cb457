"""A walker over ONE raw deflate stream (RFC 1951) in pure Python: what a decoder sees, token by token -- for tests that ask
which code a member was written in and how wide its tokens are.  It is slow (a bit at a time): single members only.

    walk(raw) -> [Block, ...]     every block of the stream up to and including the one with BFINAL
    Block.btype                   0 stored, 1 fixed code, 2 dynamic code
    Block.litlen, Block.dist      the code lengths of a dynamic block's two codes (as many as HLIT / HDIST say); None otherwise
    Block.tokens                  (literal | length, distance, bits): distance 0 marks a literal; bits counts the token's Huffman
                                  codes and extra bits.  The end-of-block symbol is no token.  A stored block has none:
    Block.stored                  its bytes (b"" otherwise)
    expand(blocks) -> bytes       the text the tokens stand for
    kraft(lengths) -> Fraction    the code's Kraft sum (1: complete)
"""
import collections
from fractions import Fraction

Block = collections.namedtuple("Block", "btype litlen dist tokens stored")

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


def kraft(lengths):
    return sum(Fraction(1, 1 << l) for l in lengths if l)


def _decoder(lengths):
    """(length, code) -> symbol of the canonical code with these lengths"""
    count = collections.Counter(l for l in lengths if l)
    code, nxt = 0, {}
    for bits in range(1, 16):
        code = (code + count.get(bits - 1, 0)) << 1
        nxt[bits] = code
    table = {}
    for sym, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = sym
            nxt[l] += 1
    return table


class _Bits:
    def __init__(self, raw):
        self.raw, self.at = raw, 0

    def take(self, n):
        v = 0
        for i in range(n):
            if self.at >> 3 >= len(self.raw):
                raise ValueError("the stream ends inside a block")
            v |= ((self.raw[self.at >> 3] >> (self.at & 7)) & 1) << i
            self.at += 1
        return v

    def symbol(self, table):
        code = 0
        for l in range(1, 16):
            code = code << 1 | self.take(1)
            if (l, code) in table:
                return table[(l, code)], l
        raise ValueError("no code of 15 bits or fewer")


def walk(raw):
    b, blocks = _Bits(bytes(raw)), []
    while True:
        final, btype = b.take(1), b.take(2)
        if btype == 0:
            b.at = (b.at + 7) & ~7
            n, nn = b.take(16), b.take(16)
            if n ^ nn != 0xFFFF:
                raise ValueError("LEN and NLEN of a stored block disagree")
            at = b.at >> 3
            if at + n > len(b.raw):
                raise ValueError("the stream ends inside a stored block")
            blocks.append(Block(0, None, None, [], b.raw[at:at + n]))
            b.at += 8 * n
        elif btype in (1, 2):
            litlen = dist = None
            if btype == 1:
                ll, dl = FIXED_LITLEN, FIXED_DIST
            else:
                hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = b.take(3)
                clt, lens = _decoder(cl), []
                while len(lens) < hlit + hdist:
                    s, _ = b.symbol(clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        if not lens:
                            raise ValueError("a repeat with nothing before it")
                        lens += [lens[-1]] * (3 + b.take(2))
                    else:
                        lens += [0] * (3 + b.take(3) if s == 17 else 11 + b.take(7))
                if len(lens) != hlit + hdist:
                    raise ValueError("a run of lengths goes beyond the two codes")
                ll = litlen = lens[:hlit]
                dl = dist = lens[hlit:]
            lt, dt, tokens = _decoder(ll), _decoder(dl), []
            while True:
                s, bits = b.symbol(lt)
                if s < 256:
                    tokens.append((s, 0, bits))
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise ValueError("length symbol %d" % s)
                    length = LEN_BASE[s - 257] + b.take(LEN_EXTRA[s - 257])
                    d, dbits = b.symbol(dt)
                    if d > 29:
                        raise ValueError("distance symbol %d" % d)
                    distance = DIST_BASE[d] + b.take(DIST_EXTRA[d])
                    tokens.append((length, distance, bits + LEN_EXTRA[s - 257] + dbits + DIST_EXTRA[d]))
            blocks.append(Block(btype, litlen, dist, tokens, b""))
        else:
            raise ValueError("BTYPE 3")
        if final:
            return blocks


def expand(blocks):
    out = bytearray()
    for blk in blocks:
        out += blk.stored
        for v, d, _ in blk.tokens:
            if d == 0:
                out.append(v)
            else:
                if d > len(out):
                    raise ValueError("a distance reaches below the stream's first byte")
                for _ in range(v):
                    out.append(out[-d])
    return bytes(out)
