"""tests/deflate_walk.py against zlib (no device): the walker reads what `zlib.compressobj(1, zlib.DEFLATED, -15)` writes of
every BGZF test input, its tokens expand to the input, and it says of each block what zlib says of the stream."""
import zlib
from fractions import Fraction

import pytest

from tests import deflate_walk
from tests.test_bgzf_cpu import INPUTS


def _raw(data, level=1, strategy=zlib.Z_DEFAULT_STRATEGY):
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return z.compress(data) + z.flush()


@pytest.mark.parametrize("name", list(INPUTS))
def test_tokens_expand_to_the_input(name):
    data = INPUTS[name]
    raw = _raw(data)
    blocks = deflate_walk.walk(raw)
    assert deflate_walk.expand(blocks) == data
    assert blocks and all(b.btype in (0, 1, 2) for b in blocks)
    for b in blocks:
        if b.btype == 2:
            assert 257 <= len(b.litlen) <= 286 and 1 <= len(b.dist) <= 30
            assert max(b.litlen) <= 15 and max(b.dist) <= 15
            assert deflate_walk.kraft(b.litlen) == 1                    # zlib's literal/length code is complete
            assert deflate_walk.kraft(b.dist) <= 1
        else:
            assert b.litlen is None and b.dist is None
        for v, d, bits in b.tokens:
            assert (0 <= v <= 255 and 1 <= bits <= 15) if d == 0 else (3 <= v <= 258 and 1 <= d <= 32768 and 2 <= bits <= 48)


def test_block_types_and_bit_counts():
    text = INPUTS["text65280"]
    fixed = deflate_walk.walk(_raw(text, 1, zlib.Z_FIXED))
    assert [b.btype for b in fixed] == [1] * len(fixed) and deflate_walk.expand(fixed) == text
    assert all(bits in (8, 9) for b in fixed for _, d, bits in b.tokens if d == 0)
    stored = deflate_walk.walk(_raw(INPUTS["random70000"], 0))
    assert {b.btype for b in stored} == {0} and b"".join(b.stored for b in stored) == INPUTS["random70000"]
    # the bits of all tokens, the end-of-block symbols and the headers are the stream: a dynamic stream of one block
    raw = _raw(text[:3000], 9)
    blk, = deflate_walk.walk(raw)
    assert blk.btype == 2
    body = sum(bits for _, _, bits in blk.tokens) + blk.litlen[256]
    assert body < 8 * len(raw) and 8 * len(raw) - body < 8 * 200         # what is left is the block's header (and the padding)


def test_kraft_and_errors():
    assert deflate_walk.kraft([1, 2, 3, 3]) == 1 and deflate_walk.kraft([2, 2, 0, 2]) == Fraction(3, 4)
    with pytest.raises(ValueError):
        deflate_walk.walk(b"\x07")                                      # BFINAL = 1, BTYPE = 3
    with pytest.raises(ValueError):
        deflate_walk.walk(_raw(INPUTS["runs"])[:-3])                    # cut
