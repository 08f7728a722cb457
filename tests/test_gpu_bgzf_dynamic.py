"""BGZF made on the device with a Huffman table per stream (kasa_bgzf.h: KASA_BGZF_DYNAMIC, kasa_bgzf_deflate_coded,
kasa_ctx_set_bgzf_code): every gzip reader and the device's own inflater take the stream, the tokens are the fixed code's, both
codes are complete and within 15 bits -- also where a block outside the counted sample uses symbols the sample never saw and
tokens wider than 32 bits -- and the stream is a fifth smaller at least than the fixed code's."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from kasa_amd import capi, formats, reads, report
from tests import deflate_walk
from tests.test_bgzf_cpu import BLOCK, INPUTS, PAIRS_DIR, check_stream, golden_texts

pytestmark = pytest.mark.gpu

FIXED, DYNAMIC = capi.BGZF_FIXED, capi.BGZF_DYNAMIC
GOLDEN_TEXTS = {os.path.basename(f): f for f in golden_texts()}
RATIO_FILES = ("out_default.json", "out_b100.jsonl", "out_w25_7.jsonl")
SAMPLE = 64                                                             # kasa_bgzf.h: every block up to 64, else blocks j * nBlk // 64


def _texts():
    d = dict(INPUTS)
    for name, path in GOLDEN_TEXTS.items():
        d[name] = open(path, "rb").read()
    return d


TEXTS = _texts()


def _member(stream, i):
    """the raw deflate stream of member i"""
    return [payload for _, payload, _, _ in formats.bgzf_members(stream)][i]


@pytest.mark.parametrize("name", list(TEXTS))
def test_dynamic_stream(name):
    assert capi.device_count() > 0
    data = TEXTS[name]
    stream = capi.bgzf_deflate(0, data, DYNAMIC)
    assert capi.bgzf_deflate(0, data, DYNAMIC) == stream, "a second call gives other bytes"
    kinds = check_stream(stream, data, device=True)
    blocks = (len(data) + BLOCK - 1) // BLOCK
    assert len(kinds) == blocks
    assert len(stream) <= len(data) + 31 * blocks                       # the give-up rule: no member beyond its stored form
    if data:
        text, status, member = capi.bgzf_inflate(0, stream)
        assert (status, member) == (0, 0) and text == data
    if name in ("len1", "len2", "len3", "len4"):
        assert len(stream) <= len(capi.bgzf_deflate(0, data, FIXED))
    if name.startswith("text") or name in RATIO_FILES:                  # per-read text of a block and more: every full block has the table
        assert all(btype == 2 for (btype, _), at in zip(kinds, range(0, len(data), BLOCK)) if len(data) - at >= 2048), kinds


@pytest.mark.parametrize("name", list(INPUTS))
def test_fixed_unchanged(name):
    data = INPUTS[name]
    src = np.frombuffer(data, dtype=np.uint8)
    cap = len(data) + 31 * ((len(data) + BLOCK - 1) // BLOCK)
    out, got = np.zeros(max(1, cap), dtype=np.uint8), C.c_uint64(0)
    rc = capi.lib().kasa_bgzf_deflate(C.c_int(0), C.c_void_p(src.ctypes.data) if len(data) else None, C.c_uint64(len(data)), C.c_void_p(out.ctypes.data),
                                      C.c_uint64(cap), C.byref(got))
    assert rc == 0
    assert capi.bgzf_deflate(0, data, FIXED) == out[:got.value].tobytes()


def test_tap_takes_two_codes_only():
    got = C.c_uint64(0)
    assert capi.lib().kasa_bgzf_deflate_coded(C.c_int(0), C.c_int(2), None, C.c_uint64(0), None, C.c_uint64(0), C.byref(got)) == 1   # KASA_E_ARG
    assert capi.bgzf_deflate(0, b"", DYNAMIC) == b""


@pytest.mark.parametrize("name", ["text65280", "out_b100.tsv"])
def test_same_tokens(name):
    data = TEXTS[name]
    fixed, = deflate_walk.walk(_member(capi.bgzf_deflate(0, data, FIXED), 0))
    dynamic, = deflate_walk.walk(_member(capi.bgzf_deflate(0, data, DYNAMIC), 0))
    assert fixed.btype == 1 and dynamic.btype == 2
    assert [(v, d) for v, d, _ in dynamic.tokens] == [(v, d) for v, d, _ in fixed.tokens]      # the matcher did not change, only the code
    assert deflate_walk.expand([dynamic]) == data[:BLOCK]
    assert len(dynamic.litlen) == 286 and len(dynamic.dist) == 30
    for lengths in (dynamic.litlen, dynamic.dist):
        assert deflate_walk.kraft(lengths) == 1 and 1 <= min(lengths) and max(lengths) <= 15


@pytest.mark.parametrize("name", RATIO_FILES + ("text195857",))
def test_ratio(name):
    data = TEXTS[name]
    fixed, dynamic = capi.bgzf_deflate(0, data, FIXED), capi.bgzf_deflate(0, data, DYNAMIC)
    print("%s: %d bytes -> fixed %d (%.3f), dynamic %d (%.3f): %.3f of fixed" % (name, len(data), len(fixed), len(fixed) / len(data), len(dynamic),
                                                                                 len(dynamic) / len(data), len(dynamic) / len(fixed)))
    assert len(data) >= 20000
    assert len(dynamic) <= 0.80 * len(fixed), (len(dynamic), len(fixed))


# ---- blocks outside the sample, 15-bit codes, tokens beyond 32 bits ----
SKEW = bytes([ord("a")] * 230 + [ord("c")] * 21 + [ord("g")] * 4 + [ord("t")])       # a byte -> a letter: 89.8 / 8.2 / 1.6 / 0.4 %
SEED, N_BLOCKS = 11, 130


def _skewed(n, seed):
    return random.Random(seed).randbytes(n).translate(SKEW)


def _text_with_an_unsampled_block():
    """130 blocks of letters from a skewed alphabet of four; the first block outside the counted sample is replaced by
    all 256 byte values, 20 000 letters, 18 more times the byte values (4608 bytes) and a copy of the first 10 000 letters
    24 608 bytes behind their original, then letters to the block's end."""
    text = bytearray(_skewed(N_BLOCKS * BLOCK, SEED))
    sampled = {j * N_BLOCKS // SAMPLE for j in range(SAMPLE)}
    special = next(i for i in range(N_BLOCKS) if i not in sampled)
    letters = _skewed(20000, SEED + 1)
    block = bytes(range(256)) + letters + bytes(range(256)) * 18 + letters[:10000]
    block += _skewed(BLOCK - len(block), SEED + 2)
    text[special * BLOCK:(special + 1) * BLOCK] = block
    return bytes(text), special


def test_unsampled_block_long_codes_wide_tokens():
    """The sampled blocks hold some 430 000 tokens of four literals, short lengths and near distances, so the symbols that
    keep their floor count of 1 -- 252 literals, the long lengths -- end at the limit of 15 bits.  The one block that uses them
    is not counted.  A restatement of the matcher and the table build in Python gives for this seed: that member coded in
    11 021 bytes (stored: 65 311), a longest code of 15 bits, and three tokens wider than 32 bits -- length 256 at distance
    20 256 (15 + 5 + 10 + 13 = 43 bits: the byte values found again behind the letters) and twice length 258 at distance 24 608
    (38 bits: the copy, where a 4-gram of its first 1024 bytes stands nowhere else before it)."""
    data, special = _text_with_an_unsampled_block()
    assert len(data) == N_BLOCKS * BLOCK and special == 1
    stream = capi.bgzf_deflate(0, data, DYNAMIC)
    kinds = check_stream(stream, data, device=True)
    assert len(kinds) == N_BLOCKS
    blk, = deflate_walk.walk(_member(stream, special))
    assert blk.btype in (0, 2)
    assert blk.btype == 2, "the block outside the sample came out stored: the wide tokens were not reached -- change SEED or the mix"
    assert deflate_walk.kraft(blk.litlen) == 1 and deflate_walk.kraft(blk.dist) == 1
    assert max(blk.litlen + blk.dist) == 15
    wide = [(v, d, bits) for v, d, bits in blk.tokens if bits > 32]
    print("tokens of more than 32 bits:", wide)
    assert wide, "no token of more than 32 bits: change SEED or the mix"
    assert any(d > 16384 for _, d, _ in wide) and max(bits for _, _, bits in blk.tokens) <= 48
    assert any(bits == 15 for _, d, bits in blk.tokens if d == 0)      # literals the sample never saw


# ---- through a context ----
@pytest.mark.parametrize("fmt", ["jsonl", "tsv"])
def test_through_a_context(fmt):
    assert capi.device_count() > 0
    lib = capi.lib()
    ix = formats.load_index(os.path.join(PAIRS_DIR, "idx"), os.path.join(PAIRS_DIR, "content.txt"))
    batch = reads.parse_reads(os.path.join(PAIRS_DIR, "reads.fastq"))
    dix = capi.DeviceIndex(ix)
    ctx = capi.Context(dix, 12, 7, 3)
    ctx.run_batch(batch.bases, batch.offsets, True)
    den, rclass = report.rank_denominators(ix.freq_at(12), batch.lengths, ix.K, False)
    best = np.array([report.best_score(int(L), 12, 7, 3, False) for L in np.unique(batch.lengths)], dtype=np.float32)
    ctx.rank(den, rclass, 0.0, 100)
    ctx.set_taxa_text(ix.content.taxids, ix.content.names)
    text, _, _ = ctx.text(fmt, 100, 0, batch.names, batch.lengths, best)
    assert len(text) > 3000
    today = ctx.batch_bgzf()
    assert today == capi.bgzf_deflate(0, text, FIXED)
    ctx.set_bgzf_code(DYNAMIC)
    whole = ctx.batch_bgzf()
    kinds = check_stream(whole, text, device=True)
    assert whole == capi.bgzf_deflate(0, text, DYNAMIC) and kinds[0][0] == 2 and len(whole) < len(today)
    for piece in (1, 7, 4097):
        assert ctx.batch_bgzf(piece=piece) == whole, piece
    again = np.zeros(len(text), dtype=np.uint8)
    assert lib.kasa_batch_text_fetch_range(ctx.h, C.c_void_p(again.ctypes.data), C.c_uint64(0), C.c_uint64(len(text))) == 0
    assert again.tobytes() == text                                      # the text itself stays valid
    assert lib.kasa_ctx_set_bgzf_code(ctx.h, C.c_int(2)) == 1           # KASA_E_ARG
    with pytest.raises(RuntimeError):
        ctx.set_bgzf_code(-1)
    assert ctx.batch_bgzf() == whole                                    # a refused code leaves the context's
    ctx.set_bgzf_code(FIXED)
    assert ctx.batch_bgzf() == today
    ctx.close()
    dix.close()
