"""BGZF made on the device (kasa_bgzf.h: kasa_bgzf_deflate, kasa_batch_bgzf): every gzip reader takes the stream, its members
are the blocks of 65 280 bytes in order, the same input gives the same bytes twice -- and it compresses: an always-stored
stream would pass the round trips alone."""
import ctypes as C
import os

import numpy as np
import pytest

from kasa_amd import capi, formats, reads, report
from tests import helpers
from tests.test_bgzf_cpu import BLOCK, INPUTS, PAIRS_DIR, check_stream, golden_texts

pytestmark = pytest.mark.gpu

GOLDEN_TEXTS = {os.path.basename(f): f for f in golden_texts()}
RATIO_FILES = ("out_default.json", "out_b100.jsonl", "out_w25_7.jsonl")      # the golden .json / .jsonl of 20 KB and more that the ratio is asked of by name


def _deflate_twice(data):
    stream = capi.bgzf_deflate(0, data)
    assert capi.bgzf_deflate(0, data) == stream, "a second call gives other bytes"
    return stream


@pytest.mark.parametrize("name", list(INPUTS))
def test_device_stream(name):
    assert capi.device_count() > 0
    data = INPUTS[name]
    stream = _deflate_twice(data)
    kinds = check_stream(stream, data, device=True)
    blocks = (len(data) + BLOCK - 1) // BLOCK
    assert len(kinds) == blocks
    assert len(stream) <= len(data) + 26 * blocks + 5 * blocks
    if name == "zeros":
        assert len(stream) < len(data) // 64, len(stream)
    if name in ("zeros", "period"):
        assert all(btype != 0 for btype, _ in kinds), kinds
    if name == "random70000":
        assert all(n <= 65536 for _, n in kinds)


@pytest.mark.parametrize("name", list(GOLDEN_TEXTS))
def test_device_stream_of_golden_files(name):
    assert capi.device_count() > 0
    data = open(GOLDEN_TEXTS[name], "rb").read()
    stream = _deflate_twice(data)
    kinds = check_stream(stream, data, device=True)
    blocks = (len(data) + BLOCK - 1) // BLOCK
    assert len(stream) <= len(data) + 31 * blocks
    print("%s: %d -> %d bytes (%.3f)" % (name, len(data), len(stream), len(stream) / max(1, len(data))))
    if name.endswith((".json", ".jsonl")):                               # ASCII in the fixed code: n + 2 bytes against n + 5 stored
        assert all(btype != 0 for btype, _ in kinds), kinds
        if name in RATIO_FILES:
            assert len(data) >= 20000
        if len(data) >= 20000:                                          # zlib level 1 with the fixed code: 0.25-0.30 on every one of them
            assert 2 * len(stream) <= len(data), (len(stream), len(data))


def test_the_files_the_ratio_is_asked_of_exist():
    assert all(f in GOLDEN_TEXTS for f in RATIO_FILES)


def test_tap_edges():
    lib = capi.lib()
    got = C.c_uint64(7)
    assert lib.kasa_bgzf_deflate(C.c_int(0), None, C.c_uint64(0), None, C.c_uint64(0), C.byref(got)) == 0 and got.value == 0   # an empty stream: no member
    src = np.frombuffer(INPUTS["runs"], dtype=np.uint8)
    small = np.zeros(8, dtype=np.uint8)
    rc = lib.kasa_bgzf_deflate(C.c_int(0), C.c_void_p(src.ctypes.data), C.c_uint64(src.shape[0]), C.c_void_p(small.ctypes.data), C.c_uint64(8), C.byref(got))
    assert rc == 5 and got.value > 8 and not small.any()                # KASA_E_LIMIT; says what it needs, writes nothing


@pytest.mark.parametrize("fmt", ["tsv", "json", "jsonl", "kraken"])
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
    with pytest.raises(RuntimeError, match="no text of this batch"):   # KASA_E_STATE
        ctx.batch_bgzf()
    n, nb = C.c_uint64(0), C.c_uint64(0)
    assert lib.kasa_batch_bgzf(ctx.h, C.byref(n), C.byref(nb)) == 4
    text, _, _ = ctx.text(fmt, 100, 0, batch.names, batch.lengths, best)
    assert len(text) > 3000
    whole = ctx.batch_bgzf()
    check_stream(whole, text, device=True)
    for piece in (1, 7, 4097):
        assert ctx.batch_bgzf(piece=piece) == whole, piece
    again = np.zeros(len(text), dtype=np.uint8)
    assert lib.kasa_batch_text_fetch_range(ctx.h, C.c_void_p(again.ctypes.data), C.c_uint64(0), C.c_uint64(len(text))) == 0
    assert again.tobytes() == text                                      # the text itself stays valid
    buf = np.zeros(16, dtype=np.uint8)
    assert lib.kasa_batch_bgzf_fetch_range(ctx.h, C.c_void_p(buf.ctypes.data), C.c_uint64(len(whole) - 8), C.c_uint64(16)) != 0   # beyond the end
    ctx.close()
    dix.close()
