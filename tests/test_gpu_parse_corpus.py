"""The device parser (kasa_amd/csrc/kasa_parse.h) on tests/parse_corpus.py: every alignment of both gathers, line feeds on
lane, step and tile edges, every byte value, records without letters, refusals with the position `kasa_parse_status` gives,
and the pool's branches under seeded scripts.  The reference throughout is `reads.parse_reads` on the same bytes."""
import numpy as np
import pytest

from kasa_amd import capi, reads
from tests import parse_corpus as pc
from tests.test_gpu_device_parse import _assert_equal
from tests.test_gpu_device_parse_host import _run

pytestmark = pytest.mark.gpu

AFTER = b"@z\nGATTACA\n+\nIIIIIII\n"                        # the good append behind a refused one


def _T():
    return capi.parse_tile_bytes()


def _host(tmp_path, chunks):
    """`parse_reads` of every chunk, one behind the other."""
    parts = []
    for k, (text, _) in enumerate(chunks):
        p = tmp_path / f"chunk{k}.txt"
        p.write_bytes(text)
        parts.append(reads.parse_reads(str(p)))
    off = np.concatenate([[0]] + [b.offsets[1:] + sum(int(x.offsets[-1]) for x in parts[:k]) for k, b in enumerate(parts)]).astype(np.int64)
    return reads.ReadBatch(np.concatenate([b.bases for b in parts]), off, [n for b in parts for n in b.names], np.concatenate([b.lengths for b in parts]))


def _chunks(m):
    return ([(m.prefill, m.prefill_fasta)] if m.prefill else []) + [(m.text, m.fasta)]


PARSABLE = [("A", False), ("A", True), ("B", False), ("B", True), ("C", False), ("C", True), ("D", False), ("D", True), ("E", None), ("F", None)]


@pytest.mark.parametrize("g,fasta", PARSABLE, ids=[g + {None: "", False: "-fastq", True: "-fasta"}[f] for g, f in PARSABLE])
def test_parsable_members_equal_the_host_parser(g, fasta, tmp_path):
    """One append of every member (group A: behind the prefill that sets the lead of both gathers): all five arrays, and a
    range out of the middle.  Every member gets a pool of its own -- the cases the corpus claims for a text count from a
    fresh pool's lead --, closed before the next one opens."""
    assert capi.device_count() > 0, "no HIP device visible: the device parser needs a real MI355X"
    members = [m for m in pc.group(_T(), g, fasta) if m.expectation == pc.PARSABLE]
    assert members
    for m in members:
        host = _host(tmp_path, _chunks(m))
        ps = capi.Parser(0, long_sequence=m.long_sequence)
        try:
            total = 0
            for text, fa in _chunks(m):
                n, ok = ps.append(text, fa)
                assert ok, (m.name, ps.status())
                total += n
            assert total == host.n, m.name
            assert ps.sizes() == (host.n, int(host.offsets[-1]), sum(len(n) for n in host.names)), m.name
            _assert_equal(ps.fetch(), host)
            if host.n > 2:
                _assert_equal(ps.fetch(1, host.n - 2), host.slice(1, host.n - 1))
        except AssertionError as e:
            raise AssertionError(f"corpus member {m.name}") from e
        finally:
            ps.close()


@pytest.mark.parametrize("chunk_bytes", [1, 100, 4096])
def test_parse_reads_device_in_chunks(chunk_bytes, tmp_path):
    """`reads.parse_reads_device(path, 0, chunk_bytes)`: at 1 every record start is a cut."""
    assert capi.device_count() > 0 and _T() == 4096
    path = str(tmp_path / "in.txt")
    for m in pc.group(_T(), "A") + pc.group(_T(), "C"):
        with open(path, "wb") as f:
            f.write(m.text)
        host, dev = reads.parse_reads(path), reads.parse_reads_device(path, 0, chunk_bytes)
        assert dev.names == host.names and dev.fasta == host.fasta and dev.protein == host.protein, m.name
        assert np.array_equal(dev.lengths, host.lengths) and np.array_equal(dev.offsets, host.offsets) and np.array_equal(dev.bases, host.bases), m.name


def _refusals(kind):
    out = [m for m in pc.group(4096, "F") if m.expectation != pc.PARSABLE]
    pick = {"whole-vector": lambda n: n.startswith("F-whole-"), "spanning-lines": lambda n: n.startswith("F-span-"),
            "positions": lambda n: not n.startswith(("F-whole-", "F-span-"))}[kind]
    return [m for m in out if pick(m.name)]


@pytest.mark.parametrize("kind", ["whole-vector", "spanning-lines", "positions"])
def test_refusals_say_where_and_leave_the_pool_unchanged(kind, tmp_path):
    assert capi.device_count() > 0
    members = _refusals(kind)
    assert len(members) >= 20
    good = _host(tmp_path, [(pc.GOOD, False), (AFTER, False)])
    for m in members:
        at, code = pc.reported(m.expectation, m.fasta)
        ps = capi.Parser(0, long_sequence=m.long_sequence)
        try:
            assert ps.append(m.prefill, m.prefill_fasta) == (2, True)
            before, kept = ps.sizes(), ps.fetch()
            assert ps.append(m.text, m.fasta) == (0, False)
            status = ps.status()
            assert (status[0], status[2]) == (code, at), (m.name, status, m.expectation)
            assert ps.sizes() == before == (2, 12, 6)
            for x, y in zip(ps.fetch(), kept):
                assert np.array_equal(x, y)
            assert ps.append(AFTER, False) == (1, True)             # ... and lands right behind the two
            _assert_equal(ps.fetch(), good)
        except AssertionError as e:
            raise AssertionError(f"corpus member {m.name}") from e
        finally:
            ps.close()


@pytest.fixture(scope="module")
def world():
    from tests.test_gpu_parity import synthetic_world
    assert capi.device_count() > 0
    ix, _ = synthetic_world(29, 4, 3000, 1)
    dix = capi.DeviceIndex(ix)
    dev, ref = capi.Context(dix), capi.Context(dix)
    yield dev, ref
    dev.close(); ref.close(); dix.close()


@pytest.mark.parametrize("seed", pc.POOL_SEEDS)
def test_pool_scripts_against_the_list_model(seed, world):
    """Appends, takes and fetches in a seeded order: after every operation the pool's sizes are the model's, every fetch is
    the model's slice, every take encodes to the queries of the same reads uploaded from the host."""
    dev, ref = world
    model = pc.PoolModel()
    ps = capi.Parser(0)
    try:
        for step, op in enumerate(pc.pool_script(seed)):
            if op[0] == "append":
                _, text, fasta, rs = op
                assert ps.append(text, fasta) == (len(rs), True), (step, ps.status())
                model.append(rs)
            elif op[0] == "take":
                want = pc.as_batch(model.take(op[1]))
                ps.take(dev, op[1])
                dev.encode()
                ref.upload(want.bases, want.offsets)
                ref.encode()
                got_q, want_q = dev.queries(), ref.queries()
                assert want_q[0].shape[0] > 0 and len(got_q) == len(want_q) == 2
                for x, y in zip(got_q, want_q):
                    assert x.tobytes() == y.tobytes(), (step, op[1])
            elif op[0] == "fetch":
                _assert_equal(ps.fetch(op[1], op[2]), pc.as_batch(model.fetch(op[1], op[2])))
            else:
                _assert_equal(ps.fetch(), pc.as_batch(model.pooled))
            assert ps.sizes() == model.sizes(), (step, op[0])
        assert ps.sizes() == (0, 0, 0)
        with pytest.raises(RuntimeError, match="pooled"):
            ps.take(dev, 1)
    finally:
        ps.close()


def _dump_members():
    T = 4096
    safe = lambda g, fasta: [m for m in pc.group(T, g, fasta) if pc.dump_safe(m)]
    return [safe("A", True)[3], safe("A", False)[9], next(m for m in safe("C", True) if m.name == f"C-feed{T}-fasta-seq")]


@pytest.mark.parametrize("block", [None, "1500", "4099"])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["A-fasta", "A-fastq", "C"])
def test_parse_dump_device_equals_parse_dump(which, block, tmp_path):
    """The corpus through Batcher::refillDevice's own chunking, as tests/test_gpu_device_parse_host.py does for the golden files."""
    m = _dump_members()[which]
    path = str(tmp_path / "in.txt")
    with open(path, "wb") as f:
        f.write(m.text)
    env = {"KASA_READ_BLOCK": block} if block else {}
    host = _run(["parse-dump", path, "2"], env=env).stdout.split("== streamed\n")[1]
    dev = _run(["parse-dump-device", path, "2"], env=env).stdout
    assert dev.split("\n", 2)[2] == host and len(host) > 100, m.name
