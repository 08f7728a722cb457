"""bench.py's --dump-outputs on the host: the rows of the seeded sample are gathered from the CSR exactly, the files are
float32 / float64, and a CSR too large for the size limit is cut to a prefix of the sample that fits."""
import numpy as np

import bench


class _Ctx:
    """What dump_outputs asks of a capi.Context: profile() and scores()."""

    def __init__(self, n_reads, seed=5):
        rng = np.random.default_rng(seed)
        lens = rng.integers(0, 40, n_reads)
        self.off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
        nnz = int(self.off[-1])
        self.tax = rng.integers(1, 1400, nnz).astype(np.uint32)
        self.sc = rng.random(nnz).astype(np.float32)
        self.prof = (rng.random((6, 9)), rng.integers(0, 1 << 40, (6, 9)).astype(np.uint64),
                     rng.integers(0, 1 << 40, (6, 9)).astype(np.uint64))

    def profile(self):
        return self.prof

    def scores(self):
        return self.off, self.tax, self.sc


def _load(d):
    return {f.name[:-4]: np.load(f) for f in d.iterdir()}


def test_dump_outputs_gathers_the_sampled_rows(tmp_path):
    ctx = _Ctx(50_000)
    bench.dump_outputs(ctx, str(tmp_path / "a"), True)
    got = _load(tmp_path / "a")
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["profile_count_all"], ctx.prof[0]) and np.array_equal(got["profile_count_unique"], ctx.prof[1].astype(np.float64))
    pick = got["scores_read"].astype(np.int64)
    assert pick.shape[0] == bench.DUMP_SAMPLE_READS and np.all(np.diff(pick) > 0)
    at = np.concatenate([np.arange(int(ctx.off[i]), int(ctx.off[i + 1])) for i in pick])
    assert np.array_equal(got["scores_row_length"], (ctx.off[pick + 1] - ctx.off[pick]).astype(np.float64))
    assert np.array_equal(got["scores_taxon"], ctx.tax[at].astype(np.float64)) and np.array_equal(got["scores_value"], ctx.sc[at])
    assert got["scores_batch"][0] == 50_000 and got["scores_batch"][1] == ctx.tax.shape[0]
    bench.dump_outputs(ctx, str(tmp_path / "b"), True)                   # the same sample every time
    again = _load(tmp_path / "b")
    assert all(np.array_equal(got[k], again[k]) for k in got)


def test_dump_outputs_stays_within_its_size_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    ctx = _Ctx(200_000)
    bench.dump_outputs(ctx, str(tmp_path), True)
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= 1 << 20
    got = _load(tmp_path)
    n = got["scores_read"].shape[0]
    assert 0 < n < bench.DUMP_SAMPLE_READS and got["scores_taxon"].shape[0] == got["scores_row_length"].sum()
    order = np.random.default_rng(bench.DUMP_SEED).permutation(200_000)[:n]   # a prefix of the seeded sample
    assert np.array_equal(np.sort(order), got["scores_read"].astype(np.int64))


def test_dump_outputs_profile_only(tmp_path):
    bench.dump_outputs(_Ctx(100), str(tmp_path), False)
    assert sorted(f.name for f in tmp_path.iterdir()) == ["profile_count_all.npy", "profile_count_total.npy", "profile_count_unique.npy"]
