"""The stage and kernel timers of a context (kasa_ctx_stage_ms, kasa_ctx_kernel_ms, kasa_ctx_stage_reset): which spans one
batch closes, that every closed span took time, that a second batch closes the same ones again, and that the kernels timed
inside a stage take no longer than the stage.

The tables hold the counts of the commit before the host glue was refactored (spans became scoped objects there): they were
taken by running this file's `measure()` on a build of that commit, on an MI355X."""
import os

import pytest

from kasa_amd import capi, reads
from tests import helpers
from tests.test_gpu_parity import _gpu_or_fail

pytestmark = pytest.mark.gpu

# launches of one run_batch(..., True) of tests/golden/pairs/reads.fastq: {stage: n}, {kernel: n}
NARROW = ("idx", 12, 7,                                                    # 32-byte records, six levels
          {"encode": 1, "sort": 1, "lookup": 1, "group": 2, "regroup": 0, "score": 2},
          {"lookup_tile_kernel": 1, "group_kernel": 1, "score_main_kernel": 1, "score_other_kernel": 1, "row_merge_kernel": 1,
           "score_general_kernels": 1, "profile_table_kernels": 1, "row_copy_kernels": 1, "sort_pass_kernels": 1,
           "bucket_rank_kernel": 1, "score_dense_kernel": 1, "score_replay_kernels": 1})
WIDE = ("idx25", 25, 7,                                                    # 64-byte records, nineteen levels
        {"encode": 1, "sort": 1, "lookup": 1, "group": 2, "regroup": 0, "score": 2},
        {"lookup_tile_kernel": 1, "group_kernel": 1, "score_main_kernel": 1, "score_other_kernel": 1, "row_merge_kernel": 1,
         "score_general_kernels": 1, "profile_table_kernels": 2, "row_copy_kernels": 1, "sort_pass_kernels": 1,
         "bucket_rank_kernel": 1, "score_dense_kernel": 0, "score_replay_kernels": 1})

# kernel spans that lie inside a stage's span
INSIDE = {"score": ("score_main_kernel", "score_other_kernel", "row_merge_kernel", "score_general_kernels", "score_dense_kernel",
                    "score_replay_kernels", "row_copy_kernels"),
          "group": ("group_kernel", "profile_table_kernels")}
# ms by which the kernels of a stage may exceed the stage.  Measured on the commit before the refactor: the largest excess over
# the two batches of this test, both stages, in 20 fresh contexts was none -- the sums stayed below their stage by at least
# 0.13 ms (score) and 0.02 ms (group): the spans between the kernels' own are never empty -- so: zero.
SLACK_MS = 0.0


def _case(stem, k_high, k_low):
    _gpu_or_fail()
    d, ix = helpers.load_case("pairs", stem)
    batch = reads.parse_reads(os.path.join(d, "reads.fastq"))
    return capi.Context(capi.DeviceIndex(ix), k_high, k_low, 3), batch


def _launches(table):
    return {name: n for name, (_, n) in table.items()}


def _excess(ctx):
    """per stage of INSIDE: the time of the kernels inside it minus the stage's own"""
    st, kn = ctx.stage_ms(), ctx.kernel_ms()
    return {stage: sum(kn[k][0] for k in inside) - st[stage][0] for stage, inside in INSIDE.items()}


def measure(repeats=20):
    """What the tables and SLACK_MS above are taken from (not a test)."""
    for stem, k_high, k_low, _, _ in (NARROW, WIDE):
        worst = 0.0
        for rep in range(repeats):
            ctx, batch = _case(stem, k_high, k_low)
            ctx.stage_reset()
            for b in range(2):
                ctx.run_batch(batch.bases, batch.offsets, True)
                if rep == 0 and b == 0:
                    print(stem, "stages", _launches(ctx.stage_ms()))
                    print(stem, "kernels", _launches(ctx.kernel_ms()))
                    print(stem, "ms", ctx.stage_ms(), ctx.kernel_ms())
                if stem == NARROW[0]:           # (wide records: one of the two table spans lies in the score stage, INSIDE is not theirs)
                    ex = _excess(ctx)
                    print(stem, "rep", rep, "batch", b, "excess", ex)
                    worst = max(worst, max(ex.values()))
        print(stem, "largest excess", worst)


def test_reset_clears_every_timer():
    ctx, batch = _case(*NARROW[:3])
    ctx.run_batch(batch.bases, batch.offsets, True)
    ctx.stage_reset()
    assert set(ctx.stage_ms().values()) == {(0.0, 0)}
    assert set(ctx.kernel_ms().values()) == {(0.0, 0)}


def test_one_batch_then_two():
    ctx, batch = _case(*NARROW[:3])
    stages, kernels = NARROW[3], NARROW[4]
    ctx.stage_reset()
    ctx.run_batch(batch.bases, batch.offsets, True)
    st, kn = ctx.stage_ms(), ctx.kernel_ms()
    print("stages", st, "kernels", kn, "excess", _excess(ctx))
    assert _launches(st) == stages and _launches(kn) == kernels
    for name, (ms, n) in list(st.items()) + list(kn.items()):
        assert (ms > 0) if n else (ms == 0), name
    assert all(e <= SLACK_MS for e in _excess(ctx).values())
    ctx.run_batch(batch.bases, batch.offsets, True)                       # the same batch again: every count doubles
    st, kn = ctx.stage_ms(), ctx.kernel_ms()
    print("stages", st, "kernels", kn, "excess", _excess(ctx))
    assert _launches(st) == {k: 2 * n for k, n in stages.items()}
    assert _launches(kn) == {k: 2 * n for k, n in kernels.items()}
    assert all(e <= SLACK_MS for e in _excess(ctx).values())


def test_wide_records_close_their_spans():
    ctx, batch = _case(*WIDE[:3])
    ctx.stage_reset()
    ctx.run_batch(batch.bases, batch.offsets, True)
    st, kn = ctx.stage_ms(), ctx.kernel_ms()
    print("stages", st, "kernels", kn)
    assert _launches(st) == WIDE[3] and _launches(kn) == WIDE[4]
    for name, (ms, n) in list(st.items()) + list(kn.items()):
        assert (ms > 0) if n else (ms == 0), name
