"""CPU checks of the stage-A case table (tests/_stage_a.py), no device and no emulator: the per-pair composition the table compares
with equals the oracle's own CalcPosteriors, the predictor puts every run of both tables on the path it claims (and on the same
batches whatever memory is free), every overflow run exceeds its room by the stated number of doublings, far from the edge, and the
GPU table stays within its oracle budget."""
import numpy as np
import pytest

import _parity as P
import _stage_a as S
from muscle_amd.synth import make_family


def test_pair_composition_equals_the_oracles_calc_posteriors():
    seqs = make_family(4, 60, seed=3) + ["MKV", "A" * 30]
    for mega in (None, S.with_mega(seqs, 4)):
        stages, ea = P.run_oracle(seqs, iters=2, mega=mega)
        want = S.oracle_pairs(seqs, mega)
        assert np.array_equal(S.bits(ea), S.bits(np.array([w["ea"] for w in want], np.float32)))
        got = S.oracle_relax(seqs, want)
        for a, b in zip(got, stages):
            for (o1, v1), (o2, v2) in zip(a, b):
                assert np.array_equal(o1, o2) and np.array_equal(v1, v2)


@pytest.mark.parametrize("name", S.CASE_NAMES)
@pytest.mark.parametrize("size", ["gpu", "emu"])
def test_predictor_puts_every_run_on_its_path(size, name):
    for run in S.case(size, name).runs:
        S.check_plan(run, size)


@pytest.mark.parametrize("size", ["gpu", "emu"])
def test_overflow_runs_exceed_the_room(size):
    """the first room is max(MPCGPU_CAND_PER_ROW * longest sequence, 1024) and doubles up to LXmax * LYmax: every overflow run needs
    exactly the doublings it states (check_plan holds each 10 % away from the rooms on either side)"""
    seen = 0
    for cs in S.cases(size):
        for run in cs.runs:
            if run.want.get("retries"):
                pr = S.check_plan(run, size)
                assert pr["retries"] == run.want["retries"] and pr["capc"] > pr["capc0"], (size, cs.name, run.what)
                seen += 1
    assert seen >= 7
    # the oracle's count for poly-A 60 x 100: 1627 candidates against a room of 12 x 100
    run = S.case(size, "overflow_natural").runs[0]
    want, k0, k1, lens, pr = S.plan(run, size)
    assert want[0]["cand"] == 1627 and pr["capc0"] == 1200


def test_gpu_table_oracle_budget():
    seen = set()
    total = sum(cs.cells(seen) for cs in S.cases("gpu"))
    print("oracle DP cells over the GPU table: %d" % total)
    assert total <= S.MAX_GPU_CELLS, total


def test_the_clamp_needs_other_tables():
    """mpcgpu_stage_a.inc clamps a doubled room at LXmax * LYmax. That needs a pair with more candidates than
    max(1024, LXmax * LYmax / 2): more than half of its cells at P >= 0.01. Under the amino-acid tables what spreads widest, poly-A of
    unequal lengths, stays under a third (the oracle's counts: 598 of 2040 cells at 34 x 60); overflow_clamp therefore runs under
    S.block_hmm(), where poly-A 26 x 78 has 1352 of 2028."""
    assert S.oracle_pairs(["A" * 34, "A" * 60])[0]["cand"] == 598
    run = S.case("gpu", "overflow_clamp").runs[0]
    want, k0, k1, lens, pr = S.plan(run, "gpu")
    assert want[1]["cand"] == 1352 and pr["capc0"] == 1024 and pr["capc"] == 26 * 78 < 2048 and pr["retries"] == 1
