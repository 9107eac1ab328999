"""CPU checks of the relax case table (tests/_relax.py), no device and no emulator: every run's inputs have the properties its path
needs, from the oracle's matrices (row spans against the window descriptor's 5-bit field, sequence counts against 64 and against
MPCGPU_RELAX_SMALL_PAIRS, the largest pair against the staging budget it must not fit, the tile count of the tail case against
split_tail's threshold on 256 CUs and on the emulator's 2, the tail pair's empty half), and the GPU table stays within its oracle
budget."""
import time

import pytest

import _relax as R


@pytest.mark.parametrize("name", R.CASE_NAMES)
@pytest.mark.parametrize("size", ["gpu", "emu"])
def test_inputs_are_what_the_case_claims(size, name):
    for run in R.case(size, name).runs:
        R.check_claims(run, size)


def test_tail_threshold_is_the_librarys():
    """split_tail: per_xcd = max(cus * 2 / 8, 1) resident workgroups, tiles >= per_xcd * 8 * 3"""
    assert R.tail_threshold(256) == (1536, 64) and R.tail_threshold(2) == (24, 1)
    n = len(R.tail_set("gpu"))
    assert n * (n - 1) // 2 == 1596


def test_every_case_names_a_witness():
    for size in ("gpu", "emu"):
        for cs in R.cases(size):
            for run in cs.runs:
                assert run.store or run.trace or run.claims.get("halves") or any(w.get("has") for w in run.it), (cs.name, run.what)
                assert len(run.script) >= 2, (cs.name, run.what, "two iterations: the second runs on what the first left")


def test_gpu_table_oracle_budget():
    """the oracle's DP cells over the distinct inputs of the GPU table (measured: 2.36 M cells; the oracle's stage A and two relax
    rounds over all of them, with every other check of this file, take 2.6 s)"""
    seen = set()
    total = sum(cs.cells(seen) for cs in R.cases("gpu"))
    t0 = time.time()
    for seqs in seen:
        R.oracle(seqs)
    print("oracle DP cells over the GPU table: %d, %.1f s" % (total, time.time() - t0))
    assert total <= R.MAX_GPU_CELLS, total
