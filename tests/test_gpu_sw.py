"""sw_kernel on the device: the checks of tests/_sw.py — the golden bits of the compiled reference's SWFast_Seqs_BLOSUM62 through
mpcgpu_sw_scores, the case table (the emulator's, plus one 5 000 x 5 000 pair and one 30 x 20 000 pair) against the restatement bit
for bit with the route of every case (mpcgpu_sw_bins against the restated plan), lists long enough that waves take a second item, other
tables, reuse of a context, a call beside the posterior stage, refusals by name."""
import pytest

import _sw

pytestmark = pytest.mark.gpu


def test_sw_golden_bits():
    _sw.check_golden()


@pytest.mark.parametrize("name", _sw.CASES + _sw.GPU_ONLY)
def test_sw_case(name):
    _sw.check_case(name)


def test_sw_refusals():
    _sw.check_refusals()


def test_sw_queue_reuse():
    _sw.check_queue_reuse("gpu")


def test_sw_tables():
    _sw.check_tables()


def test_sw_context_reuse():
    _sw.check_context_reuse()


def test_sw_beside_the_stage():
    _sw.check_beside_the_stage()
