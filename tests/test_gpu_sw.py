"""sw_kernel on the device: the checks of tests/_sw.py — the golden bits of the compiled reference's SWFast_Seqs_BLOSUM62 through
mpcgpu_sw_scores, the case table (the emulator's, plus one 5 000 x 5 000 pair and one 30 x 20 000 pair) against the restatement bit
for bit, refusals by name."""
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
