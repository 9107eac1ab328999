"""The device AlignPairFlat (mpcgpu_align_pairs + mpcgpu_get_list_sparse) on MI355X at production shapes, every path of its dispatcher
pinned bit for bit against the oracle: the short list in every rows-per-lane bin, each exit from it, the overflow redo, chains, row
blocks under H = 7 / 4 / 1, several chunks, chunk halving, Mega, one context reused, the refusal and degenerate pairs. Each call
proves its path by launch counters (in this process) and by MPCGPU_TRACE lines (in a child process); tests/_align_pairs.py holds
the table."""
import pytest

import _align_pairs as A

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", A.CASE_NAMES_GPU)
def test_align_pairs_case(name):
    A.run_case(A.case("gpu", name))
    A.check_case_traced("gpu", name)
