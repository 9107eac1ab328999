"""mpcgpu_search_pairs on the device: the case table of tests/_search.py at 0 ulp against the CPU oracle and against mpcgpu_align_pairs on
a fresh context, the route of every case and the saving (dense posteriors and trace-backs for the accepted groups alone) from
mpcgpu_search_info, refusals that leave context and outputs untouched, one context across accepted and refused calls."""
import pytest

import _search

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", _search.CASES)
def test_search_case(name):
    _search.check_case(name, "gpu")


def test_search_refusals():
    _search.check_refusals()


def test_search_one_context_across_calls():
    _search.check_sequence("gpu")
