"""post_ea_kernel on the device: the case table of tests/_ea.py — mpcgpu_ea_scores at 0 ulp against the CPU oracle's EA and against
mpcgpu_calc_posteriors + mpcgpu_get_ea on a second context, the route of every case by mpcgpu_ea_info and the launch counters, a call
beside a store, refusals by name."""
import pytest

import _ea

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", _ea.CASES)
def test_ea_case(name):
    _ea.check_case(name)


def test_ea_inert_beside_a_store():
    _ea.check_inert()


def test_ea_refusals():
    _ea.check_refusals()
