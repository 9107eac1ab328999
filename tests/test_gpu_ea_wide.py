"""post_wide_ea_kernel on the device: the case table of tests/_ea_wide.py — mpcgpu_ea_scores under MPCGPU_EA_WIDE=1 at 0 ulp against the
CPU oracle's EA and, where affordable, against mpcgpu_calc_posteriors + mpcgpu_get_ea on a second context; the route of every case by
mpcgpu_ea_info, mpcgpu_ea_wide_info and the launch counters; a call beside a store; the refusal that stays."""
import pytest

import _ea_wide as W

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", W.CASES)
def test_ea_wide_case(name):
    W.check_case(name)


def test_ea_wide_inert_beside_a_store():
    W.check_inert()


def test_ea_wide_refusals():
    W.check_refusals()
