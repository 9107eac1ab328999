"""Store build and consistency relax on MI355X, every path of build_var_store, mpcgpu_cons_iter's iteration-time fallbacks, the band
tile cutter (routes, halving, the tail) and the four merges in both staging modes pinned bit for bit against the oracle, with the
hand-scheduled merges the emulator cannot run. Each case runs in a child process of its own with MPCGPU_TRACE=1 under its own
timeout and proves its path by relax_info, store_info, launch counters and trace lines; after a child that died of a signal or
hung no further child is started. tests/_relax.py holds the table and the path map."""
import pytest

import _relax as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_relax_case(name):
    R.check_case("gpu", name)
