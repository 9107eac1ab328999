"""mpcgpu_align_pairs beyond the row-list limit on MI355X at real sizes, ONE context, bit for bit against ap_oracle (path, score and
EA bits, get_list_sparse), each call on its route by trace lines and launch counters (tests/_align_pairs_long.py):

  12200 x 12200      the smallest square off the row-list kernel (LX + 2 LY = 36 600 > 36 344): raw dense build, "rows in LDS"
  300 x 20000        the list does not fit: raw dense build, "rows in LDS"
  20000 x 300,       fit the row-list kernel: dense_post_kernel as before; "waves, rows in registers" / "rows in LDS" /
  2 x 15000,           "waves, rows in registers"
  15000 x 2
  300 x 60000        wider than the LDS rows: raw dense build, "rows in LDS, column tiles" (4 tiles of 16 384 columns)
  6000 x 60000       the same with row blocks and 16-bit keys (test_align_pairs_long_6000x60000: a context of its own, see
                     tests/_align_pairs_long.py gpu_wide_scenario)
  mixed list         one 300 x 20000 pair among L~400 pairs: the whole list leaves the row-list kernel
  20800 x 20800      outside LX * LY * 5 + 100 <= INT_MAX: refused by name with both lengths, no device work; the next call matches

ap_oracle of the 12 200 x 12 200 pair on the CPU (one thread): ORACLE_12200 below. The whole scenario asks the oracle for
~0.55 G cells (6000 x 60000 alone: 360 M cells, ~17 GB for the forward and backward planes).

The forced small-size cases of tests/test_emu_align_pairs_long.py run once more on the device."""
import pytest

import _align_pairs_long as L

pytestmark = pytest.mark.gpu

ORACLE_12200 = "32 s, 6.1 GB peak resident (7 709 candidate cells, path of 12 403 letters); 6000 x 60000: 78 s, 14.8 GB, 48 014 545 candidate cells"


@pytest.fixture(scope="module")
def long_run():
    return L.run_child("long", None, timeout=1700)


@pytest.mark.parametrize("k", range(len(L.GPU_CALLS)), ids=[w.split(":")[0].replace(" ", "") for w in L.GPU_CALLS])
def test_align_pairs_long(long_run, k):
    sc, parts = long_run
    L.check_call(sc, k, parts[k], 16)


def test_align_pairs_long_6000x60000():
    L.check("long_wide", None, 16, timeout=3000)


@pytest.mark.parametrize("name", L.SMALL_NAMES)
def test_align_pairs_forced_route_on_the_device(name):
    L.check(name, None, 16)
