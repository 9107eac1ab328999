"""post_wide_kernel on the device (workgroups of 1024 threads): the checks of tests/_post_wide.py — candidate lists through
mpcgpu_post_scores(kernel = 2) against the oracle and post_kernel with the keys in LDS and through the global slots, a whole stage
under MPCGPU_POST_WIDE=1 with the shard's bytes against post_kernel's, mpcgpu_align_pairs on the forced route (candidate regrowth
included). Small shapes only: no real long pair runs here."""
import pytest

import _post_wide as W

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("key", W.SPECIAL + list(W.SHAPES), ids=str)
def test_post_wide_lists(key):
    W.check_lists(key)


def test_post_scores_kernel_argument():
    W.check_kernel_argument()


@pytest.mark.parametrize("which", W.STAGE_SETS)
def test_post_wide_stage(which):
    W.check_stage(which)


@pytest.mark.parametrize("wide", ["1", "0"])
@pytest.mark.parametrize("name", W.L.SMALL_NAMES)
def test_align_pairs_forced_route_post_wide(name, wide):
    """"regrowth" with wide = 1: MPCGPU_CAND_PER_ROW=1 overflows the lists of post_wide_kernel, the flag reaches the host and the
    regrown run matches the oracle"""
    W.check_align_pairs(name, None, 16, wide)


def test_align_pairs_post_info():
    W.check_align_pairs_info()
