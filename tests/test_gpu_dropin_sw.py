"""`muscle_gpu -swdistmx` and `muscle_gpu -super7 in.fa` with NO tree option on the device: the guide tree comes from mpcgpu_sw_scores
(hostcxx/mpcflat_gpu.cpp: CalcGuideTree_SW_BLOSUM62), the Newick bytes and the MSAs are the compiled reference's
(tests/golden/sw_dropin.json)."""
import os

import pytest

import _msa
import _sw
import _sw_dropin as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_muscle():
    if not os.path.exists(_msa.GPU_MUSCLE):
        pytest.fail("hostcxx/_build/muscle_gpu missing: run __graft_entry__.build() where the reference sources are, "
                    "or where oracle/_ref/muscle_gpu built there travelled along")
    return _msa.GPU_MUSCLE


@pytest.mark.parametrize("name", list(_sw.DROPIN_SETS))
def test_swdistmx_newick(gpu_muscle, name):
    D.check_newick(gpu_muscle, name)


@pytest.mark.parametrize("name", list(_sw.DROPIN_SETS))
def test_super7_without_tree_option(gpu_muscle, name):
    D.check_super7(gpu_muscle, name)


def test_sw_tree_off_is_the_reference_loop(gpu_muscle):
    D.check_newick(gpu_muscle, "swx_12x40", env={"MUSCLE_GPU_SW_TREE": "0"})
    D.check_super7(gpu_muscle, "swx_12x40", env={"MUSCLE_GPU_SW_TREE": "0"})


def test_super7_without_terminators_completes(gpu_muscle):
    got, want = D.check_unterminated(gpu_muscle, "swx_12x40")
    assert got == want
