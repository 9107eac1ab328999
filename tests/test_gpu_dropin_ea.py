"""`muscle_gpu -super5` on the device: the EA of all pairs of consensus sequences comes from ONE mpcgpu_ea_scores call
(hostcxx/mpcflat_gpu.cpp: CalcEADistMx), the timing report counts the call, the MSA is the committed MD5 of the reference, and
MUSCLE_GPU_EA_DISTMX=0 takes the old route to the same MSA. (`-eadistmx` itself: tests/_ea_dropin.py says why it has no test.)"""
import os

import pytest

import _ea_dropin as D
import _msa

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_muscle():
    if not os.path.exists(_msa.GPU_MUSCLE):
        pytest.fail("hostcxx/_build/muscle_gpu missing: run __graft_entry__.build() where the reference sources are, "
                    "or where oracle/_ref/muscle_gpu built there travelled along")
    return _msa.GPU_MUSCLE


def test_super5_takes_the_route(gpu_muscle):
    D.check_super5(gpu_muscle)
