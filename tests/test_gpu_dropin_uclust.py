"""`muscle_gpu -super5` and `-uclust` on the device with UClust::Run by windows (hostcxx/mpcflat_gpu.cpp): the reference's bytes
(tests/golden/uclust_dropin.json, written by the compiled reference) under MUSCLE_GPU_UCLUST_WINDOW = 0, 1, 4 and 64 with one and
four threads, and what the `uclust windows` row of the timing report must say of the route (tests/_uclust_dropin.py)."""
import os

import pytest

import _msa
import _uclust_dropin as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_muscle():
    if not os.path.exists(_msa.GPU_MUSCLE):
        pytest.fail("hostcxx/_build/muscle_gpu missing: run __graft_entry__.build() where the reference sources are, "
                    "or where oracle/_ref/muscle_gpu built there travelled along")
    return _msa.GPU_MUSCLE


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("cmd", ["super5", "uclust"])
@pytest.mark.parametrize("name", U.SETS)
def test_windows_write_the_reference_bytes(gpu_muscle, name, cmd, threads):
    U.check(gpu_muscle, name, cmd, threads)
