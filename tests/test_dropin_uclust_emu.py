"""UClust::Run by windows WITHOUT a GPU: the reference's `muscle` linked with the drop-in and the emulator build of the library (the
machinery of tests/test_dropin_emu.py) — `-super5` and `-uclust` on the thin sets of tests/_uclust_dropin.py write the reference's bytes (tests/golden/uclust_dropin.json) under
MUSCLE_GPU_UCLUST_WINDOW = 0, 1, 4 and 64 with one and four threads, and the `uclust windows` row names the route. Needs the reference
objects (oracle/_ref/obj): skipped where the reference sources were never available."""
import os
import subprocess

import pytest

import _msa
import _uclust_dropin as U

ROOT = _msa.ROOT
pytestmark = pytest.mark.ref


@pytest.fixture(scope="module")
def emu_muscle():
    if os.path.isdir(os.path.join(ROOT, "oracle", "_ref", "obj")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu")], stdout=subprocess.DEVNULL)
        env = dict(os.environ, MPCGPU_LIBDIR=os.path.join(ROOT, "tests", "emu"), MPCGPU_LIBNAME="mpcgpu_emu",
                   MPCGPU_BIN="muscle_gpu_emu")
        subprocess.check_call(["bash", os.path.join(ROOT, "hostcxx", "build_muscle_gpu.sh")], env=env, stdout=subprocess.DEVNULL)
    if not os.path.exists(_msa.EMU_MUSCLE):
        pytest.skip("reference objects not available")
    return _msa.EMU_MUSCLE


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("cmd", ["super5", "uclust"])
@pytest.mark.parametrize("name", U.SETS_EMU)
def test_emu_windows_write_the_reference_bytes(emu_muscle, name, cmd, threads):
    U.check(emu_muscle, name, cmd, threads)
