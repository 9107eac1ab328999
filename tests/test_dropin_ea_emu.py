"""The drop-in's CalcEADistMx WITHOUT a GPU: the reference's `muscle` linked with the drop-in and the emulator build of the library
(the machinery of tests/test_dropin_emu.py) — -super5's committed MD5 through the new route, one library call in the timing report,
and the old route under MUSCLE_GPU_EA_DISTMX=0. Needs the reference objects
(oracle/_ref/obj): skipped where the reference sources were never available."""
import os
import subprocess

import pytest

import _ea_dropin as D
import _msa

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


def test_emu_super5_takes_the_route(emu_muscle):
    D.check_super5(emu_muscle)
