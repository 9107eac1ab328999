"""`muscle -swdistmx` and `muscle -super7 in.fa` with NO tree option through the drop-in linked with the emulator build of the library:
the guide tree comes from mpcgpu_sw_scores (hostcxx/mpcflat_gpu.cpp: CalcGuideTree_SW_BLOSUM62) and the bytes are the compiled
reference's (tests/golden/sw_dropin.json). Needs the reference objects (oracle/_ref/obj), like tests/test_dropin_emu.py."""
import os
import subprocess

import pytest

import _msa
import _sw
import _sw_dropin as D

ROOT = _msa.ROOT
pytestmark = pytest.mark.ref


@pytest.fixture(scope="module")
def emu_muscle():
    if os.path.isdir(os.path.join(ROOT, "oracle", "_ref", "obj")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu")], stdout=subprocess.DEVNULL)
        env = dict(os.environ, MPCGPU_LIBDIR=os.path.join(ROOT, "tests", "emu"), MPCGPU_LIBNAME="mpcgpu_emu", MPCGPU_BIN="muscle_gpu_emu")
        subprocess.check_call(["bash", os.path.join(ROOT, "hostcxx", "build_muscle_gpu.sh")], env=env, stdout=subprocess.DEVNULL)
    if not os.path.exists(_msa.EMU_MUSCLE):
        pytest.skip("reference objects not available")
    return _msa.EMU_MUSCLE


@pytest.mark.parametrize("name", list(_sw.DROPIN_SETS))
def test_emu_swdistmx_newick(emu_muscle, name):
    D.check_newick(emu_muscle, name)


@pytest.mark.parametrize("name", list(_sw.DROPIN_SETS))
def test_emu_super7_without_tree_option(emu_muscle, name):
    D.check_super7(emu_muscle, name)


def test_emu_sw_tree_off_is_the_reference_loop(emu_muscle):
    D.check_newick(emu_muscle, "swx_12x40", env={"MUSCLE_GPU_SW_TREE": "0"})
    D.check_super7(emu_muscle, "swx_12x40", env={"MUSCLE_GPU_SW_TREE": "0"})


def test_emu_super7_without_terminators_completes(emu_muscle):
    got, want = D.check_unterminated(emu_muscle, "swx_12x40")
    assert got == want
