"""The relax case table (tests/_relax.py) on the SIMT emulator: the same rows as tests/test_gpu_relax.py with the C++ statement of
the merges, the emulator's CU count for the tail of the tile list, and the iteration-time fallbacks of mpcgpu_cons_iter again with
threads run in reverse and in random order between synchronisation points."""
import os
import subprocess

import pytest

import _relax as R

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_emu_relax_case(emu, name):
    """every run of the case against the oracle (EA, the store, every iteration) and on its path by relax_info, store_info, launch
    counters and MPCGPU_TRACE lines: the table runs once, in child processes side by side (_relax.emu_table)"""
    R.check_case_emu(name, emu)


@pytest.mark.parametrize("sched", ["reverse", "random"])
@pytest.mark.parametrize("name", R.FALLBACK_CASES)
def test_emu_relax_fallbacks_thread_order(emu, name, sched):
    R.check_case_emu(name, emu, sched)
