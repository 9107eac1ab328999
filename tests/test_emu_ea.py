"""post_ea_kernel WITHOUT a GPU: the emulator build of the same sources (the kernel source as it is) through the case table of
tests/_ea.py — mpcgpu_ea_scores at 0 ulp against the CPU oracle's EA and against mpcgpu_calc_posteriors + mpcgpu_get_ea on a second
context, the route of every case, a call beside a store, refusals by name, other lane orders."""
import os
import subprocess

import pytest

import _ea

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("name", _ea.CASES_BASE + _ea.CASES_PATHS)  # (CASES_DEVICE: their lists at a tenth of the long column are in CASES_PATHS)
def test_emu_ea_case(emu, name):
    _ea.check_case(name, emu)


def test_emu_ea_inert_beside_a_store(emu):
    _ea.check_inert(emu)


def test_emu_ea_refusals(emu):
    _ea.check_refusals(emu)


@pytest.mark.parametrize("order", ["reverse", "random"])
def test_emu_ea_other_thread_orders(emu, order):
    """the fibers of a wave in reverse / shuffled order: a lane that read the list or the DP row before its neighbour wrote it would show"""
    old = os.environ.get("EMU_SCHED")
    os.environ["EMU_SCHED"] = order
    try:
        for name in ("tiny_1_1_2", "chaining", "regrowth", "persistent_small", "sort_cap_mixed", "post_batch_3", "batches_regrowth"):
            _ea.check_case(name, emu)
    finally:
        if old is None:
            os.environ.pop("EMU_SCHED", None)
        else:
            os.environ["EMU_SCHED"] = old
