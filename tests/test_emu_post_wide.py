"""post_wide_kernel WITHOUT a GPU: the emulator build of the same sources (workgroups of 128 threads, two waves) through the checks of
tests/_post_wide.py — candidate lists against the oracle and against post_kernel with both buffer placements, a whole stage under
MPCGPU_POST_WIDE=1 with the shard's bytes against post_kernel's, mpcgpu_align_pairs on the forced route (candidate regrowth
included), and other thread orders of the workgroup."""
import os
import subprocess

import pytest

import _post_wide as W

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")
EMU_ALN_WAVES = 2  # tests/emu/hip_emu.h: MPC_ALN_THREADS = 128


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("key", W.SPECIAL + list(W.SHAPES), ids=str)
def test_emu_post_wide_lists(emu, key):
    W.check_lists(key, emu)


def test_emu_post_scores_kernel_argument(emu):
    W.check_kernel_argument(emu)


@pytest.mark.parametrize("which", W.STAGE_SETS)
def test_emu_post_wide_stage(emu, which):
    W.check_stage(which, emu)


@pytest.mark.parametrize("wide", ["1", "0"])
@pytest.mark.parametrize("name", W.L.SMALL_NAMES)
def test_emu_align_pairs_forced_route_post_wide(emu, name, wide):
    """"regrowth" with wide = 1: MPCGPU_CAND_PER_ROW=1 overflows the lists of post_wide_kernel, the flag reaches the host and the
    regrown run matches the oracle"""
    W.check_align_pairs(name, emu, EMU_ALN_WAVES, wide)


def test_emu_align_pairs_post_info(emu):
    W.check_align_pairs_info(emu)


@pytest.mark.parametrize("order", ["reverse", "random"])
def test_emu_post_wide_other_thread_orders(emu, order):
    """the fibers of a workgroup in reverse / shuffled order: a missing barrier in the scatter, the scans or the DP rows shows"""
    old = os.environ.get("EMU_SCHED")
    os.environ["EMU_SCHED"] = order
    try:
        for key in ("fixed", (5, 200), (90, 70), (12, 40)):
            W.check_lists(key, emu)
    finally:
        if old is None:
            os.environ.pop("EMU_SCHED", None)
        else:
            os.environ["EMU_SCHED"] = old
