"""mpcgpu_upgma WITHOUT a GPU: the emulator build of the same sources (kernels_upgma.h under MPC_EMU) against the numpy restatement of
UPGMA5 (tests/_upgma.py) — 65 leaves, ScaleDistMx, average linkage, a matrix of 4 distinct values (ties, the redirect, stale minima), with
the row state in LDS and in global memory."""
import os
import subprocess

import pytest

import _sw
import _upgma as U

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


def test_emu_upgma_65_avg_scale(emu):
    U.check_case(emu, 65, "quant", "scale", "avg", lds=True)


def test_emu_upgma_65_avg_scale_row_state_in_global_memory(emu):
    _sw._with_env({"MPCGPU_UPGMA_LDS_ROWS": "0"}, lambda: U.check_case(emu, 65, "quant", "scale", "avg", lds=False))
