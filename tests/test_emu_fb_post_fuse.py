"""fb_chain_post_kernel WITHOUT a GPU: the emulator build of the same sources through the cases of tests/_fb_post_fuse.py (four waves
of a workgroup, each finishing its own chains between its sweeps)."""
import os
import subprocess

import pytest

import _fb_post_fuse as F

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("name", F.EMU_NAMES)
def test_emu_fused_finish_matches_separate_launch_and_oracle(emu, name):
    F.check(name, emu)


def test_emu_default_rule(emu):
    F.check_default(emu)
