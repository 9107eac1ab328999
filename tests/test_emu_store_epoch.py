"""mpcgpu_store_epoch WITHOUT a GPU: the checks of tests/test_gpu_store_epoch.py on the emulator build of the same library
sources (tests/emu), so that the bookkeeping is proven before GPU minutes are spent."""
import os
import subprocess

import pytest

import _store_epoch as SE

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


def test_emu_readers_leave_the_epoch(emu):
    SE.check_readers_leave_it(emu)


@pytest.mark.parametrize("name", sorted(SE.MOVERS))
def test_emu_epoch_moves(emu, name):
    SE.check_mover(name, emu)


def test_emu_list_stage_moves_the_epoch(emu):
    SE.check_list_stage_moves_it(emu)


def test_emu_new_context_is_zero_and_refused_calls_leave_it(emu):
    SE.check_new_context_and_refusals(emu)


def test_emu_epoch_guards_a_reused_store(emu):
    SE.check_epoch_guards_reuse(emu)


def test_emu_group_calls_move_every_context(emu):
    SE.check_group_moves_every_context(emu, devices=(0, 0))
