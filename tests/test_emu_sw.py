"""sw_kernel WITHOUT a GPU: the emulator build of the same sources through the checks of tests/_sw.py — the golden bits of the compiled
reference through mpcgpu_sw_scores, the case table against the restatement bit for bit with the route of every case (mpcgpu_sw_bins
against the restated plan), waves that take a second item, other tables, reuse of a context, a call beside the posterior stage,
refusals by name, other lane orders."""
import os
import subprocess

import pytest

import _sw

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


def test_emu_sw_golden_bits(emu):
    _sw.check_golden(emu)


@pytest.mark.parametrize("name", _sw.CASES)
def test_emu_sw_case(emu, name):
    _sw.check_case(name, emu)


def test_emu_sw_refusals(emu):
    _sw.check_refusals(emu)


def test_emu_sw_queue_reuse(emu):
    _sw.check_queue_reuse("emu", emu)


def test_emu_sw_tables(emu):
    _sw.check_tables(emu)


def test_emu_sw_context_reuse(emu):
    _sw.check_context_reuse(emu)


def test_emu_sw_beside_the_stage(emu):
    _sw.check_beside_the_stage(emu)


@pytest.mark.parametrize("order", ["reverse", "random"])
def test_emu_sw_other_thread_orders(emu, order):
    """the fibers of a wave in reverse / shuffled order: a lane that read a neighbour's value before it was handed on would show — the
    row-block cases too, whose lines are written by lane 63 and read by all lanes of the next block"""
    old = os.environ.get("EMU_SCHED")
    os.environ["EMU_SCHED"] = order
    try:
        for name in ("identical", "chain_cut", "explicit_list", "long_chains", "long_chain_separators", "long_chain_separators_513",
                     "long_chain_separators_1024", "long_chain_separators_1536"):
            _sw.check_case(name, emu)
    finally:
        if old is None:
            os.environ.pop("EMU_SCHED", None)
        else:
            os.environ["EMU_SCHED"] = old
