"""search_pick_kernel and the indirect dense / alignment kernels WITHOUT a GPU: the emulator build of the same sources through the case
table of tests/_search.py (thin shapes) — mpcgpu_search_pairs at 0 ulp against the CPU oracle and against mpcgpu_align_pairs on a fresh
context, routes and the saving from mpcgpu_search_info, refusals, one context across calls, other lane orders."""
import os
import subprocess

import pytest

import _search

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("name", _search.CASES)
def test_emu_search_case(emu, name):
    _search.check_case(name, "emu", emu)


def test_emu_search_refusals(emu):
    _search.check_refusals(emu)


def test_emu_search_one_context_across_calls(emu):
    _search.check_sequence("emu", emu)


@pytest.mark.parametrize("order", ["reverse", "random"])
def test_emu_search_other_thread_orders(emu, order):
    """the fibers of a wave in reverse / shuffled order: the fold of search_pick_kernel must not depend on which lane runs first"""
    old = os.environ.get("EMU_SCHED")
    os.environ["EMU_SCHED"] = order
    try:
        _search.check_case("threshold", "emu", emu)
        _search.check_case("mega", "emu", emu)
    finally:
        if old is None:
            os.environ.pop("EMU_SCHED", None)
        else:
            os.environ["EMU_SCHED"] = old
