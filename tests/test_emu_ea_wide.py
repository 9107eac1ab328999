"""post_wide_ea_kernel WITHOUT a GPU: the emulator build of the same sources (MPC_POSTW_THREADS = 128 there) through the forced-threshold
cases of tests/_ea_wide.py, one run under other lane orders, and the drop-in's -super5 with every pair of consensus sequences forced
wide (needs the reference objects, oracle/_ref/obj: skipped where the reference sources were never available)."""
import os
import subprocess

import pytest

import _ea_dropin as D
import _ea_wide as W
import _msa

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("name", W.CASES_FORCED)
def test_emu_ea_wide_case(emu, name):
    W.check_case(name, emu)


def test_emu_ea_wide_inert_beside_a_store(emu):
    W.check_inert(emu)


def test_emu_ea_wide_refusals(emu):
    W.check_refusals(emu)


@pytest.mark.parametrize("order", ["reverse", "random"])
def test_emu_ea_wide_other_thread_orders(emu, order):
    """the fibers of a wave in reverse / shuffled order: a lane that read a key, a row start or the DP row before its neighbour wrote it would show"""
    old = os.environ.get("EMU_SCHED")
    os.environ["EMU_SCHED"] = order
    try:
        for name in ("tiny", "lds_forced_64", "regrowth"):
            W.check_case(name, emu)
    finally:
        if old is None:
            os.environ.pop("EMU_SCHED", None)
        else:
            os.environ["EMU_SCHED"] = old


@pytest.mark.ref
def test_emu_super5_all_wide(emu):
    """-super5's committed MD5 with MPCGPU_EA_WIDE_MIN=1: CalcEADistMx's one call finishes every pair in post_wide_ea_kernel"""
    if os.path.isdir(os.path.join(_msa.ROOT, "oracle", "_ref", "obj")):
        env = dict(os.environ, MPCGPU_LIBDIR=EMU_DIR, MPCGPU_LIBNAME="mpcgpu_emu", MPCGPU_BIN="muscle_gpu_emu")
        subprocess.check_call(["bash", os.path.join(_msa.ROOT, "hostcxx", "build_muscle_gpu.sh")], env=env, stdout=subprocess.DEVNULL)
    if not os.path.exists(_msa.EMU_MUSCLE):
        pytest.skip("reference objects not available")
    name = "super5_14x20"
    md5, err = D.super5(_msa.EMU_MUSCLE, name, env={"MPCGPU_EA_WIDE_MIN": "1", "MPCGPU_TRACE": "1"})
    assert md5 == _msa.golden_md5()[name] and D.ea_calls(err) == 1, (md5, err[-2000:])
    assert "[mpcgpu] post wide ea:" in err and "[mpcgpu] post ea:" not in err, err[-2000:]
