"""fb_coop_kernel on the SIMT emulator (tests/emu): the emulator runs every thread of a workgroup as a fiber and __syncthreads as a
cooperative barrier, so the W waves of a workgroup really interleave at the macro-step barriers and a wave that met a different
number of them would hang the launch. What the emulator cannot show is memory ordering between waves (its stores are visible at
once): that is the device test's part (tests/test_gpu_fb_coop.py). Thin shapes; the checks are tests/_fb_coop.py's."""
import os
import subprocess

import pytest

import _align_pairs as A
import _fb_coop as F
import _golden as G
import _parity as P

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("W", [2, 3, 4])
def test_emu_coop_rows(emu, W):
    """two blocks (idle waves under W = 3, 4), one block per wave, one wave wrapping to a one-row block, two rounds and a tail"""
    for k, LX in enumerate([65, 64 * W, 64 * W + 1, 64 * 2 * W + 37]):
        seqs, pairs = F.pair_of(LX, 9, 300 + k)
        F.check_list(seqs, pairs, W, lib_path=emu)


@pytest.mark.parametrize("LY", [1, 63, 64, 65, 127, 129])
def test_emu_coop_columns(emu, LY):
    """each side of a macro-step edge; with 1 column every block is shorter than the two-macro-step lag"""
    seqs, pairs = F.pair_of(64 * 3 + 5, LY, 320 + LY)
    F.check_list(seqs, pairs, 3, lib_path=emu)


def test_emu_coop_list(emu):
    """three row-block pairs of 2, 3 and 5 blocks, two short pairs, a pair given twice; MPCGPU_SCRATCH_GB=0 is not used: one stage A"""
    seqs = A.related([70, 150, 290, 40, 64, 12, 7], 341)
    pairs = [(0, 5), (3, 6), (2, 6), (1, 5), (4, 5), (0, 5)]
    F.check_list(seqs, pairs, 2, lib_path=emu)
    short = [(3, 6), (4, 5)]
    assert F.check_list(seqs, short, 2, lib_path=emu) == (0, 0)


def test_emu_coop_all_pairs_store_and_relax(emu):
    seqs = A.related([130, 70, 200, 9], 351)
    F.check_all_pairs(seqs, 3, {"MPCGPU_FB_LONG_MIN": "100", "MPCGPU_FB_LONG_H": "1"}, nlong=4, lib_path=emu)


def test_emu_coop_mega(emu):
    m = G.mega("mega_bb11001")
    mega = dict(m)
    stages, ea = F.all_pairs(m["seqs"], F.coop_env(F.FORCE_H1, 2), emu, mega, iters=0)[0]
    off = F.all_pairs(m["seqs"], F.coop_env(F.FORCE_H1, 0), emu, mega, iters=0)[0]
    assert (P.bits(ea) == P.bits(m["ea"])).all()
    assert G.stage_digest(stages[0]) == m["digest"][0]
    P.assert_same((stages, ea), off, "cooperative against single-wave, mega")


def test_emu_coop_no_memory_for_a_workgroup(emu):
    F.check_no_memory(emu)


def test_emu_coop_rule_and_unset(emu):
    """MPCGPU_FB_COOP=1, the rule: one pair of 4 blocks on the emulator's 8 wave slots -> W = min(4 waves of a workgroup, 4 blocks, 8 / 1);
    ten such pairs leave no slot for a second wave; unset: the single-wave kernel"""
    seqs, pairs = F.pair_of(64 * 3 + 9, 20, 360)
    assert F.check_list(seqs, pairs, 1, lib_path=emu, want_w=4) == (1, 4)
    assert F.check_list(seqs, pairs * 10, 1, lib_path=emu, want_pairs=0) == (0, 0)
    from muscle_amd._lib import MpcGpu
    h, (s, t, m, i, thr) = A.hmm()
    g = MpcGpu(0, emu)
    try:
        g.set_hmm(s, t, m, i, thr)
        g.set_seqs_registry(seqs)
        assert os.environ.get("MPCGPU_FB_COOP") is None
        assert F.run_list(g, seqs, pairs, F.FORCE_H1)[3] == (0, 0)
    finally:
        g.close()
