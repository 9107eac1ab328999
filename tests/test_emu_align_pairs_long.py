"""mpcgpu_align_pairs beyond the row-list limit, on the SIMT emulator: small related sequences forced onto the route that long pairs
take (tests/_align_pairs_long.py: MPCGPU_POST_SORT_CAP=20000 keeps every list off the row-list finishing kernel, MPCGPU_PAIRS_SMALL=0)
— dense posteriors from the raw candidate lists (dense_post_raw_kernel) and the column-tiled alignment kernel
(calc_aln_tiled_kernel, MPCGPU_ALN_KERNEL=4, tiles of 37 columns) — bit for bit against ap_oracle, each call on its route by the
trace lines and launch counters. Letters, row blocks with 16-bit keys, Mega profiles, both expf variants, two chunks, chunk halving,
candidate regrowth; the three alignment kernels on the same pairs; mpcgpu_calc_aln alone; other thread orders."""
import os
import subprocess

import numpy as np
import pytest

import _align_pairs_long as L
import _oracle as O
import _parity as P
from muscle_amd._lib import MpcGpu

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")
EMU_ALN_WAVES = 2  # tests/emu/hip_emu.h: MPC_ALN_THREADS = 128


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("name", L.SMALL_NAMES)
def test_emu_align_pairs_forced_route(emu, name):
    L.check(name, emu, EMU_ALN_WAVES)


@pytest.mark.parametrize("order", ["reverse", "random"])
def test_emu_align_pairs_forced_route_other_thread_orders(emu, order):
    """the GPU threads of a block in reverse / shuffled order: a missing barrier around the tile edges or the DP rows shows"""
    L.check("sched", emu, EMU_ALN_WAVES, extra_env={"EMU_SCHED": order})


def calc_aln_matrices():
    """random thresholded matrices for mpcgpu_calc_aln alone: 1 x N, N x 1, widths off the tile and the thread count, all zero,
    ties on every cell"""
    rng = np.random.default_rng(11)
    mats = []
    for LX, LY in ((1, 1), (1, 300), (300, 1), (7, 36), (7, 37), (7, 38), (9, 127), (12, 129), (5, 333), (40, 75)):
        P0 = (rng.random((LX, LY)) < 0.15) * rng.random((LX, LY))
        mats.append(P0.astype(np.float32))
        mats.append((np.round(P0 * 4) / 4).astype(np.float32))  # many exact ties
    mats.append(np.zeros((6, 90), np.float32))
    mats.append(np.full((8, 101), 0.25, np.float32))
    mats.append(np.full((101, 8), 0.5, np.float32))
    return mats


def run_calc_aln(lib, env):
    def go():
        g = MpcGpu(0, lib)
        try:
            return [g.calc_aln(M) for M in calc_aln_matrices()]
        finally:
            g.close()
    return P_with_env(env, go)


def P_with_env(env, fn):
    import _align_pairs as A
    return A.with_env(env, fn)


@pytest.mark.parametrize("tile", ["37", "128", ""])
def test_emu_calc_aln_tiled_against_lds_rows(emu, tile):
    """MPCGPU_ALN_KERNEL=4 (tiles of 37 / 128 columns, one tile) against MPCGPU_ALN_KERNEL=3 and the oracle"""
    env4 = {"MPCGPU_ALN_KERNEL": "4"}
    if tile:
        env4["MPCGPU_ALN_TILE"] = tile
    got4, got3 = run_calc_aln(emu, env4), run_calc_aln(emu, {"MPCGPU_ALN_KERNEL": "3"})
    for M, (p4, s4), (p3, s3) in zip(calc_aln_matrices(), got4, got3):
        s0, p0 = O.calc_aln(M)
        assert p4 == p3 == p0, M.shape
        assert P.bits(s4) == P.bits(s3) == P.bits(s0), M.shape


@pytest.mark.parametrize("order", ["reverse", "random"])
def test_emu_calc_aln_tiled_other_thread_orders(emu, order):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, EMU_SCHED=order, PYTHONPATH=os.path.dirname(here) + os.pathsep + here)
    code = ("import test_emu_align_pairs_long as T, _oracle as O, _parity as P\n"
            "got = T.run_calc_aln(T.EMU_LIB, {'MPCGPU_ALN_KERNEL': '4', 'MPCGPU_ALN_TILE': '37'})\n"
            "for M, (p, s) in zip(T.calc_aln_matrices(), got):\n"
            "    s0, p0 = O.calc_aln(M)\n"
            "    assert p == p0 and P.bits(s) == P.bits(s0), M.shape\n"
            "print('OK tiled', flush=True)\n")
    r = subprocess.run([sys.executable, "-u", "-c", code], env=env, cwd=here, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, text=True)
    assert r.returncode == 0 and "OK tiled" in r.stdout, r.stdout[-3000:]


def test_emu_outside_the_envelope_is_refused_by_name(emu):
    """LX * LY * 5 + 100 > INT_MAX: refused before any device work with both lengths and the bound; the context stays usable"""
    import _align_pairs as A
    from muscle_amd._lib import MpcGpuError
    h, (s, t, m, i, thr) = A.hmm()
    seqs = A.related([30, 25], 207) + ["A" * 20800, "C" * 20800]
    g = MpcGpu(0, emu)
    try:
        g.set_hmm(s, t, m, i, thr)
        g.set_seqs_registry(seqs)
        with pytest.raises(MpcGpuError) as e:
            g.align_pairs([0, 2], [1, 3])
        msg = str(e.value)
        assert "mpcgpu_align_pairs" in msg and msg.count("20800") >= 2 and str(L.INT_MAX) in msg, msg
        (p, sc, ea), = g.align_pairs([0], [1])
        w = A.ap_oracle(h, seqs[0].encode(), seqs[1].encode())
        assert p == w["path"] and A.bits(sc) == A.bits(w["score"]) and A.bits(ea) == A.bits(w["ea"])
    finally:
        g.close()
