"""fb_chain_mega_kernel on the SIMT emulator (no GPU): the chain sweeps of structure-profile input (kernels_fbc.h, MEGA = true;
MPCGPU_FB_CHAIN_MEGA) against the bb11001 golden and the oracle, with MPCGPU_FB_CHAIN_MEGA=1 and with MPCGPU_FB_CHAIN=0: EA bits,
nnz and every sparse matrix equal; chains reported under =1 and none under =0 or with the knob unset."""
import os
import subprocess

import numpy as np
import pytest

import _align_pairs as A
import _golden as G
import _mega_chains as MC
import _parity as P
from muscle_amd.synth import make_family

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


def _both(emu, seqs, mega):
    on = A.with_env(dict(MC.ON, **MC.GRADE0), lambda: MC.run(seqs, mega, emu))
    off = A.with_env(MC.OFF, lambda: MC.run(seqs, mega, emu))
    return on, off


def test_emu_mega_chains_bb11001(emu):
    m = G.mega("mega_bb11001")
    on, off = _both(emu, m["seqs"], m)
    for tag, got in (("MPCGPU_FB_CHAIN_MEGA=1", on), ("MPCGPU_FB_CHAIN=0", off)):
        MC.same(tag, got, m["ea"], m["stage"][0])
        assert G.stage_digest(got["store"]) == m["digest"][0], tag
    # 83, 85, 91, 86 residues: two rows per lane; (0,1) (0,2) (0,3) and (1,2) (1,3) chain, (2,3) is a chain of one
    assert on["info"] == (6, 5, 2) and on["bins"] == [2], (on["info"], on["bins"])
    assert off["info"] == (6, 0, 0) and off["bins"] == [], (off["info"], off["bins"])


def test_emu_mega_chains_unset_is_off(emu):
    m = G.mega("mega_bb11001")
    got = A.with_env(MC.GRADE0, lambda: MC.run(m["seqs"], m, emu))
    MC.same("unset", got, m["ea"], m["stage"][0])
    assert got["info"] == (6, 0, 0) and got["bins"] == [], (got["info"], got["bins"])


def test_emu_mega_chains_vs_oracle(emu):
    """seeded synthetic profiles as test_emu_mega_vs_oracle makes them (ragged alphabets, 8 features); lengths in the bins of one,
    two and three rows per lane, a column sequence of exactly T - 1 residues (chains) and one of T - 2 (leaves the chain)"""
    seqs = ["MKVLA", make_family(1, 70, seed=9)[0], "ACDEFGHIKLMNPQRSTVWY" * 4, make_family(1, 130, seed=3)[0][:126],
            make_family(1, 62, seed=4)[0], make_family(1, 61, seed=5)[0], make_family(1, 140, seed=6)[0], "WWWWWWWW"]
    mega = P.random_mega(seqs, seed=11)
    (want,), want_ea = P.run_oracle(seqs, iters=0, mega=mega)
    on, off = _both(emu, seqs, mega)
    MC.same("MPCGPU_FB_CHAIN_MEGA=1", on, want_ea, want)
    MC.same("MPCGPU_FB_CHAIN=0", off, want_ea, want)
    exp = MC.expected_chains([len(s) for s in seqs])
    assert exp[0] > 0 and on["info"] == (28,) + exp, (on["info"], exp)
    assert on["bins"] == [1, 2, 3], on["bins"]
    assert off["info"] == (28, 0, 0) and off["bins"] == []
