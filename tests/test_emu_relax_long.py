"""The long form of the record store and of relax_band_kernel (MPCGPU_RELAX_LONG=1 forces it at any length) on the SIMT emulator:
the forced small shapes of tests/test_gpu_relax_long.py, the same source, no GPU. tests/_relax_long.py holds the inputs."""
import os
import subprocess

import pytest

import _relax_long as L

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("n", [3, 5, 9])
def test_emu_relax_long_forced(emu, n):
    """store, both iterations and EA equal the oracle's; relax_info names the long form, not a fallback (fails without the long
    form: the knob is unknown, the store is today's band layout)"""
    seqs = L.forced_seqs(n)
    L.check_forced_claims(seqs)
    infos = L.run(seqs, L.FORCE, has=L.LONG, lacks=("window records", "CSR slabs"), fallback=False, lib_path=emu, store=("band-long",))
    assert all("MpcRbLongCxx" in i for i in infos[1:]), infos


@pytest.mark.parametrize("n", [3, 5, 9])
def test_emu_relax_long_joins(emu, n):
    """the joins' reader of the block records (BuildPost by rows) follows the long form"""
    info, fb = L.check_join(L.forced_seqs(n), L.FORCE, emu)
    assert "band-long" in info and "MpcRbLongCxx" in info and not fb, info


def test_emu_relax_long_segments(emu):
    """the long form in a store cut into segments (MPCGPU_STORE_SEG_BLOCKS: the test hook of the > 64 GiB stores): the per-step base
    address in the staging, MpcRbSegmented<MpcRbLongCxx>"""
    seqs = L.forced_seqs(9)
    blocks = sum(len(s) for s in seqs)
    infos = L.run(seqs, dict(L.FORCE, MPCGPU_STORE_SEG_BLOCKS=str(4 * blocks)), has=("band-long", "MpcRbSegmented<MpcRbLongCxx>", "segments"),
                  fallback=False, lib_path=emu)
    assert infos


def test_emu_relax_long_off(emu):
    """MPCGPU_RELAX_LONG=0 on a store within today's limits: today's layout"""
    infos = L.run(L.forced_seqs(5), {"MPCGPU_RELAX_LONG": "0"}, has=("relax_band_kernel",), lacks=("band-long", "MpcRbLong"), fallback=False, lib_path=emu)
    assert infos
