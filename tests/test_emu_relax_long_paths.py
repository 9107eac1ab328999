"""The small-shape cases of tests/test_gpu_relax_long_paths.py on the SIMT emulator (the same kernel sources, no GPU): grid-stride
trips of var_build_long_kernel, split ranges, batched and wide joins over the long form, form changes on one context, and a
distance with a non-zero upper half at the smallest size that has one. tests/_relax_long.py holds the inputs."""
import os
import subprocess
import sys

import pytest

import _relax as R
import _relax_long as L

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


def test_emu_long_grid_stride(emu):
    """n from the emulator's CU count (2: a grid of 8 workgroups, 16 records): every workgroup builds two records on its scratch"""
    n = L.check_stride(R.CUS["emu"], emu)
    assert n * n >= 2 * 4 * R.CUS["emu"]


def test_emu_long_grid_stride_in_random_thread_order(emu):
    """the grid-stride store with the fibers of a block in a shuffled order between synchronisation points (EMU_SCHED is read once
    per process: a child). What this order can show: a lane of var_build_long_kernel, commit_pairs_long_kernel or the several waves
    of relax_band_kernel<MpcRbLongCxx> that reads what another lane has yet to write. What it cannot show: the loss of
    var_build_long_kernel's trailing __syncthreads(). Its workgroup is ONE wave, and the shuffles of the next record's scans, which
    every lane passes before any lane writes s_start again, are a rendezvous of that wave, here as on the device: the barrier is
    kept because var_build_kernel has it, and no run in any order depends on it"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, EMU_SCHED="random", PYTHONPATH=os.path.dirname(here) + os.pathsep + here)
    code = ("import _relax as R, _relax_long as L\n"
            "L.check_stride(R.CUS['emu'], %r)\n"
            "print('OK stride', flush=True)\n" % emu)
    r = subprocess.run([sys.executable, "-u", "-c", code], env=env, cwd=here, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
    assert r.returncode == 0 and "OK stride" in r.stdout, r.stdout[-3000:]


def test_emu_long_ranges(emu):
    L.check_ranges(emu)


def test_emu_long_joins(emu):
    L.check_joins(emu)


def test_emu_long_form_changes(emu):
    L.check_forms("emu", emu)


def test_emu_long_dist_hi_small(emu):
    """the smallest store with a distance that needs its upper half: 4200 positions with a low-complexity stretch at row 40, so that
    the first blocks of those rows lie 4096 and more blocks before their overflow blocks (dist.hi = 1, asserted from the layout);
    no knob: the library's trigger. Store, two iterations and a join by rows against the oracle"""
    seqs = L.field_seqs("dist_hi_small")
    c = L.field_counts(seqs)
    assert c["hi1_lo"] > 0 and c["hi0_lo"] > 0 and c["rows_3_blocks"] > 0, c
    L.check_field("dist_hi_small", emu)
