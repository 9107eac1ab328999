"""The drop-in's ensemble reuse WITHOUT a GPU: the reference's `muscle` linked with the drop-in and the emulator build of
libmpcgpu (as tests/test_dropin_emu.py builds it) runs `-align -stratified` on three sequences — the smallest run that still
relaxes — and writes the compiled reference's bytes from 4 computed and 12 reused posterior stages. Needs the reference objects
(oracle/_ref/obj): skipped where the reference sources were never available."""
import os
import subprocess

import pytest

import _ensemble as E
import _msa

ROOT = _msa.ROOT
pytestmark = pytest.mark.ref


@pytest.fixture(scope="module")
def emu_muscle():
    if os.path.isdir(os.path.join(ROOT, "oracle", "_ref", "obj")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu")], stdout=subprocess.DEVNULL)
        env = dict(os.environ, MPCGPU_LIBDIR=os.path.join(ROOT, "tests", "emu"), MPCGPU_LIBNAME="mpcgpu_emu",
                   MPCGPU_BIN="muscle_gpu_emu")
        subprocess.check_call(["bash", os.path.join(ROOT, "hostcxx", "build_muscle_gpu.sh")], env=env, stdout=subprocess.DEVNULL)
    if not os.path.exists(_msa.EMU_MUSCLE):
        pytest.skip("reference objects not available")
    return _msa.EMU_MUSCLE


def test_emu_stratified_n3(emu_muscle):
    name = "strat_n3_L30"
    outs, err = E.run_case(emu_muscle, name, threads=2, timeout=900, env={"MUSCLE_GPU_TIMING": "1"})
    assert E.stage_counts(err) == E.CASES[name][3] == (4, 12)
    assert E.md5s(outs) == E.golden()[name]


@pytest.mark.parametrize("env,counts", [({"MUSCLE_GPU_DOWNLOAD": "1"}, (4, 12)), ({"MUSCLE_GPU_DEVICES": "0,0"}, (4, 12)),
                                        ({"MUSCLE_GPU_ENSEMBLE_REUSE": "0"}, (16, 0))])
def test_emu_stratified_n2_host_matrix_path(emu_muscle, env, counts):
    """two sequences: Consistency is skipped, so the kept stage is complete at the end of stage A (with MUSCLE_GPU_DOWNLOAD the
    host matrices are downloaded again for every replicate); a group of two contexts; the switch"""
    name = "strat_n2_L40"
    outs, err = E.run_case(emu_muscle, name, threads=2, timeout=900, env=dict(env, MUSCLE_GPU_TIMING="1"))
    assert E.stage_counts(err) == counts
    assert E.md5s(outs) == E.golden()[name]
