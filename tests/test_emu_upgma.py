"""mpcgpu_upgma WITHOUT a GPU: the emulator build of the same sources (kernels_upgma.h under MPC_EMU: a join workgroup of 128 fibers, 2
CUs) against the numpy restatement of UPGMA5 (tests/_upgma.py), node indices and float bits, on the named cases tests/test_upgma_table.py
shows to reach every path: 65 and 129 leaves; 300 leaves (rows in a second and a third stride of the workgroup, ties across waves and
strides, redirects, stale picks) under every linkage with the row state in LDS and in global memory, twice more in a random thread order;
Min and Max in a later pass of the grid-stride loops; the value edges (subnormals, zeros of both signs, NaN, inf, EA values at and beyond
the ends of 0 .. 1) with the kind of refusal and its join; outputs untouched by a refusal; one context reused across sizes and refusals."""
import os
import subprocess
import sys

import pytest

import _sw
import _upgma as U

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")
N = U.STRIDE_N["emu"]


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


def _global(fn):
    return _sw._with_env({"MPCGPU_UPGMA_LDS_ROWS": "0"}, fn)


def test_emu_upgma_65_avg_scale(emu):
    U.check_case(emu, 65, "quant", "scale", "avg", lds=True)


def test_emu_upgma_65_avg_scale_row_state_in_global_memory(emu):
    _global(lambda: U.check_case(emu, 65, "quant", "scale", "avg", lds=False))


@pytest.mark.parametrize("kind", ("quant", "random", "negative", "fltmax"))
def test_emu_upgma_129(emu, kind):
    """one row beyond the workgroup; the four matrices of the device test (negative entries: the clamp of the transform kernel)"""
    for transform in U.TRANSFORMS:
        for linkage in U.LINKAGES:
            U.check_case(emu, 129, kind, transform, linkage, lds=True)


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("linkage", U.LINKAGES)
@pytest.mark.parametrize("kind", U.STRIDE_KINDS)
def test_emu_upgma_strides(emu, kind, linkage, lds):
    def go():
        for transform in ("none", "scale"):
            U.check_case(emu, N, kind, transform, linkage, lds=lds)
    go() if lds else _global(go)


def test_emu_upgma_extremes(emu):
    U.check_extremes(emu, N, U.CUS["emu"])


def test_emu_upgma_value_edges(emu):
    for n, kind, transform, linkage in U.edge_cases("emu"):
        U.check_case(emu, n, kind, transform, linkage, lds=True)
    _global(lambda: [U.check_case(emu, n, kind, transform, linkage, lds=False) for n, kind, transform, linkage in U.edge_cases("emu")
                     if kind in ("subnormal", "nan_mid", "nan_all")])


def test_emu_upgma_refusal_leaves_the_outputs(emu):
    n = U.EA_BAD_N["emu"]
    U.check_refusal_leaves_outputs(emu, n, ("ea_one_bad", "nan"), "ea", "avg", "ea_range")
    U.check_refusal_leaves_outputs(emu, U.SMALL_N["emu"], "nan_all", "ea", "avg", "ea_range")
    U.check_refusal_leaves_outputs(emu, U.SMALL_N["emu"], "nan_first", "scale", "avg", "no_min")


def test_emu_upgma_reuse(emu):
    U.check_reuse(emu, N, 65)


def test_emu_sw_tree_refuses_a_long_sequence(emu):
    U.check_long_sequence_refused(emu)


def test_emu_upgma_strides_in_random_thread_order(emu):
    """the fibers of the join workgroup in a shuffled order between barriers (EMU_SCHED is read once per process: a child): a wave that
    wrote its slot of one slot set while another still read it — the two sets of mpc_block_argmin alternate so that no barrier is needed
    between the folds — or a lane that read m_NodeIndex / m_NearestNeighbor before lane 0 wrote the join's result would show"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, EMU_SCHED="random", PYTHONPATH=os.path.dirname(here) + os.pathsep + here)
    code = ("import _sw, _upgma as U\n"
            "for lds in (True, False):\n"
            "    for linkage in ('avg', 'max'):\n"
            "        for transform in ('none', 'scale'):\n"
            "            _sw._with_env({} if lds else {'MPCGPU_UPGMA_LDS_ROWS': '0'}, lambda: U.check_case(%r, %d, 'quant', transform, linkage, lds=lds))\n"
            "print('OK random order', flush=True)\n" % (emu, N))
    r = subprocess.run([sys.executable, "-u", "-c", code], env=env, cwd=here, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
    assert r.returncode == 0 and "OK random order" in r.stdout, r.stdout[-3000:]
