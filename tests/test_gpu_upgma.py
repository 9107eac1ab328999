"""mpcgpu_upgma, mpcgpu_sw_tree and mpcgpu_upgma_info on the device against the numpy restatement of UPGMA5 (tests/_upgma.py): node indices
equal, float bits of the branch lengths equal. Sizes: 2 (the first), 3, 65 (one past a wavefront) and 1025 (one past the workgroup of the
join kernel: a lane owns more than one row), each with every transform and linkage on a random matrix, a matrix of 4 distinct values (ties,
the neighbour redirect, stale minima), one with negative entries and one with FLT_MAX entries; 65 and 1025 again with the row state in
global memory. Where the reference itself asserts or dies (an EA value outside 0 .. 1; no distance below FLT_MAX left: a scaled matrix of
one value, FLT_MAX under "max") the library must refuse by name."""
import hashlib
import os

import numpy as np
import pytest

import _golden as G
import _msa
import _sw
import _sw_dropin as D
import _upgma as U
from muscle_amd._lib import MpcGpu, MpcGpuError
from muscle_amd.synth import make_family

pytestmark = pytest.mark.gpu

KINDS = ("random", "quant", "negative", "fltmax")


@pytest.mark.parametrize("transform", U.TRANSFORMS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [2, 3, 65, 1025])
def test_upgma_bits(n, kind, transform):
    for linkage in U.LINKAGES:
        U.check_case(None, n, kind, transform, linkage, lds=True)


@pytest.mark.parametrize("transform", U.TRANSFORMS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [65, 1025])
def test_upgma_bits_row_state_in_global_memory(n, kind, transform):
    def run():
        for linkage in U.LINKAGES:
            U.check_case(None, n, kind, transform, linkage, lds=False)
    _sw._with_env({"MPCGPU_UPGMA_LDS_ROWS": "0"}, run)


def test_upgma_lds_cut_is_inclusive():
    """MPCGPU_UPGMA_LDS_ROWS = n: LDS; n - 1: global memory"""
    _sw._with_env({"MPCGPU_UPGMA_LDS_ROWS": "65"}, lambda: U.check_case(None, 65, "quant", "scale", "avg", lds=True))
    _sw._with_env({"MPCGPU_UPGMA_LDS_ROWS": "64"}, lambda: U.check_case(None, 65, "quant", "scale", "avg", lds=False))


def test_upgma_refusals_leave_the_context():
    """every refusal made before any device work: the store epoch and mpcgpu_align_alns' answer on a store built before stay"""
    seqs = make_family(6, 50, seed=46)
    s, t, m, i, thr = G.hmm_tables()
    g = MpcGpu(0)
    try:
        g.set_hmm(s, t, m, i, thr)
        g.set_seqs(seqs)
        g.calc_posteriors()
        g.build_store()

        def join():
            maps = [np.arange(len(x), dtype=np.uint32) for x in seqs]
            C = max(len(x) for x in seqs)
            return g.align_alns([0, 1, 2], [3, 4, 5], maps[:3], maps[3:], C, C)
        epoch, before = g.store_epoch(), join()
        tri = U.make_tri(5, "random", 9)
        out = [np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.float32), np.zeros(4, np.float32)]
        ptr = [a.ctypes.data for a in out]

        def refused(fn, *words):
            try:
                fn()
            except MpcGpuError as e:
                assert all(w in str(e) for w in words), str(e)
            else:
                raise AssertionError("accepted: %s" % (words,))
            assert g.store_epoch() == epoch
            assert join() == before
        refused(lambda: g.upgma(1, np.zeros(1, np.float32)), "mpcgpu_upgma", "1 leaves")
        refused(lambda: g.upgma(0, np.zeros(1, np.float32)), "mpcgpu_upgma", "0 leaves")
        refused(lambda: g.upgma(65537, np.zeros(1, np.float32)), "mpcgpu_upgma", "65537", "65536")
        refused(lambda: g.upgma(5, tri, 4, "avg"), "mpcgpu_upgma", "transform 4")
        refused(lambda: g.upgma(5, tri, -1, "avg"), "mpcgpu_upgma", "transform -1")
        refused(lambda: g.upgma(5, tri, "none", 4), "mpcgpu_upgma", "linkage 4")
        for k in range(5):  # dist and each of the four outputs NULL
            args = [tri.ctypes.data] + ptr
            args[k] = None
            refused(lambda: g._ck(g.L.mpcgpu_upgma(g.h, 5, args[0], 0, 0, args[1], args[2], args[3], args[4])), "mpcgpu_upgma", "NULL")
        refused(lambda: g._ck(g.L.mpcgpu_upgma_info(g.h, None)), "mpcgpu_upgma_info", "NULL")
        refused(lambda: _sw._with_env({"MPCGPU_UPGMA_MEM_MB": "1"}, lambda: g.upgma(1025, U.make_tri(1025, "random", 3))),
                "mpcgpu_upgma", "1025 leaves", "device memory")
        # mpcgpu_sw_tree: no tables; then NULL, an unknown linkage
        refused(lambda: g.sw_tree(), "mpcgpu_sw_tree", "mpcgpu_sw_set_scores")
        g.sw_set_scores(*_sw.tables())
        assert g.store_epoch() == epoch
        refused(lambda: g.sw_tree(linkage=7), "mpcgpu_sw_tree", "linkage 7")
        refused(lambda: g._ck(g.L.mpcgpu_sw_tree(g.h, 0, None, ptr[1], ptr[2], ptr[3], None)), "mpcgpu_sw_tree", "NULL")
        # accepted calls are readers too
        got = g.upgma(5, tri, "scale", "avg")
        U.assert_same_tree(got, U.upgma(5, tri, "scale", "avg"), "after the refusals")
        g.sw_tree()
        assert g.store_epoch() == epoch and join() == before
    finally:
        g.close()


def _sw_tree_seqs():
    """70 synthetic sequences of lengths 5 .. 300"""
    fam = make_family(70, 310, seed=31)
    rng = np.random.default_rng(8)
    lens = [5, 300, 64, 65] + [int(x) for x in rng.integers(5, 301, 66)]
    return [s[:ln] for s, ln in zip(fam, lens)]


def test_sw_tree_is_scores_normalisation_upgma():
    seqs = _sw_tree_seqs()
    n = len(seqs)
    g = _sw.context(seqs)
    try:
        raw = g.sw_scores().copy()
        left, right, ll, rl, sc = g.sw_tree(want_scores=True)
        assert np.array_equal(_sw.bits(sc), _sw.bits(raw))
        info = g.upgma_info()
        assert info[0] == n and info[1] == 1
        lens = np.array([len(x) for x in seqs], np.uint32)
        iu = np.triu_indices(n, 1)
        mean = (lens[iu[0]] + lens[iu[1]]).astype(np.float32) / np.float32(2.0)  # swdistmx.cpp:75
        norm = (raw / mean).astype(np.float32)                                    # swdistmx.cpp:76
        U.assert_same_tree((left, right, ll, rl), U.upgma(n, norm, "scale", "avg"), "sw_tree")
        mn, mx = g.upgma_scale()
        assert mn == norm.min() and mx == norm.max()
        # without the scores, and another linkage
        U.assert_same_tree(g.sw_tree(linkage="biased"), U.upgma(n, norm, "scale", "biased"), "sw_tree biased")
    finally:
        g.close()


# ---- the drop-in: MUSCLE_GPU_UPGMA=1 (mpcgpu_sw_tree) against =0 (device scores, host UPGMA5) -----------------------------------
@pytest.fixture(scope="module")
def gpu_muscle():
    if not os.path.exists(_msa.GPU_MUSCLE):
        pytest.fail("hostcxx/_build/muscle_gpu missing: run __graft_entry__.build() where the reference sources are, "
                    "or where oracle/_ref/muscle_gpu built there travelled along")
    return _msa.GPU_MUSCLE


def _dropin_seqs():
    """40 related sequences, X-terminated: no best local alignment ends on a last residue (the comment above CalcGuideTree_SW_BLOSUM62)"""
    return [s + "X" for s in make_family(40, 60, seed=57)]


def test_dropin_swdistmx_same_newick(gpu_muscle):
    seqs = _dropin_seqs()
    on = D.swdistmx(gpu_muscle, seqs, env={"MUSCLE_GPU_UPGMA": "1"})
    off = D.swdistmx(gpu_muscle, seqs, env={"MUSCLE_GPU_UPGMA": "0"})
    assert on == off and on.count(",") == len(seqs) - 1


def test_dropin_super7_same_msa(gpu_muscle):
    seqs = _dropin_seqs()
    extra = ["-shrub_size", "10"]
    on = D.super7(gpu_muscle, seqs, extra, env={"MUSCLE_GPU_UPGMA": "1"})[0]
    off = D.super7(gpu_muscle, seqs, extra, env={"MUSCLE_GPU_UPGMA": "0"})[0]
    assert len(on) > 0 and hashlib.md5(on).hexdigest() == hashlib.md5(off).hexdigest()
