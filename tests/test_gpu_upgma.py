"""mpcgpu_upgma, mpcgpu_sw_tree and mpcgpu_upgma_info on the device against the numpy restatement of UPGMA5 (tests/_upgma.py): node indices
equal, float bits of the branch lengths equal. Sizes: 2 (the first), 3, 65 (one past a wavefront) and 1025 (one past the workgroup of the
join kernel: a lane owns more than one row), each with every transform and linkage on a random matrix, a matrix of 4 distinct values (ties,
the neighbour redirect, stale minima), one with negative entries and one with FLT_MAX entries; 65 and 1025 again with the row state in
global memory. Where the reference itself asserts or dies (an EA value outside 0 .. 1; no distance below FLT_MAX left: a scaled matrix of
one value, FLT_MAX under "max") the library must refuse by name, as the same kind of refusal and naming the same join.

The named cases of tests/_upgma.py, which tests/test_upgma_table.py shows to reach their paths: 2100 leaves (rows in a second and a third
stride of the join workgroup: Lmin, Rmin, ties across strides, redirects, stale picks) in LDS and in global memory; Min and Max where only a
later pass of the grid-stride loops or a later round of the fold over the partials finds them (placed with the device's CU count);
subnormals, zeros of both signs, NaN, inf, EA values at and just beyond the ends of 0 .. 1; outputs untouched by a refusal; the largest
LDS request (12 288 leaves) and the first size in global memory with no knob set (12 289, which also strides upgma_init_kernel); one
context reused across sizes and refusals; mpcgpu_sw_tree on 2100 sequences (upgma_sw_norm_kernel strides its rows)."""
import hashlib
import os
import time

import numpy as np
import pytest
import torch  # before the library is loaded: one HIP runtime in the process, the one the CU count is read from

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


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


N = U.STRIDE_N["gpu"]


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("linkage", U.LINKAGES)
@pytest.mark.parametrize("kind", U.STRIDE_KINDS)
def test_upgma_strides(kind, linkage, lds):
    def run():
        for transform in ("none", "scale"):
            U.check_case(None, N, kind, transform, linkage, lds=lds)
    run() if lds else _sw._with_env({"MPCGPU_UPGMA_LDS_ROWS": "0"}, run)


def test_upgma_extremes():
    cus = _cus()
    m = U.n_tri(N)
    assert U.passes(m, cus) >= 2 and U.fold_rounds(m, cus) >= 2, (cus, "a triangle of %d leaves no longer reaches a second pass / round" % N)
    U.check_extremes(None, N, cus)


def test_upgma_value_edges():
    for n, kind, transform, linkage in U.edge_cases("gpu"):
        U.check_case(None, n, kind, transform, linkage, lds=True)


def test_upgma_value_edges_row_state_in_global_memory():
    def run():
        for n, kind, transform, linkage in U.edge_cases("gpu"):
            if kind in ("subnormal", "nan_mid", "nan_all"):
                U.check_case(None, n, kind, transform, linkage, lds=False)
    _sw._with_env({"MPCGPU_UPGMA_LDS_ROWS": "0"}, run)


def test_upgma_refusal_leaves_the_outputs():
    U.check_refusal_leaves_outputs(None, U.EA_BAD_N["gpu"], ("ea_one_bad", "nan"), "ea", "avg", "ea_range")
    U.check_refusal_leaves_outputs(None, U.SMALL_N["gpu"], "nan_all", "ea", "avg", "ea_range")
    U.check_refusal_leaves_outputs(None, U.SMALL_N["gpu"], "nan_first", "scale", "avg", "no_min")


@pytest.mark.parametrize("n,linkage,lds", [(12288, "avg", True), (12289, "biased", False)], ids=["lds_max", "global_natural"])
def test_upgma_natural_cut(n, linkage, lds):
    """no knob set: 12 288 leaves ask for 147 712 bytes of LDS, 12 289 run in global memory; both stride upgma_init_kernel's rows"""
    assert "MPCGPU_UPGMA_LDS_ROWS" not in os.environ
    cus = _cus()
    assert U.join_lds(n) == (lds, 147712 if lds else 256) and U.init_row_passes(n, cus) >= 2, (n, cus)
    t0 = time.time()
    U.want(n, "random", "scale", linkage)
    t1 = time.time()
    U.check_case(None, n, "random", "scale", linkage, lds=lds)
    info = U.ctx(None).upgma_info()
    print("n %d: restatement %.1f s, device call with the triangle's copy %.2f s, device transform + init %.3f ms, joins %.3f ms"
          % (n, t1 - t0, time.time() - t1, info[2] / 1e6, info[3] / 1e6))


def test_upgma_reuse():
    U.check_reuse(None, N, 65)


def _sw_tree_strides_seqs():
    """2100 sequences of 5 .. 40 positions, every seventh an exact copy of an earlier one: equal scores, equal distances"""
    fam = make_family(N, 44, seed=77)
    rng = np.random.default_rng(12)
    seqs = [s[:int(ln)] for s, ln in zip(fam, rng.integers(5, 41, N))]
    for i in range(7, N, 7):
        seqs[i] = seqs[int(rng.integers(0, i))]
    return seqs


def test_sw_tree_strides():
    seqs = _sw_tree_strides_seqs()
    n = len(seqs)
    assert n - 1 > 8 * _cus() and U.sw_norm_grid(n, _cus()) < n - 1  # upgma_sw_norm_kernel takes more than one row per workgroup
    g = _sw.context(seqs)
    try:
        raw = g.sw_scores().copy()
        lens = np.array([len(x) for x in seqs], np.uint32)
        mean = np.concatenate([(lens[i] + lens[i + 1:]).astype(np.float32) / np.float32(2.0) for i in range(n - 1)])  # swdistmx.cpp:75
        norm = (raw / mean).astype(np.float32)                                                                          # swdistmx.cpp:76
        assert len(np.unique(norm)) < len(norm) - n  # the copies (and short sequences anyway): distances tie
        for linkage in ("avg", "biased"):
            left, right, ll, rl, sc = g.sw_tree(linkage=linkage, want_scores=True)
            assert np.array_equal(_sw.bits(sc), _sw.bits(raw))
            info = g.upgma_info()
            assert info[0] == n and info[1] == 1
            U.assert_same_tree((left, right, ll, rl), U.upgma(n, norm, "scale", linkage), "sw_tree " + linkage)
            mn, mx = g.upgma_scale()
            assert (U.float_bits(mn), U.float_bits(mx)) == tuple(U.float_bits(x) for x in U.device_min_max(norm))
    finally:
        g.close()


def test_sw_tree_refuses_a_long_sequence():
    U.check_long_sequence_refused(None)


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
