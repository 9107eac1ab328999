"""What the named UPGMA cases of tests/_upgma.py reach, shown on the CPU without the library: run()'s counters per tree (which joins
take a row beyond the first stride of the join workgroup, which are decided by a tie across waves or strides, which redirect, which pick a
stale minimum), the launcher of mpcgpu_upgma.inc restated (grids, passes, partials, the LDS cut and request), where "extremes_at" puts Min
and Max, and which refusal the reference makes of every input that is there to be refused. The device tests (tests/test_gpu_upgma.py) and
the emulator tests (tests/test_emu_upgma.py) run these cases; this file is why they are the right ones.

Floors, not measured values: each is what the path needs to be called reached "in most joins" / "in some joins", below what the seeded
matrices give (quant, 2100 leaves, T = 1024: a row beyond the first stride is Lmin in 821-1076 joins under avg / max / biased, random:
860-932; Rmin in about 1075; the argmin is tied across strides in 2044-2099 joins (quant) and 277-930 (random); the new row's minimum in 9
(avg), 89 (biased), 2034 (max) and 2046 (min) joins. 300 leaves, T = 128: Lmin 169-174, ties across strides 253-299, redirects in 16-292
joins, stale picks 280-288)."""
import numpy as np
import pytest

import _upgma as U

_STATS = {}


def stats(n, kind, transform, linkage, T):
    key = (n, kind, transform, linkage, T)
    if key not in _STATS:
        st = U.new_stats(T)
        try:
            U.upgma_full(n, U.make_tri(n, kind, 1000 + n), transform, linkage, st)
        except U.UpgmaDies:
            pass
        _STATS[key] = st
    return _STATS[key]


# floors per (kind, linkage) as fractions of the n - 1 joins: (Lmin >= T, argmin tied across strides, new minimum tied across strides,
# joins with a redirect, stale picks; None: no claim, 0: must not occur)
FLOORS = {
    ("quant", "avg"): (0.35, 0.8, 5, 0.9, 0.9),
    ("quant", "min"): (None, 0.9, 0.8, 15, 0),
    ("quant", "max"): (0.35, 0.8, 0.8, 0.9, 0.9),
    ("quant", "biased"): (0.35, 0.8, 6, 0.7, 0.7),
    ("random", "avg"): (0.35, 0.1, None, 0.6, 0.7),
    ("random", "min"): (0.08, 0.4, None, 0.4, 0),
    ("random", "max"): (0.35, 0.1, None, 0.6, 0.7),
    ("random", "biased"): (0.35, 0.1, None, 0.6, 0.7),
}


def _at_least(st, key, floor, what):
    if floor is None:
        return
    if floor == 0:
        assert st[key] == 0, (what, key, st[key])
    else:
        need = floor if floor >= 1 else int(floor * st["joins"])
        assert st[key] >= need, (what, key, st[key], need)


@pytest.mark.parametrize("linkage", U.LINKAGES)
@pytest.mark.parametrize("kind", U.STRIDE_KINDS)
@pytest.mark.parametrize("where", ["gpu", "emu"])
def test_stride_cases_reach_the_second_stride(where, kind, linkage):
    n, T = U.STRIDE_N[where], U.JOIN_THREADS[where]
    assert n > 2 * T and n % T != 0
    for transform in ("none", "scale"):
        st = stats(n, kind, transform, linkage, T)
        what = (where, kind, transform, linkage)
        assert st["joins"] == n - 1 and st["dies_at"] is None, what
        fl = FLOORS[(kind, linkage)]
        _at_least(st, "L_ge_T", fl[0], what)
        _at_least(st, "R_ge_T", 0.45, what)  # the right child of about every second join lies beyond the first stride
        _at_least(st, "argmin_tied_strides", fl[1], what)
        assert st["argmin_tied_waves"] >= 1 and st["argmin_tied"] >= st["argmin_tied_strides"], what
        _at_least(st, "newmin_tied_strides", fl[2], what)
        _at_least(st, "redirect_joins", fl[3], what)
        assert st["redirects"] >= st["redirect_joins"], what
        _at_least(st, "stale_picks", fl[4], what)
        if linkage == "min":
            # the new row keeps the smaller of two distances, so its cached minimum is never above what it was taken from, the lowest
            # row among equals is the left child, and no pick is stale
            assert st["L_gt_R"] == 0 and st["stale_picks"] == 0, what
        else:
            _at_least(st, "L_gt_R", 0.3, what)


def test_counters_do_not_change_the_tree():
    for kind, transform, linkage in (("quant", "scale", "max"), ("random", "none", "biased"), ("nan_mid", "none", "avg")):
        tri = U.make_tri(129, kind, 7)
        res = []
        for st in (None, U.new_stats(128), U.new_stats(1024)):
            try:
                res.append(U.upgma_full(129, tri, transform, linkage, st))
            except U.UpgmaDies as e:
                res.append(e)
                assert st is None or st["dies_at"] == e.join
        for r in res[1:]:
            if isinstance(res[0], U.UpgmaDies):
                assert U.outcome(r) == U.outcome(res[0])
            else:
                assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(r, res[0]))


def test_matrix_by_rows_is_the_triangle():
    for n in (2, 3, 65, 257, 600):
        tri = U.make_tri(n, "zeros_both" if n >= 65 else "random", 3)
        mx = U.mx_of(n, tri, 5.0)
        iu = np.triu_indices(n, 1)
        assert np.array_equal(mx[iu].view(np.uint32), tri.view(np.uint32)) and np.array_equal(mx.T[iu].view(np.uint32), tri.view(np.uint32))
        assert np.all(mx.diagonal() == 5.0) and np.array_equal(U.tri_of(mx).view(np.uint32), tri.view(np.uint32))


def test_launch_geometry():
    """upgma_run's arithmetic (mpcgpu_upgma.inc) at the CU counts of MI355X (256) and MI300X (304)"""
    n = U.STRIDE_N["gpu"]
    m = U.n_tri(n)
    assert m == 2203950
    assert U.grid(m, 256) == 2048 and U.passes(m, 256) == 5 and U.passes(m, 256) > 4 and U.fold_rounds(m, 256) == 8
    assert U.grid(m, 304) == 2432 and U.passes(m, 304) == 4 and U.fold_rounds(m, 304) == 10
    assert U.grid(1, 256) == 1 and U.grid(257, 256) == 2 and U.passes(256, 256) == 1
    # n = 1025, the largest size before: 512 entries in a second pass
    assert U.n_tri(1025) - U.grid(U.n_tri(1025), 256) * 256 == 512
    for cus in (256, 304):
        assert U.init_row_passes(12289, cus) == 2 and U.init_row_passes(32 * cus, cus) == 1 and U.init_row_passes(32 * cus + 1, cus) == 2
        assert U.init_row_passes(n, cus) == 1
    assert U.sw_norm_grid(n, 256) == 2048 and n - 1 > 8 * 256  # upgma_sw_norm_kernel strides its rows at 2100 sequences on 256 CUs
    assert U.sw_norm_grid(70, 256) == 69
    assert U.lds_cut() == 12288 and U.lds_cut(0) == 0 and U.lds_cut(-5) == 0 and U.lds_cut(65) == 65 and U.lds_cut(1 << 20) == 12288
    assert U.join_lds(12288) == (True, 147712) and 147712 <= 160 * 1024
    assert U.join_lds(12289) == (False, 256)
    assert U.join_lds(65, 64) == (False, 256) and U.join_lds(65, 65) == (True, 256 + 65 * 12)
    # the emulator: 2 CUs, 16 workgroups
    me = U.n_tri(U.STRIDE_N["emu"])
    assert U.grid(me, 2) == 16 and U.passes(me, 2) == 11 and U.fold_rounds(me, 2) == 1 and U.init_row_passes(300, 2) == 5


@pytest.mark.parametrize("where,cus", [("gpu", 256), ("gpu", 304), ("emu", 2)])
def test_extremes_positions(where, cus):
    n = U.STRIDE_N[where]
    m, g = U.n_tri(n), U.grid(U.n_tri(n), cus)
    (mn0, mx0), (mn1, mx1) = U.extremes_positions(n, cus)
    per = g * 256
    assert mn0 == m - 1 and mn0 // per == U.passes(m, cus) - 1  # the last entry, in the last pass
    assert mx0 == per and mx0 // per == 1 and (mx0 % per) // 256 == 0  # first entry of the second pass: workgroup 0 again
    assert mn1 < per and mx1 < per  # first pass
    if where == "gpu":
        assert mn1 // 256 == 256 and mn1 % 256 == 255 and mx1 // 256 == g - 1 >= 256 and mx1 % 256 == 0
        # partial q is folded by lane q % 256 in round q // 256: both in a later round than the first
        assert (mn1 // 256) // 256 >= 1 and (mx1 // 256) // 256 >= 1
    for pos in U.extremes_positions(n, cus):
        tri = U.make_tri(n, ("extremes_at",) + pos, 1000 + n)
        assert int(np.argmin(tri)) == pos[0] and int(np.argmax(tri)) == pos[1]
        assert (tri == tri.min()).sum() == 1 and (tri == tri.max()).sum() == 1
        assert U.device_min_max(tri) == (np.float32(0.125), np.float32(0.875))


@pytest.mark.parametrize("where", ["gpu", "emu"])
def test_edge_cases_are_what_they_are_named(where):
    FLT_MIN = np.finfo(np.float32).tiny
    for n, kind, transform, linkage in U.edge_cases(where):
        name = kind if isinstance(kind, str) else kind[0]
        tri = U.make_tri(n, kind, 1000 + n)
        bits = tri.view(np.uint32)
        m = len(tri)
        got = U.outcome(U.want(n, kind, transform, linkage))
        what = (n, kind, transform, linkage, got)
        if (name, transform) in U.REFUSED:
            assert got == U.REFUSED[(name, transform)], what
        elif name in ("nan_mid", "inf"):
            assert got == "tree" or got[0] == "no_min", what  # whichever the reference's procedure gives; the device must give the same
        else:
            assert got == "tree", what
        if name == "subnormal":
            assert np.all((tri > 0) & (tri < FLT_MIN)) and (bits == 1).sum() >= 3 and len(np.unique(tri)) < m
            assert (U.SUB_MIN / np.float32(2)) == 0
        elif name == "zeros_both":
            z = np.nonzero(tri == 0)[0]
            assert list(bits[z]) == [0, 0, 0x80000000, 0x80000000] and z[0] == 0 and z[-1] == m - 2 and np.all(np.delete(tri, z) > 0)
            mx = U.mx_of(n, tri)
            assert [U.float_bits(x) for x in U.fold_min_max(mx)][0] == 0  # the reference keeps the +0 it meets first
            assert U.float_bits(U.device_min_max(tri)[0]) == 0x80000000   # the device: -0 is the Min
        elif name == "zeros_both_max":
            z = np.nonzero(tri == 0)[0]
            assert list(bits[z]) == [0x80000000, 0x80000000, 0, 0] and np.all(np.delete(tri, z) < 0)
            assert U.float_bits(U.fold_min_max(U.mx_of(n, tri))[1]) == 0x80000000 and U.float_bits(U.device_min_max(tri)[1]) == 0
        elif name == "nan_mid":
            assert np.isnan(tri).sum() == 3 and not np.isnan(tri[0])
            mn, ma = U.fold_min_max(U.mx_of(n, tri))
            assert mn == np.nanmin(tri) and ma == np.nanmax(tri) and U.device_min_max(tri) == (mn, ma)  # skipped, as the reference does
        elif name == "nan_first":
            assert np.isnan(tri[0]) and np.isnan(tri).sum() == 1
            assert all(np.isnan(x) for x in U.fold_min_max(U.mx_of(n, tri)) + U.device_min_max(tri))
        elif name == "inf":
            assert np.isposinf(tri).sum() == 2
        elif name == "ea_edge_ok":
            assert np.all((tri >= 0) & (tri <= 1)) and (bits == 0x80000000).any() and (bits == 0).any() and (tri == 1).any()
        elif name == "ea_one_bad":
            assert np.all((tri[:-1] >= 0) & (tri[:-1] <= 1)) and not (tri[-1] >= 0 and tri[-1] <= 1)
            assert U.float_bits(tri[-1]) == U.float_bits(U.EA_BAD[kind[1]])
            # the last entry lies in the last pass of the transform kernel's grid-stride loop, in a workgroup that is not workgroup 0
            cus = U.CUS[where]
            per = U.grid(m, cus) * 256
            assert ((m - 1) % per) // 256 != 0
    assert {U.float_bits(v) for v in U.EA_BAD.values()} == {0x3F800001, 0x80000001, 0x7FC00000}


def test_zero_rule_is_the_only_difference_from_the_reference_fold():
    """the tree under the device's Min / Max against the tree under the reference's own fold: equal for every edge matrix but the two whose
    extreme is a zero of both signs, where the sign of a zero distance (and of a zero branch length) follows the extreme's"""
    for n, kind, transform, linkage in U.edge_cases("gpu"):
        if transform not in ("scale", "scale_dist") or n > 129:
            continue
        tri = U.make_tri(n, kind, 1000 + n)
        try:
            ref = U.run(U.transform_mx(U.mx_of(n, tri, 0.0), transform), linkage)[:4]
        except U.UpgmaDies as e:
            ref = e
        dev = U.want(n, kind, transform, linkage)
        if isinstance(ref, U.UpgmaDies) or isinstance(dev, U.UpgmaDies):
            assert U.outcome(ref) == U.outcome(dev), (kind, transform, linkage)
            continue
        same = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(ref, dev))
        if kind in ("zeros_both", "zeros_both_max"):
            assert np.array_equal(ref[0], dev[0]) and np.array_equal(ref[1], dev[1])  # the same joins
            for a, b in zip(ref[2:], dev[2:]):
                assert np.array_equal(a, b)  # equal as numbers: only signs of zeros differ
        else:
            assert same, (kind, transform, linkage)
