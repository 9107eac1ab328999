"""The device joins on MI355X at production shapes, every path of the dispatcher (muscle_amd/csrc/mpcgpu_joins.inc) pinned bit for bit:
BuildPost's row form with 8 and 16 columns per lane, the row form that overflows its list, the general path (generating kernel,
rocprim radix sort, in-order reduction) reached without forcing and with MPCGPU_BP=sort, long runs of the reduction, the three
alignment kernels, align_alns_batch beyond one 1 GiB chunk, and align_msas on long pair lists. Each case proves the path it ran
(tests/_joins.py). MPCGPU_TEST_JOINS_SEEDS=k runs the row / general table over k seeds (default 1)."""
import os

import numpy as np
import pytest

import _buildpost as BP
import _joins as J
from muscle_amd.synth import make_family

pytestmark = pytest.mark.gpu

SEEDS = range(int(os.environ.get("MPCGPU_TEST_JOINS_SEEDS", "1")))


@pytest.fixture(scope="module")
def mid():
    """112 sequences: a family of 96 x L~120 and the poly-A pairs of J.HOMOPOLYMERS (at 96..111)"""
    ctx = J.Ctx(make_family(96, 120, seed=3) + J.HOMOPOLYMERS)
    yield ctx
    ctx.close()


def _groups(rng, n1, n2, n=96):
    """random disjoint rows of the family, with pairs stored in both orientations"""
    while True:
        perm = rng.permutation(n)
        g1, g2 = [int(x) for x in perm[:n1]], [int(x) for x in perm[n1:n1 + n2]]
        if min(g1) < max(g2) and min(g2) < max(g1):
            return g1, g2


# (name, n1, n2, Join arguments, path by default)
TABLE = [("row8", 8, 8, {}, "row"), ("row8 C2=512", 8, 8, {"C2": 512}, "row"), ("row16 C2=513", 8, 8, {"C2": 513}, "row"),
         ("row16 C2=1024", 8, 8, {"C2": 1024}, "row"), ("row8 2048 pairs", 32, 64, {}, "row"),
         ("row8 1 x 95", 1, 95, {}, "row"), ("row16 95 x 1", 95, 1, {"C2": 700}, "row"),
         ("general 46 x 46 pairs", 46, 46, {}, "general"), ("general C2=1100", 8, 8, {"C2": 1100}, "general")]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("mode", [None, "sort"])
@pytest.mark.parametrize("case", [c[0] for c in TABLE])
def test_join_paths(mid, case, mode, seed):
    """each case on its own path, and again forced through the general path (MPCGPU_BP=sort)"""
    name, n1, n2, kw, path = next(c for c in TABLE if c[0] == case)
    rng = np.random.default_rng(1000 * seed + len(name))
    j = mid.join(*_groups(rng, n1, n2), rng, **kw)
    mid.check(j, path if mode is None else "general", mode=mode, what=name)


def test_row_list_overflow(mid):
    """64 pairs whose output rows list ~1700 entries: the row kernel reports the overflow and the general path redoes the join"""
    j = mid.join(*J.overflow_groups(96), np.random.default_rng(4))
    assert BP.row_chunk_max(mid.stage, mid.pidx, j.grp1, j.grp2, j.m1, j.C1) > J.BPR_CAP
    mid.check(j, "overflow", what="row list overflow")


def test_alignment_kernels_traced():
    """one join ending in each alignment kernel (the class above 4096 columns: two sequences of 4200 residues) and the overflowed
    row form, proven by the MPCGPU_TRACE=1 lines of a child process"""
    J.check_aln_cases_traced(None, "gpu", timeout=400)


def test_long_runs_at_scale():
    """a 200 x L~400 family split 100 x 100 (even / odd: both stored orientations): cells collect more than 4096 terms and the
    radix sort orders more than 5 * 10^6 records; the 1 x 199 and 199 x 1 splits"""
    seqs = make_family(200, 400, seed=8)
    ctx = J.Ctx(seqs)
    try:
        rng = np.random.default_rng(3)
        j = ctx.join(list(range(0, 200, 2)), list(range(1, 200, 2)), rng)
        cnt, total = BP.term_counts(ctx.stage, ctx.pidx, *j.args())
        assert cnt.max() > 4096 and (cnt > 512).sum() > 100 and (cnt > 64).sum() > 1000, (cnt.max(), (cnt > 512).sum())
        assert total >= 5_000_000, total
        ctx.check(j, "general", what="100 x 100")
        others = [q for q in range(200) if q != 100]
        ctx.check(ctx.join([100], others, rng), "row", what="1 x 199")
        ctx.check(ctx.join(others, [100], rng), "row", what="199 x 1")
    finally:
        ctx.close()


def test_align_alns_batch_level_scale(mid):
    """860 one-wave joins of 638 x 511 cells (more than the 1 GiB budget of one chunk: two chunks) mixed with joins that are not
    small (C2 + 1 > 512, 46 x 46 pairs), results in list order; a batch whose chunk overflows the row form's list; a batch of one"""
    rng = np.random.default_rng(9)
    joins = []
    for q in range(860):
        a, b = (int(x) for x in rng.choice(96, 2, replace=False))
        joins.append(mid.join([a], [b], rng, C1=638, C2=511))
    joins.insert(100, mid.join(*_groups(rng, 3, 2), rng, C2=600))
    joins.insert(500, mid.join(*_groups(rng, 46, 46), rng))
    chunks, single = mid.check_batch(joins, "level")
    assert len(chunks) == 2 and single == [100, 500], (len(chunks), single)
    over = mid.join(*J.overflow_groups(96), rng)
    chunks, single = mid.check_batch([joins[0], over, joins[100], joins[1]], "overflowed chunk")
    assert chunks == [[0, 1, 3]] and sorted(single) == [0, 1, 2, 3]
    chunks, single = mid.check_batch([joins[7]], "batch of one")
    assert chunks == [] and single == [0]


def test_align_msas_long_lists():
    """2500 pairs over more than 512 columns, repeated sequences, MSA1 sequences with the larger index and the smaller"""
    rng = np.random.default_rng(13)
    seqs = make_family(100, 150, seed=12)
    grp1 = [int(x) for x in rng.integers(0, 50, 50) * 2]
    grp2 = [int(x) for x in rng.integers(0, 50, 50) * 2 + 1]
    pairs = [(a, b) for a in range(50) for b in range(50)]
    C1, C2, npairs = J.check_align_msas(seqs, grp1, grp2, pairs, rng, extra=400, what="2500 pairs")
    assert npairs > 2048 and min(C1, C2) > 512
