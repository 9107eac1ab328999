"""The vectorised restatements of BuildPost and CalcPosteriorFlat3 (tests/_buildpost.py: build_post_fast, build_post_list_fast), which
the path-pinned join tests use at production shapes, against the loop forms on random stores and against the matrices the compiled
reference produced (tests/golden/bp_*.npz), bit for bit. CPU only."""
import numpy as np
import pytest

import _buildpost as BP
import _golden as G
import _oracle as O
import _parity as P


def _random_store(lens, rng, density):
    """a random MySparseMx-layout matrix per pair (i < j, pair-index order): rows ascending, columns ascending per row"""
    n = len(lens)
    stage = []
    for a in range(n):
        for b in range(a + 1, n):
            off, cols, probs = [0], [], []
            for _ in range(lens[a]):
                k = int(rng.binomial(lens[b], density))
                cols.extend(np.sort(rng.choice(lens[b], size=k, replace=False)).tolist())
                probs.extend(rng.uniform(0.0, 1.0, k).astype(np.float32).tolist())
                off.append(len(cols))
            val = np.empty(2 * len(cols), np.uint32)
            val[0::2] = np.asarray(probs, np.float32).view(np.uint32)
            val[1::2] = np.asarray(cols, np.uint32)
            stage.append((np.asarray(off, np.uint32), val))
    pidx = {p: k for k, p in enumerate((a, b) for a in range(n) for b in range(a + 1, n))}
    return stage, pidx


@pytest.mark.parametrize("seed", range(6))
def test_fast_build_post_equals_loop(seed):
    """random stores (dense enough that cells collect many terms), random groups in both stored orientations, 1 x n and n x 1,
    plain and weighted"""
    rng = np.random.default_rng(seed)
    n = 9
    lens = rng.integers(1, 14, n).tolist()
    seqs = ["A" * L for L in lens]
    stage, pidx = _random_store(lens, rng, 0.5)
    perm = rng.permutation(n).tolist()
    groups = [(perm[:4], perm[4:]), (perm[4:], perm[:4]), ([perm[0]], perm[1:]), (perm[1:], [perm[0]]), ([perm[2]], [perm[3]])]
    for grp1, grp2 in groups:
        rows1, C1 = BP.random_msa(seqs, grp1, rng)
        rows2, C2 = BP.random_msa(seqs, grp2, rng)
        m1 = [BP.pos_to_col(r) for r in rows1]
        m2 = [BP.pos_to_col(r) for r in rows2]
        w1 = rng.uniform(0.2, 1.8, len(grp1)).astype(np.float32)
        w2 = rng.uniform(0.2, 1.8, len(grp2)).astype(np.float32)
        for w in ((None, None), (w1, w2)):
            want = BP.build_post(stage, pidx, grp1, grp2, m1, m2, C1, C2, *w)
            got = BP.build_post_fast(stage, pidx, grp1, grp2, m1, m2, C1, C2, *w)
            assert np.array_equal(P.bits(got), P.bits(want)), (seed, grp1, grp2, w[0] is not None)
        cnt, total = BP.term_counts(stage, pidx, grp1, grp2, m1, m2, C1, C2)
        assert total == sum(len(stage[pidx[(min(S, T), max(S, T))]][1]) // 2 for S in grp1 for T in grp2)
        assert (got[cnt == 0] == 0).all()
        if min(len(grp1), len(grp2)) > 1:
            assert cnt.max() > 2  # cells that add several pairs' terms: the order of addition matters


@pytest.mark.parametrize("seed", range(4))
def test_fast_build_post_list_equals_loop(seed):
    """pair lists with repeated pairs and rows, in list order"""
    rng = np.random.default_rng(100 + seed)
    lens = rng.integers(1, 14, 6).tolist()
    seqs = ["A" * L for L in lens]
    stage, pidx = _random_store(lens, rng, 0.5)
    npairs = int(rng.integers(1, 40))
    X = rng.integers(0, 6, npairs).tolist()
    Y = [int((x + rng.integers(1, 6)) % 6) for x in X]
    C1, C2 = max(lens) + 5, max(lens) + 7
    sparse, m1, m2 = [], [], []
    for x, y in zip(X, Y):
        off, val = stage[pidx[(min(x, y), max(x, y))]]
        if x > y:  # the list form wants the MSA1 sequence on the rows: transpose the stored matrix
            d = np.zeros((lens[y], lens[x]), np.float32)
            rows, cols, p = BP._entries(off, val)
            d[rows, cols] = p
            d = d.T
            r, c = np.nonzero(d)
            off = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=lens[x]))]).astype(np.uint32)
            val = np.empty(2 * len(r), np.uint32)
            val[0::2], val[1::2] = d[r, c].view(np.uint32), c
        sparse.append((off, val))
        m1.append(np.sort(rng.choice(C1, lens[x], replace=False)).astype(np.uint32))
        m2.append(np.sort(rng.choice(C2, lens[y], replace=False)).astype(np.uint32))
    want = BP.build_post_list(sparse, m1, m2, C1, C2)
    got = BP.build_post_list_fast(sparse, m1, m2, C1, C2)
    assert np.array_equal(P.bits(got), P.bits(want))


@pytest.mark.parametrize("name", P.BP_SETS)
def test_fast_restatements_vs_reference_golden(name):
    """on the oracle's store after two consistency iterations, both forms reproduce the compiled reference's BuildPost matrices
    (plain and weighted) and CalcPosteriorFlat3 matrices (posteriors of the listed pairs from the oracle)"""
    z = G.load(name)
    seqs = [str(x) for x in z["seqs"]]
    stages, _ = P.run_oracle(seqs)
    stage = stages[2]
    n = len(seqs)
    pidx = {p: k for k, p in enumerate((a, b) for a in range(n) for b in range(a + 1, n))}
    for j in range(int(z["njoins"])):
        k = "j%d_" % j
        grp1, grp2 = [int(x) for x in z[k + "idx1"]], [int(x) for x in z[k + "idx2"]]
        rows1, rows2 = [str(x) for x in z[k + "rows1"]], [str(x) for x in z[k + "rows2"]]
        C1, C2 = len(rows1[0]), len(rows2[0])
        m1, m2 = [BP.pos_to_col(r) for r in rows1], [BP.pos_to_col(r) for r in rows2]
        w = z[k + "w"]  # indexed by the row inside each alignment (buildpostflat.cpp:42,52)
        for form in (BP.build_post, BP.build_post_fast):
            got = form(stage, pidx, grp1, grp2, m1, m2, C1, C2)
            assert np.array_equal(P.bits(got), P.bits(z[k + "post"])), (name, j, form.__name__)
            got = form(stage, pidx, grp1, grp2, m1, m2, C1, C2, w[:len(grp1)], w[:len(grp2)])
            assert np.array_equal(P.bits(got), P.bits(z[k + "postw"])), (name, j, form.__name__, "weighted")
    s, t, m, i, _ = G.hmm_tables()
    h = O.make_hmm(s, t, m, i)
    for j in range(int(z["nmsas"])):
        k = "m%d_" % j
        grp1, grp2 = [int(x) for x in z[k + "idx1"]], [int(x) for x in z[k + "idx2"]]
        rows1, rows2 = [str(x) for x in z[k + "rows1"]], [str(x) for x in z[k + "rows2"]]
        C1, C2 = len(rows1[0]), len(rows2[0])
        r1, r2 = [int(x) for x in z[k + "row1"]], [int(x) for x in z[k + "row2"]]
        sparse = []
        for a, b in zip(r1, r2):
            x, y = seqs[grp1[a]].encode(), seqs[grp2[b]].encode()
            sparse.append(O.sparse_from_post(O.post(O.fwd(h, x, y), O.bwd(h, x, y), len(x), len(y))))
        m1, m2 = [BP.pos_to_col(rows1[a]) for a in r1], [BP.pos_to_col(rows2[b]) for b in r2]
        for form in (BP.build_post_list, BP.build_post_list_fast):
            got = form(sparse, m1, m2, C1, C2)
            assert np.array_equal(P.bits(got), P.bits(z[k + "post"])), (name, j, form.__name__)
