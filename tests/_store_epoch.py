"""mpcgpu_store_epoch (include/mpcgpu.h) through the C ABI: which calls move the counter, which leave it, and that an unmoved
counter means the store a caller fingerprinted is still the memory it left — on an 8 x 60 family, the join's path and matrix
against the oracle (tests/_oracle.py) and the restatement of BuildPost (tests/_buildpost.py). Shared by
tests/test_gpu_store_epoch.py (the device) and tests/test_emu_store_epoch.py (the emulator build of the same sources).
TEST INFRASTRUCTURE."""
import numpy as np

import _buildpost as BP
import _golden as G
import _oracle as O
import _parity as P
from muscle_amd._lib import MpcGpu, MpcGpuError, MpcGroup
from muscle_amd.synth import make_family

SEQS = make_family(8, 60, seed=5)
N = len(SEQS)
PIDX = {p: k for k, p in enumerate((a, b) for a in range(N) for b in range(a + 1, N))}
GRP1, GRP2 = [0, 3, 5], [1, 2, 6]  # both stored orientations occur: (0,1) and (3,1)
# the pair triangle of 8 sequences as two triangles and the rectangle between them: every pair once
RECTS_OK = [[0, 4, 0, 4], [0, 4, 4, 8], [4, 8, 4, 8]]
RECTS_TWICE = [[0, 4, 0, 4], [0, 4, 0, 4], [0, 4, 4, 8], [4, 8, 4, 8]]  # the pairs of the first triangle are listed twice

_ref = {}


def reference():
    """computed once: the oracle's matrices after 0..3 relax iterations, the join, and per iteration count the matrix BuildPost
    must give and CalcAlnFlat's path and score on it"""
    if not _ref:
        stages, ea = P.run_oracle(SEQS, iters=3)
        rng = np.random.default_rng(23)
        rows1, C1 = BP.random_msa(SEQS, GRP1, rng)
        rows2, C2 = BP.random_msa(SEQS, GRP2, rng)
        join = (GRP1, GRP2, [BP.pos_to_col(r) for r in rows1], [BP.pos_to_col(r) for r in rows2], C1, C2)
        _ref["stages"], _ref["ea"], _ref["join"] = stages, ea, join
        for it in (2, 3):
            post = BP.build_post_fast(stages[it], PIDX, *join)
            score, path = O.calc_aln(post)
            _ref[it] = (post, path, score)
        assert not np.array_equal(P.bits(_ref[2][0]), P.bits(_ref[3][0]))  # a third iteration is visible in this join
    return _ref


def new_ctx(lib_path=None, upto="commit", iters=2):
    """a context taken as far as `upto`: create | hmm | seqs | stage_a | store | iter (cons_iter of the first iteration queued, not
    committed) | commit (`iters` full iterations)"""
    s, t, m, i, thr = G.hmm_tables()
    g = MpcGpu(0, lib_path)
    steps = ["create", "hmm", "seqs", "stage_a", "store", "iter", "commit"]
    at = steps.index(upto)
    if at >= 1:
        g.set_hmm(s, t, m, i, thr)
    if at >= 2:
        g.set_seqs(SEQS)
    if at >= 3:
        g.calc_posteriors()
    if at >= 4:
        g.build_store()
    if at == 5:
        g.cons_iter()
    if at >= 6:
        for _ in range(iters):
            g.cons_iter()
            g.cons_commit()
    return g


def assert_join_is(g, it, what):
    """the join on g's store gives the oracle's path, score and matrix for a store of `it` relax iterations"""
    post, path, score = reference()[it]
    join = reference()["join"]
    p1, s1 = g.align_alns(*join)
    assert p1 == path and P.bits(s1) == P.bits(score), (what, "path / score")
    assert np.array_equal(P.bits(g.last_post(join[4], join[5])), P.bits(post)), (what, "matrix")


def check_readers_leave_it(lib_path=None):
    ref = reference()
    join = ref["join"]
    g = new_ctx(lib_path)
    try:
        e0 = g.store_epoch()
        assert e0 > 0
        ea = g.get_ea().copy()
        g.get_nnz()
        stage = g.get_sparse_range()
        path, score = g.align_alns(*join)
        (bpath, bscore), = g.align_alns_batch([join])
        post = g.build_post(*join)
        last = g.last_post(join[4], join[5])
        g.store_complete()
        g.relax_info()
        g.store_info()
        g.synchronize()
        assert g.store_epoch() == e0, "a reader moved the epoch"
        # ... and what they read is the oracle's two-iteration store
        assert np.array_equal(P.bits(ea), P.bits(ref["ea"]))
        for k, ((o1, v1), (o2, v2)) in enumerate(zip(stage, ref["stages"][2])):
            assert np.array_equal(o1, o2) and np.array_equal(v1, v2), ("pair", k)
        want_post, want_path, want_score = ref[2]
        assert path == want_path and bpath == want_path
        assert P.bits(score) == P.bits(want_score) and P.bits(bscore) == P.bits(want_score)
        assert np.array_equal(P.bits(post), P.bits(want_post)) and np.array_equal(P.bits(last), P.bits(want_post))
        assert_join_is(g, 2, "after the readers")
        assert g.store_epoch() == e0
    finally:
        g.close()


# call -> (state of the fresh context it is made on, the call)
def _same_hmm(g):
    s, t, m, i, thr = G.hmm_tables()
    g.set_hmm(s, t, m, i, thr)


def _commit_sub_range(g):
    first, count = g.values_slice(2, 5)
    assert count > 0
    g.cons_commit_range(first, count)


MOVERS = {
    "set_hmm, same tables": ("commit", _same_hmm),
    "set_seqs, same sequences": ("commit", lambda g: g.set_seqs(SEQS)),
    "calc_posteriors": ("seqs", lambda g: g.calc_posteriors()),
    "build_store": ("stage_a", lambda g: g.build_store()),
    "cons_iter": ("store", lambda g: g.cons_iter()),
    "cons_commit": ("iter", lambda g: g.cons_commit()),
    "cons_commit_range of a sub-range": ("iter", _commit_sub_range),
    "set_seqs_registry": ("commit", lambda g: g.set_seqs_registry(SEQS)),
    "accepted set_pair_order": ("seqs", lambda g: g.set_pair_order(RECTS_OK)),
    "accepted set_pair_order over a store": ("commit", lambda g: g.set_pair_order(RECTS_OK)),
}


def check_mover(name, lib_path=None):
    upto, call = MOVERS[name]
    g = new_ctx(lib_path, upto)
    try:
        e0 = g.store_epoch()
        call(g)
        assert g.store_epoch() > e0, name
    finally:
        g.close()


def check_list_stage_moves_it(lib_path=None):
    """set_seqs_registry + align_pairs of one pair, on a context that holds a store: either call alone moves the epoch"""
    g = new_ctx(lib_path)
    try:
        e0 = g.store_epoch()
        g.set_seqs_registry(SEQS)
        e1 = g.store_epoch()
        assert e1 > e0
        (path, score, ea), = g.align_pairs([0], [1])
        assert g.store_epoch() > e1
        assert len(path) >= max(len(SEQS[0]), len(SEQS[1]))
    finally:
        g.close()


def check_new_context_and_refusals(lib_path=None):
    g = new_ctx(lib_path, "create")
    try:
        assert g.store_epoch() == 0
    finally:
        g.close()
    g = new_ctx(lib_path)
    try:
        e0 = g.store_epoch()
        try:
            g.set_pair_order(RECTS_TWICE)
            raise AssertionError("a pair listed twice was accepted")
        except MpcGpuError as e:
            assert "listed twice" in str(e)
        assert g.store_epoch() == e0, "a refused set_pair_order moved the epoch"
        for refused in (lambda: g.cons_iter(0, g.npairs + 1), lambda: g.cons_commit_range(1 << 60, 1), lambda: g.calc_posteriors(3, 2)):
            try:
                refused()
                raise AssertionError("an out-of-range call was accepted")
            except MpcGpuError:
                pass
        assert g.store_epoch() == e0, "a call refused before it touched anything moved the epoch"
        assert_join_is(g, 2, "after the refused calls")  # "changes nothing": the store is still there, and still the same
    finally:
        g.close()


def check_epoch_guards_reuse(lib_path=None):
    """What the drop-in's ensemble reuse rests on. A stage plus two iterations; a caller that wants the same stage again and finds
    the epoch where it left it skips the work, and the untouched store gives the oracle's join for two iterations. One more
    iteration: the epoch has moved, and the same join's matrix is another one — a caller that fingerprinted the two-iteration
    store is told that this is no longer it."""
    g = new_ctx(lib_path)
    try:
        kept = g.store_epoch()
        stage2 = g.get_sparse_range()
        assert g.store_epoch() == kept
        # "the second identical run": guarded by the epoch, it is skipped
        ran_again = False
        if g.store_epoch() != kept:
            ran_again = True
            g.set_seqs(SEQS), g.calc_posteriors(), g.build_store()
        assert not ran_again
        assert_join_is(g, 2, "reused store")
        for (o1, v1), (o2, v2) in zip(g.get_sparse_range(), stage2):
            assert np.array_equal(o1, o2) and np.array_equal(v1, v2)
        assert g.store_epoch() == kept
        # a third iteration
        g.cons_iter()
        g.cons_commit()
        assert g.store_epoch() > kept
        join = reference()["join"]
        post3 = g.build_post(*join)
        assert not np.array_equal(P.bits(post3), P.bits(reference()[2][0])), "a third iteration left the join's matrix as it was"
        assert_join_is(g, 3, "after a third iteration")
    finally:
        g.close()


def check_group_moves_every_context(lib_path=None, devices=(0, 0)):
    """the mpcgpu_group_* calls move the epoch of every context of the group; reading results from rank 0 moves none"""
    s, t, m, i, thr = G.hmm_tables()
    grp = MpcGroup(list(devices), lib_path)
    try:
        def epochs():
            return [grp.ctx(r).store_epoch() for r in range(grp.size)]
        last = epochs()
        assert last == [0] * grp.size
        for name, call in (("set_hmm", lambda: grp.set_hmm(s, t, m, i, thr)), ("set_seqs", lambda: grp.set_seqs(SEQS)),
                           ("calc_posteriors", grp.calc_posteriors), ("cons_iter", grp.cons_iter), ("cons_iter", grp.cons_iter)):
            call()
            now = epochs()
            assert all(b > a for a, b in zip(last, now)), (name, last, now)
            last = now
        assert_join_is(grp.ctx(0), 2, "group, rank 0")
        assert epochs() == last
    finally:
        grp.close()
