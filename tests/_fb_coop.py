"""fb_coop_kernel (muscle_amd/csrc/kernels_fbcoop.h): the row-block forward/backward sweep with the W waves of a workgroup on one
pair. Shared by tests/test_gpu_fb_coop.py (the device) and tests/test_emu_fb_coop.py (the SIMT emulator, which runs the waves of a
workgroup as fibers against its barrier).

Every check runs the same call twice on one context — MPCGPU_FB_COOP=0 (fb_kernel<H, MEGA, LONG>, one wave per pair) and
MPCGPU_FB_COOP=W — and asserts
  * both against the oracle, bit for bit: CalcAlnFlat path and score, EA, the sparse rows (offsets, columns, probability bits);
  * both against each other;
  * stage_a_coop_info() = (row-block pairs, W) for the forced run, (0, 0) for the other;
  * the same number of family-0 (forward/backward) launches.
Block edges are reached with short sequences: MPCGPU_FB_LONG_MIN=65 MPCGPU_FB_LONG_H=1 (blocks of 64 rows). Knobs are set around
the call and restored (the library reads them per call)."""
import numpy as np

import _align_pairs as A
import _golden as G
import _parity as P
from muscle_amd._lib import MpcGpu, MpcGpuError

FORCE_H1 = {"MPCGPU_FB_LONG_MIN": "65", "MPCGPU_FB_LONG_H": "1"}


def coop_env(base, W):
    return dict(base, MPCGPU_FB_COOP=str(W))


def run_list(g, seqs, pairs, env, mega=None):
    """mpcgpu_align_pairs of registry pairs under env -> (results, sparse rows, family-0 launches, stage_a_coop_info)"""
    xs, ys = [x for x, _ in pairs], [y for _, y in pairs]

    def run():
        g.timers_reset()
        res = g.align_pairs(xs, ys)
        rows = [A.list_sparse(g, q, len(seqs[xs[q]])) for q in range(len(xs))]
        return res, rows, g.timers_get()["fb"][1], g.stage_a_coop_info()
    return A.with_env(env, run)


def check_list(seqs, pairs, W, base_env=FORCE_H1, lib_path=None, mega=None, want_w=None, long_min=65, want_pairs=None):
    """the pairs (registry indices) as one mpcgpu_align_pairs list, with MPCGPU_FB_COOP = 0 and = W. want_w: the W the library must
    report (W itself unless it is clamped); want_pairs: the row-block pairs it must report (those with LX >= long_min)"""
    h, (s, t, m, i, thr) = A.hmm()
    wants = [A.oracle_pair(seqs, x, y, mega) for x, y in pairs]
    nlong = sum(1 for x, _ in pairs if len(seqs[x]) >= long_min) if want_pairs is None else want_pairs
    g = MpcGpu(0, lib_path)
    try:
        g.set_hmm(s, t, m, i, thr)
        g.set_seqs_registry(seqs)
        if mega is not None:
            g.set_mega(mega["alpha"], mega["weight"], mega["lp"], mega["mx"], mega["profs"])
        g.timers_enable(True)
        off = run_list(g, seqs, pairs, coop_env(base_env, 0), mega)
        on = run_list(g, seqs, pairs, coop_env(base_env, W), mega)
    finally:
        g.close()
    for tag, (res, rows, fam0, info) in (("MPCGPU_FB_COOP=0", off), ("MPCGPU_FB_COOP=%d" % W, on)):
        for q, ((p, sc, ea), (o, v), w) in enumerate(zip(res, rows, wants)):
            assert p == w["path"], (tag, q, pairs[q], "path")
            assert A.bits(sc) == A.bits(w["score"]) and A.bits(ea) == A.bits(w["ea"]), (tag, q, pairs[q], "score / EA", sc, w["score"], ea, w["ea"])
            assert len(v) == len(w["val"]), (tag, q, pairs[q], "nnz", len(v) // 2, len(w["val"]) // 2)
            assert np.array_equal(o, w["off"]) and np.array_equal(v, w["val"]), (tag, q, pairs[q], "sparse rows")
    for q, (a, b) in enumerate(zip(off[0], on[0])):
        assert a[0] == b[0] and A.bits(a[1]) == A.bits(b[1]) and A.bits(a[2]) == A.bits(b[2]), (q, "cooperative against single-wave")
    for q, (a, b) in enumerate(zip(off[1], on[1])):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (q, "cooperative against single-wave: sparse rows")
    assert off[3] == (0, 0), ("MPCGPU_FB_COOP=0", off[3])
    assert on[3] == ((nlong, W if want_w is None else want_w) if nlong else (0, 0)), ("MPCGPU_FB_COOP=%d" % W, on[3], nlong)
    assert off[2] == on[2], ("family-0 launches", off[2], on[2])
    return on[3]


def pair_of(LX, LY, seed):
    """a registry of two related sequences of these lengths and the one pair (X, Y)"""
    return A.related([LX, LY], seed), [(0, 1)]


def all_pairs(seqs, env, lib_path=None, mega=None, iters=1):
    """mpcgpu_calc_posteriors over all pairs, mpcgpu_build_store, `iters` relax iterations -> ((stages, EA), coop info, family-0 launches)"""
    s, t, m, i, thr = G.hmm_tables()

    def run():
        g = MpcGpu(0, lib_path)
        try:
            g.set_hmm(s, t, m, i, thr)
            g.set_seqs(seqs)
            if mega is not None:
                g.set_mega(mega["alpha"], mega["weight"], mega["lp"], mega["mx"], mega["profs"])
            g.timers_enable(True)
            g.timers_reset()
            g.calc_posteriors()
            info, fam0 = g.stage_a_coop_info(), g.timers_get()["fb"][1]
            ea = g.get_ea().copy()
            g.build_store()
            stages = [g.get_sparse_range()]
            for _ in range(iters):
                g.cons_iter()
                g.cons_commit()
                stages.append(g.get_sparse_range())
            return (stages, ea), info, fam0
        finally:
            g.close()
    return A.with_env(env, run)


def check_all_pairs(seqs, W, base_env, nlong, lib_path=None, mega=None, want=None):
    """all pairs of seqs, COOP = 0 and = W, against the oracle (or `want`, a (stages, EA) of the same form) after one relax iteration"""
    if want is None:
        want = P.run_oracle(seqs, iters=1, mega=mega)
    off = all_pairs(seqs, coop_env(base_env, 0), lib_path, mega)
    on = all_pairs(seqs, coop_env(base_env, W), lib_path, mega)
    P.assert_same(off[0], want, "MPCGPU_FB_COOP=0")
    P.assert_same(on[0], want, "MPCGPU_FB_COOP=%d" % W)
    P.assert_same(on[0], off[0], "cooperative against single-wave")
    assert off[1] == (0, 0) and on[1] == (nlong, W), (off[1], on[1], nlong)
    assert off[2] == on[2], ("family-0 launches", off[2], on[2])


def check_no_memory(lib_path=None, L=20000):
    """a forced W against a plane budget (MPCGPU_SCRATCH_GB=0: 1 GB) smaller than one workgroup's planes (L x L floats): the call fails
    with a message before anything is launched, and the context goes on to serve a small list"""
    h, (s, t, m, i, thr) = A.hmm()
    seqs = A.related([L, L, 130, 70], 77)
    g = MpcGpu(0, lib_path)
    try:
        g.set_hmm(s, t, m, i, thr)
        g.set_seqs_registry(seqs)

        def big():
            try:
                g.align_pairs([0], [1])
                return None
            except MpcGpuError as e:
                return str(e)
        err = A.with_env({"MPCGPU_SCRATCH_GB": "0", "MPCGPU_FB_COOP": "4"}, big)
        assert err is not None and "not enough device memory for the forward plane" in err, err
        assert g.stage_a_coop_info() == (0, 0)
        res, rows, _, info = run_list(g, seqs, [(2, 3)], coop_env(FORCE_H1, 2))
        w = A.oracle_pair(seqs, 2, 3)
        assert res[0][0] == w["path"] and A.bits(res[0][1]) == A.bits(w["score"]) and np.array_equal(rows[0][1], w["val"])
        assert info == (1, 2), info
    finally:
        g.close()
