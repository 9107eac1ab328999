"""The LONG form of the record store and of relax_band_kernel (kernels_store.h: 32-bit block distances and entry positions;
MpcRbLongCxx, kernels_relaxb.h) against the oracle, bit for bit. Shared by tests/test_gpu_relax_long.py (MI355X) and
tests/test_emu_relax_long.py (the same source on the emulator). Runs go through tests/_relax.py's run_store: EA, the store after
the build and after each of two iterations (mpcgpu_get_sparse_range) equal P.run_oracle's, 0 ulp; relax_info names the path.

What the inputs are claimed to be is asserted from the oracle's matrices (check_forced_claims, record_blocks).
TEST INFRASTRUCTURE."""
import functools

import numpy as np

import _joins as J
import _relax as R
from muscle_amd._lib import MpcGpu
from muscle_amd.synth import make_family
import _golden as G

LONG = ("band-long", "relax_band_kernel", "MpcRbLongCxx")
FORCE = {"MPCGPU_RELAX_LONG": "1"}


@functools.lru_cache(None)
def forced_seqs(n):
    """n sequences of ragged lengths 5 .. 120: a family (rows store cells), one sequence of ONE residue, and one unrelated
    sequence (pairs with rows that store no cell)"""
    fam = make_family(n, 120, seed=20 + n)
    lens = [120, 5, 47, 88, 13, 101, 64, 29, 117][:n]
    seqs = [s[:ln] for s, ln in zip(fam, lens)]
    seqs[1] = seqs[0][40:41]                              # 1 residue
    if n >= 5:
        seqs[3] = make_family(1, 88, seed=77)[0][:88]      # unrelated to the family
    else:
        seqs[2] = make_family(1, 47, seed=77)[0][:47]
    return tuple(seqs)


def check_forced_claims(seqs):
    st = R.oracle(seqs)[0][0]
    assert min(len(s) for s in seqs) == 1 and max(len(s) for s in seqs) <= 120 and min(len(s) for s in seqs[2:]) >= 5
    assert any(len(v) > 0 and any(o[i + 1] == o[i] for i in range(len(o) - 1)) for o, v in st), "no pair with a row that stores no cell"
    assert any(any(o[i + 1] - o[i] > 2 for i in range(len(o) - 1)) for o, v in st), "no row with an overflow block"


def record_blocks(seqs):
    """largest record of the store in 16-byte blocks: len(A) + sum over rows of max(ceil(count / 2) - 1, 0), both orientations"""
    st = R.oracle(seqs)[0][0]
    n = len(seqs)
    best, k = 0, 0
    for x in range(n):
        for y in range(x + 1, n):
            o, v = st[k]
            k += 1
            rows = np.diff(np.asarray(o, np.int64))
            cols = np.bincount(np.asarray(v[1::2], np.int64), minlength=len(seqs[y]))
            for ln, cnt in ((len(seqs[x]), rows), (len(seqs[y]), cols)):
                best = max(best, ln + int(np.maximum((cnt + 1) // 2 - 1, 0).sum()))
    return best


def run(seqs, env, has=(), lacks=(), fallback=False, lib_path=None, store=(), store_not=()):
    """one store under env: build, two iterations, everything against the oracle; relax_info after each iteration"""
    r = R.Run("long form", seqs, env, store=store, store_not=store_not, it=R.both(has=has, lacks=lacks, fallback=fallback))
    cs = R.Case("long", [r])
    g = MpcGpu(0, lib_path)
    try:
        g.set_hmm(*G.hmm_tables())
        g.timers_enable(True)
        return R.run_store(g, cs, 0, r, marks=False)
    finally:
        g.close()


def check_join(seqs, env, lib_path=None):
    """mpcgpu_build_post / mpcgpu_align_alns(_w) on a fixed bipartition (odd against even sequences: both stored orientations) after
    two iterations on a store built under env: the row form of BuildPost reads the block records (launch counters 1/0/0), matrix,
    path and score equal the restatement + the oracle's CalcAlnFlat"""
    def body():
        ctx = J.Ctx(list(seqs), lib_path)
        try:
            info, fb = ctx.g.relax_info()
            j = ctx.join(list(range(1, len(seqs), 2)), list(range(0, len(seqs), 2)), np.random.default_rng(5))
            ctx.check(j, "row", what="join over the long form")
            return info, fb
        finally:
            ctx.close()
    return J.with_env(dict(env), body)
