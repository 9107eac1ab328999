#!/usr/bin/env python3
"""Sampled parity check of a run too large for a reference digest (3000 x L~400: a full ConsIter of the reference takes days, and so does
stage A of 4.5 * 10^6 pairs on a CPU). One process, one store, the library's own two relax iterations; checked against the CPU oracle
(oracle/mpc_oracle.c through tests/_oracle.py) for a seeded CLIQUE of c sequences, i.e. c (c - 1) / 2 pairs:

  EA, stage 0   the oracle's own stage A of every clique pair (forward/backward, posterior, sparsify, EA) == the library's, bit for bit
  stage 1, 2    the oracle's ConsPair of every clique pair over what that pair READS — the matrices (X, Z) and (Y, Z) of all Z as the
                library held them before the iteration (downloaded: c (n - 1) matrices per stage) — == the library's matrix after the
                iteration's commit, bit for bit. By induction from stage 0 the clique's stage 2 is the oracle's, provided the foreign
                operands are right, which the same check says of every one of them that lies in the clique.

Every pair reads records of every Z, so on a store in segments (mpcgpu_relax_info names them) every checked cell has walked all segments.
Prints one JSON line; exit status 1 on a mismatch.

  python scripts/sample_parity.py --n 3000 --len 400 --seed 1 [--clique 6 --sample-seed 7] [--lib PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3000)
    ap.add_argument("--len", type=int, default=400)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--clique", type=int, default=6)
    ap.add_argument("--sample-seed", type=int, default=7)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    import _golden as G
    import _oracle as O
    from muscle_amd._lib import MpcGpu
    from muscle_amd.synth import make_family
    n = a.n
    seqs = make_family(n, a.len, seed=a.seed)
    lens = [len(s) for s in seqs]
    s, t, m, i, thr = G.hmm_tables()
    hmm = O.make_hmm(s, t, m, i)
    pidx = lambda x, y: x * n - (x * (x + 1)) // 2 + (y - x - 1)  # InitPairs order, x < y
    clique = sorted(int(x) for x in np.random.default_rng(a.sample_seed).choice(n, a.clique, replace=False))
    cpairs = [(x, y) for q, x in enumerate(clique) for y in clique[q + 1:]]
    t0 = time.time()
    g = MpcGpu(0, a.lib)
    g.set_hmm(s, t, m, i, thr)
    g.set_seqs(seqs)
    g.calc_posteriors()
    ea = g.get_ea().copy()
    g.build_store()

    def snapshot():
        """pair number -> (offsets, values) of every pair that holds a clique sequence"""
        out = {}
        for x in clique:
            if x + 1 < n:  # the pairs (x, Z > x) are consecutive
                k0 = pidx(x, x + 1)
                for q, mx in enumerate(g.get_sparse_range(k0, k0 + n - 1 - x)):
                    out[k0 + q] = mx
            for z in range(x):
                k = pidx(z, x)
                if k not in out:
                    out[k], = g.get_sparse_range(k, k + 1)
        return out

    def oracle_store(mats):
        st = O.Store(seqs)
        for k, (off, val) in mats.items():
            st.set(k, off, val)
        return st

    def oracle_get(st, k, LX):
        nnz = O.lib().orc_store_nnz(st.h, k)
        off = np.empty(LX + 1, np.uint32)
        val = np.empty(max(nnz, 1) * 2, np.uint32)
        O.lib().orc_store_get(st.h, k, off.ctypes.data, val.ctypes.data)
        return off, val[:2 * nnz]

    say = lambda what: print("[sample_parity] %.0f s: %s" % (time.time() - t0, what), file=sys.stderr, flush=True)
    say("store built")
    bad = []
    cur = snapshot()
    say("stage 0 operands downloaded")
    # EA and stage 0: the oracle's stage A of the clique pairs
    st0 = O.Store(seqs)
    oea = np.zeros(st0.npairs, np.float32)
    for x, y in cpairs:
        k = pidx(x, y)
        O.lib().orc_calc_posteriors(C.byref(hmm), st0.h, st0._ptrs, oea.ctypes.data, k, k + 1, 1)
        off, val = oracle_get(st0, k, lens[x])
        if oea[k:k + 1].view(np.uint32)[0] != ea[k:k + 1].view(np.uint32)[0]:
            bad.append("EA of pair (%d,%d)" % (x, y))
        if not (np.array_equal(off, cur[k][0]) and np.array_equal(val, cur[k][1])):
            bad.append("stage 0 of pair (%d,%d)" % (x, y))
    del st0
    entries = 0
    for it in (1, 2):
        src = oracle_store(cur)
        g.cons_iter()
        g.cons_commit()
        info, fallback = g.relax_info()
        say("iteration %d committed" % it)
        nxt = snapshot() if it == 1 else {pidx(x, y): g.get_sparse_range(pidx(x, y), pidx(x, y) + 1)[0] for x, y in cpairs}
        for x, y in cpairs:
            k = pidx(x, y)
            dst = src.cons_iter(k, k + 1, threads=1)
            off, val = oracle_get(dst, k, lens[x])
            entries += len(val) // 2
            if not (np.array_equal(off, nxt[k][0]) and np.array_equal(val, nxt[k][1])):
                bad.append("stage %d of pair (%d,%d)" % (it, x, y))
            if np.array_equal(val, cur[k][1]):
                bad.append("stage %d of pair (%d,%d) equals stage %d: nothing was relaxed" % (it, x, y, it - 1))
            del dst
        del src
        cur = nxt
    si = g.store_info()
    g.close()
    out = {"check": "sampled parity against the CPU oracle: EA + stage 0 by the oracle's stage A, stages 1 and 2 by the oracle's ConsPair over the "
                    "operands the library held (scripts/sample_parity.py)",
           "n_seqs": n, "mean_len": float(np.mean(lens)), "seed": a.seed, "clique": clique, "pairs_checked": len(cpairs),
           "operand_matrices_per_stage": a.clique * (n - 1) - len(cpairs), "entries_checked_stages_1_2": entries,
           "record_bytes": si["record_bytes"], "window_bytes": si["window_bytes"], "stored_posteriors": si["entries"],
           "relax_geometry": {"layout": info, "fallback": bool(fallback)},
           "result": "match" if not bad else "MISMATCH", "mismatches": bad[:20], "seconds": round(time.time() - t0, 1)}
    print(json.dumps(out), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
