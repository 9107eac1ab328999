"""Path-pinned checks of the device joins (mpcgpu_build_post, mpcgpu_align_alns(_w), mpcgpu_align_alns_batch, mpcgpu_align_msas)
against the numpy restatement (_buildpost.py) and the oracle's CalcAlnFlat, bit for bit. Shared by tests/test_gpu_joins.py
(production shapes) and tests/test_emu_parity.py (the same path table, small).

Every case states the device path the dispatcher (muscle_amd/csrc/mpcgpu_joins.inc) must take and proves it, so that a case
which drifts off its path fails instead of quietly testing another one:
  * BuildPost: the launch counters of timers_get() (buildpost_gen counts the row kernel and the generating kernel of the general
    path; buildpost_sort and buildpost_reduce count the general path's sort and reduction): row form 1/0/0, general path 1/1/1,
    row form that overflowed its list and was redone by the general path 2/1/1.
  * The alignment kernel: the MPCGPU_TRACE=1 line "calc_aln C1 x C2: one wave | waves, rows in registers | rows in LDS" (the
    library reads MPCGPU_TRACE once per process, so those cases run in a child process: `python _joins.py aln LIB SIZE`).

Where each path is reached (gpu: tests/test_gpu_joins.py, emu: tests/test_emu_parity.py) and what proves it:
  row form, 8 columns per lane       test_join_paths[row8*], test_emu_joins_row_form[row8*]          gen/sort/reduce 1/0/0
  row form, 16 columns per lane      test_join_paths[row16*], test_emu_joins_row_form[row16*]        1/0/0 at C2 = 513, 1024
  row form overflow, general redo    test_row_list_overflow, test_emu_joins_row_list_overflow       2/1/1 + "row kernel" (traced)
  general path                       test_join_paths[general*], [*-sort], test_long_runs_at_scale,   1/1/1
                                     test_emu_joins_general_*, test_emu_align_alns_long_runs
  batch forms, chunks, fallbacks     test_align_alns_batch_level_scale, test_emu_joins_batch_paths   launch counts of the plan
  one wave / waves / rows in LDS     test_alignment_kernels_traced, test_emu_joins_alignment_kernels_traced   "calc_aln" trace line
  align_msas list form               test_align_msas_long_lists, test_emu_align_msas_long_list      matrix, path, score, EA bits
TEST INFRASTRUCTURE."""
import os
import subprocess
import sys

import numpy as np

import _buildpost as BP
import _golden as G
import _oracle as O
from muscle_amd._lib import MpcGpu
from muscle_amd.synth import make_family

# the dispatcher's limits (mpcgpu_joins.inc: rows_form_fits with MPC_ROWS_PAIRS_MAX, MPC_ROWS_CELLS1_MAX (build_post_impl) and
# MPC_ROWS_CELLS1_MAX_BATCH (mpcgpu_align_alns_batch), aln_wave_fits with MPC_LDS_MAX, the 1 GiB of cut_join_chunk; kernels_prog.h: MPC_BPR_CAP;
# kernels_aln.h: MPC_ALNW_MAXW, MPC_ALNW_ROWBYTES)
ROW_PAIRS, ROW_C2, ROW_CELLS1, BATCH_CELLS1 = 2048, 1024, 1 << 26, 1 << 22
BPR_CAP, ALNW_MAXW, ALNW_ROWBYTES, LDS_BYTES = 1024, 512, 256, 160 * 1024
BATCH_BYTES = 1 << 30
WAVE, QUAD, LDSROWS = "one wave", "waves, rows in registers", "rows in LDS"
# launch counts (buildpost_gen, buildpost_sort, buildpost_reduce) of one BuildPost on each path
BP_COUNTS = {"row": (1, 0, 0), "general": (1, 1, 1), "overflow": (2, 1, 1)}


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def aln_class(C1, C2):
    """run_calc_aln's choice by size (MPCGPU_ALN_KERNEL unset)"""
    W = C2 + 1
    if W <= ALNW_MAXW and (C1 + 1) * ALNW_ROWBYTES + 16 <= LDS_BYTES:
        return WAVE
    if (W + 255) // 256 * 64 <= 1024:
        return QUAD
    return LDSROWS


def msa_of_width(seqs, idxs, rng, width):
    """a random gapped alignment of the given sequences with exactly `width` columns: rows as strings"""
    rows = []
    for i in idxs:
        s = seqs[i]
        cols = np.sort(rng.choice(width, size=len(s), replace=False))
        row = ["-"] * width
        for ch, c in zip(s, cols):
            row[c] = ch
        rows.append("".join(row))
    return rows


class Join:
    def __init__(self, seqs, grp1, grp2, rng, C1=None, C2=None, extra1=0, extra2=0):
        self.grp1, self.grp2 = list(grp1), list(grp2)
        if C1 is None:
            rows1, C1 = BP.random_msa(seqs, self.grp1, rng, extra=extra1)
        else:
            rows1 = msa_of_width(seqs, self.grp1, rng, C1)
        if C2 is None:
            rows2, C2 = BP.random_msa(seqs, self.grp2, rng, extra=extra2)
        else:
            rows2 = msa_of_width(seqs, self.grp2, rng, C2)
        self.C1, self.C2 = C1, C2
        self.m1 = [BP.pos_to_col(r) for r in rows1]
        self.m2 = [BP.pos_to_col(r) for r in rows2]
        self.w1 = rng.uniform(0.2, 1.8, len(grp1)).astype(np.float32)
        self.w2 = rng.uniform(0.2, 1.8, len(grp2)).astype(np.float32)

    def args(self):
        return self.grp1, self.grp2, self.m1, self.m2, self.C1, self.C2

    def both_orientations(self):
        return any(S < T for S in self.grp1 for T in self.grp2) and any(S > T for S in self.grp1 for T in self.grp2)


class Ctx:
    """a context after calc_posteriors, build_store and `iters` cons_iter / cons_commit rounds, with its store read back"""

    def __init__(self, seqs, lib_path=None, iters=2):
        s, t, m, i, thr = G.hmm_tables()
        self.seqs = seqs
        self.g = g = MpcGpu(0, lib_path)
        g.set_hmm(s, t, m, i, thr)
        g.set_seqs(seqs)
        g.calc_posteriors()
        g.build_store()
        for _ in range(iters):
            g.cons_iter()
            g.cons_commit()
        g.timers_enable(True)
        self.stage = g.get_sparse_range()
        n = len(seqs)
        self.pidx = {p: k for k, p in enumerate((a, b) for a in range(n) for b in range(a + 1, n))}

    def close(self):
        self.g.close()

    def join(self, grp1, grp2, rng, **kw):
        return Join(self.seqs, grp1, grp2, rng, **kw)

    def predict(self, j, mode=None):
        """the BuildPost path build_post_impl takes for this join under MPCGPU_BP=mode"""
        n1, n2 = len(j.grp1), len(j.grp2)
        if mode == "sort" or not (n1 * n2 <= ROW_PAIRS and j.C2 <= ROW_C2 and n1 * j.C1 <= ROW_CELLS1):
            return "general"
        if BP.row_chunk_max(self.stage, self.pidx, j.grp1, j.grp2, j.m1, j.C1) > BPR_CAP:
            return "overflow"
        return "row"

    def want(self, j, weighted):
        w = (j.w1, j.w2) if weighted else (None, None)
        return BP.build_post_fast(self.stage, self.pidx, *j.args(), *w)

    def counts(self):
        t = self.g.timers_get()
        return tuple(t[k][1] for k in ("buildpost_gen", "buildpost_sort", "buildpost_reduce", "calc_aln"))

    def check(self, j, path, mode=None, what=""):
        """build_post and align_alns(_w), unweighted and weighted, under MPCGPU_BP=mode: the matrix (also get_last_post after the
        alignment), path and score bits against the restatement + the oracle's CalcAlnFlat, and the launch counts of `path`"""
        assert j.both_orientations() or min(len(j.grp1), len(j.grp2)) == 1 and len(j.grp1) + len(j.grp2) == 2, (what, "orientations")
        got_path = self.predict(j, mode)
        assert got_path == path, (what, "the case does not reach its path", path, got_path)
        gen, srt, red = BP_COUNTS[path]
        g = self.g
        out = []
        for weighted in (False, True):
            w = (j.w1, j.w2) if weighted else (None, None)
            want = self.want(j, weighted)
            tag = (what, path, mode, "weighted" if weighted else "plain")

            def run():
                g.timers_reset()
                post = g.build_post(*j.args(), *w)
                c_bp = self.counts()
                g.timers_reset()
                aln = g.align_alns(*j.args(), *w)
                c_aa = self.counts()
                return post, c_bp, aln, c_aa, g.last_post(j.C1, j.C2)
            post, c_bp, (p1, s1), c_aa, last = with_env({"MPCGPU_BP": mode}, run)
            assert c_bp == (gen, srt, red, 0), (tag, "build_post launches", c_bp)
            # an overflowed row form aligns the matrix it made before the redo: two alignments
            assert c_aa == (gen, srt, red, 2 if path == "overflow" else 1), (tag, "align_alns launches", c_aa)
            assert np.array_equal(bits(post), bits(want)), (tag, "build_post matrix")
            assert np.array_equal(bits(last), bits(want)), (tag, "get_last_post after align_alns")
            sc0, p0 = O.calc_aln(want)
            assert p1 == p0 and bits(s1) == bits(sc0), (tag, "path / score")
            out.append((p1, s1))
        return out

    def check_batch(self, joins, what=""):
        """align_alns_batch == align_alns join by join and the restatement, results in list order, and the launch counts that
        the batch's plan (small joins in chunks of at most 1 GiB of matrices; the others and the joins of an overflowed chunk one
        at a time) implies"""
        g = self.g
        nj = len(joins)
        small = []
        for q, j in enumerate(joins):
            n1, n2 = len(j.grp1), len(j.grp2)
            rows_ok = n1 * n2 <= ROW_PAIRS and j.C2 <= ROW_C2 and n1 * j.C1 <= BATCH_CELLS1
            wave_ok = j.C2 + 1 <= ALNW_MAXW and (j.C1 + 1) * ALNW_ROWBYTES + 16 <= LDS_BYTES
            if rows_ok and wave_ok and nj > 1:
                small.append(q)
        chunks, cur, cells = [], [], 0
        for q in small:
            cq = joins[q].C1 * joins[q].C2
            if cur and (cells + cq) * 4 > BATCH_BYTES:
                chunks.append(cur)
                cur, cells = [], 0
            cur.append(q)
            cells += cq
        if cur:
            chunks.append(cur)
        paths = {q: self.predict(j) for q, j in enumerate(joins)}
        single = [q for q in range(nj) if q not in small]
        for ch in chunks:
            if any(paths[q] == "overflow" for q in ch):
                single += ch
        gen = srt = red = 0
        aln = len(chunks)
        gen += len(chunks)
        for q in single:
            a, b, c = BP_COUNTS[paths[q]]
            gen, srt, red = gen + a, srt + b, red + c
            aln += 2 if paths[q] == "overflow" else 1
        g.timers_reset()
        got = g.align_alns_batch([j.args() for j in joins])
        cnt = self.counts()
        assert cnt == (gen, srt, red, aln), (what, "align_alns_batch launches", cnt, (gen, srt, red, aln), len(chunks), len(single))
        for q, j in enumerate(joins):
            sc0, p0 = O.calc_aln(self.want(j, False))
            p1, s1 = got[q]
            assert p1 == p0 and bits(s1) == bits(sc0), (what, "batch join", q, "vs restatement")
            p2, s2 = g.align_alns(*j.args())
            assert p1 == p2 and bits(s1) == bits(s2), (what, "batch join", q, "vs align_alns")
        return chunks, single


# Identical low-complexity sequences of two lengths: a position of a 60-residue poly-A has ~27 stored entries against a 100-residue
# one, so a chunk of 64 such pairs lists more than MPC_BPR_CAP entries for one output row and the row form overflows.
HOMOPOLYMERS = ["A" * 60, "A" * 100] * 8


def overflow_groups(h0):
    """MSA1 = the eight short poly-A (at h0 + even offsets), MSA2 = the eight long ones: 64 pairs, both stored orientations"""
    return [h0 + 2 * k for k in range(8)], [h0 + 2 * k + 1 for k in range(8)]


# ---- align_msas: CalcPosteriorFlat3 over an explicit pair list ------------------------------------------------------------
def check_align_msas(seqs, grp1, grp2, pairs, rng, lib_path=None, extra=0, what=""):
    """mpcgpu_align_msas on pairs [(row of MSA1, row of MSA2)] (repeats allowed) against the oracle per pair (stage A, EA) and
    the list-form restatement (matrix after the call, path, score). Returns (C1, C2, npairs)."""
    s, t, m, i, thr = G.hmm_tables()
    h = O.make_hmm(s, t, m, i)
    rows1, C1 = BP.random_msa(seqs, grp1, rng, extra=extra)
    rows2, C2 = BP.random_msa(seqs, grp2, rng, extra=extra)
    seq1 = [grp1[a] for a, b in pairs]
    seq2 = [grp2[b] for a, b in pairs]
    m1 = [BP.pos_to_col(rows1[a]) for a, b in pairs]
    m2 = [BP.pos_to_col(rows2[b]) for a, b in pairs]
    memo = {}
    sparse, ea_want = [], []
    for X, Y in zip(seq1, seq2):
        if (X, Y) not in memo:
            x, y = seqs[X].encode(), seqs[Y].encode()
            Pd = O.post(O.fwd(h, x, y), O.bwd(h, x, y), len(x), len(y))
            memo[(X, Y)] = (O.sparse_from_post(Pd), np.float32(O.aln_score(Pd)) / np.float32(min(len(x), len(y))))
        sp, e = memo[(X, Y)]
        sparse.append(sp)
        ea_want.append(e)
    want = BP.build_post_list_fast(sparse, m1, m2, C1, C2)
    sc0, p0 = O.calc_aln(want)
    g = MpcGpu(0, lib_path)
    try:
        g.set_hmm(s, t, m, i, thr)
        g.set_seqs_registry(seqs)
        path, sc, ea = g.align_msas(seq1, seq2, m1, m2, C1, C2)
        assert np.array_equal(bits(ea), bits(np.array(ea_want, np.float32))), (what, "per-pair EA")
        assert np.array_equal(bits(g.last_post(C1, C2)), bits(want)), (what, "matrix")
        assert path == p0 and bits(sc) == bits(sc0), (what, "path / score")
    finally:
        g.close()
    return C1, C2, len(pairs)


# ---- the alignment kernels after BuildPost, in a child process with MPCGPU_TRACE=1 ----------------------------------------
def aln_cases(size):
    """[(sequences, [(name, grp1, grp2, Join kwargs, BuildPost path, alignment class)])], one context per entry: joins ending in
    each alignment kernel, and a row form that overflows its list. emu: short sequences, the class above 4096 columns reached by
    gap columns; gpu: a pair of sequences longer than 4096 residues, in a context of its own (sequences that long leave the store
    without the variable-size records, so no join of that context can take the row form)."""
    short = [("one wave", [0, 3, 5], [1, 2, 6], {}, "row", WAVE),
             ("waves: C2 > 511", [1, 4], [0, 7, 2], {"C2": 700}, "row", QUAD),
             ("waves: C1 > 638", [6, 2], [3, 5], {"C1": 700}, "row", QUAD),
             ("row list overflow", *overflow_groups(8), {}, "overflow", WAVE)]
    if size == "gpu":
        return [(make_family(8, 120, seed=5) + HOMOPOLYMERS, short),
                (make_family(2, 4200, seed=6), [("rows in LDS", [1], [0], {}, "general", LDSROWS)])]
    return [(make_family(8, 30, seed=5) + HOMOPOLYMERS, short + [("rows in LDS", [4, 0], [2, 7], {"C2": 4100}, "general", LDSROWS)])]


def run_aln_cases(lib_path, size):
    rng = np.random.default_rng(17)
    for seqs, cases in aln_cases(size):
        ctx = Ctx(seqs, lib_path)
        try:
            for name, grp1, grp2, kw, path, cls in cases:
                j = ctx.join(grp1, grp2, rng, **kw)
                assert aln_class(j.C1, j.C2) == cls, (name, j.C1, j.C2)
                print("CASE %s|%d|%d|%s|%s" % (name, j.C1, j.C2, path, cls), flush=True)
                sys.stderr.flush()
                ctx.check(j, path, what=name)
                sys.stdout.flush()
        finally:
            ctx.close()
    print("OK aln", flush=True)


def check_aln_cases_traced(lib_path, size, timeout=600):
    """run_aln_cases in a child process with MPCGPU_TRACE=1; every case's alignments must be traced with its class and the
    overflow case's calls must show the row kernel"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MPCGPU_TRACE="1", PYTHONPATH=os.path.dirname(here) + os.pathsep + here)
    r = subprocess.run([sys.executable, "-u", os.path.join(here, "_joins.py"), "aln", lib_path or "", size], env=env, cwd=here,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout, text=True)
    out = r.stdout
    assert r.returncode == 0 and "OK aln" in out, "exit %d\n%s" % (r.returncode, out[-4000:])
    # the output of each case runs from its CASE line to the next one
    parts = out.split("CASE ")[1:]
    assert len(parts) == sum(len(cases) for _, cases in aln_cases(size))
    for part in parts:
        head, body = part.split("\n", 1)
        name, C1, C2, path, cls = head.split("|")
        aln_lines = [ln for ln in body.splitlines() if "calc_aln " in ln and ln.startswith("[mpcgpu]")]
        # plain + weighted: two align_alns calls, one alignment each (two for the overflowed row form)
        assert len(aln_lines) == (4 if path == "overflow" else 2), (name, aln_lines)
        for ln in aln_lines:
            assert ln.endswith("calc_aln %s x %s: %s" % (C1, C2, cls)), (name, ln)
        rowk = [ln for ln in body.splitlines() if "build_post" in ln and ": row kernel" in ln]
        assert len(rowk) == (4 if path in ("row", "overflow") else 0), (name, rowk)  # build_post + align_alns, plain + weighted
    return out


if __name__ == "__main__":
    if sys.argv[1] == "aln":
        run_aln_cases(sys.argv[2] or None, sys.argv[3])
