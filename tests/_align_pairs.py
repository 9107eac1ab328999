"""Path-pinned checks of the device AlignPairFlat (mpcgpu_align_pairs) and its FromPost matrices (mpcgpu_get_list_sparse) against
the oracle, bit for bit. Shared by tests/test_gpu_align_pairs.py (production shapes) and tests/test_emu_parity.py (the same table,
thin shapes and lowered limits).

ap_oracle composes the oracle's pieces in AlignPairFlat's order (fwd / bwd or their Mega forms, the dense thresholded CalcPostFlat,
CalcAlnFlat, EA = Score / min(LX, LY), FromPost); tests/test_align_pairs_table.py pins that composition to the compiled reference's
ap_ragged.npz. Every call of a case compares, for every pair, the path string, score bits and EA bits of align_pairs and the offsets
and values of get_list_sparse with ap_oracle (0 ulp).

Every call states the path the dispatcher (muscle_amd/csrc/mpcgpu_joins.inc: mpcgpu_align_pairs, align_pairs_small) must take, and
predict() restates the dispatcher's limits to put it there. A call that drifts off its path fails:
  short list (<= 64 pairs, one wait)     launch counters fb / post / calc_aln = bins / 1 / 1; stage_a_info()[0] = 0 on a fresh context;
                                         traced: one "align_pairs short list: fb H=" line per bin, no stage-A "fb" line
  short list overflowed, general redo    counters: post = 1 + (1 + regrowths) + 1 (the short post, the general post per attempt, the
                                         pack); stage_a_info()[0] = pairs; traced: the short lines and then stage-A "fb" lines
  general path                           counters: post = 2 + regrowths per chunk, calc_aln = 1 per all-one-wave chunk else 1 per pair,
                                         stage_a_info()[0] = pairs of the last chunk; traced: the "fb H=" / "fb chains H=" bins equal
                                         the bins of the pairs under long_min, "fb row blocks: H=" names the row-block instantiation,
                                         the "calc_aln LX x LY: <kernel>" lines list exactly the pairs of chunks that are not all one-wave
  fb_chain_kernel chains on a list       stage_a_info()[1:] = (chained pairs, chains) > 0 with MPCGPU_FB_CHAIN_GRADE=0, (0, 0) under
                                         MPCGPU_FB_CHAIN=0 or Mega
  refusal (MPCGPU_POST=sort)             MpcGpuError naming mpcgpu_align_pairs; the next call on the context matches the oracle

Where each path of the issue is reached (gpu: test_gpu_align_pairs.py::test_align_pairs_case[NAME], emu:
test_emu_parity.py::test_emu_align_pairs_case[NAME]):
  short list, bins H = 1..10                 short_bins (both sizes)
  exits: LY 511 / 512, LX 638 / 639,          exit_ly, exit_lx, exit_pairs, exit_long_min; emu also exit_long_min_knob
    64 / 65 pairs, LX 768 / 769                 (MPCGPU_FB_LONG_MIN + MPCGPU_FB_LONG_H=1)
  MPCGPU_PAIRS_SMALL=0, MPCGPU_FB_CHAIN=0     short_bins (calls 2 and 3), degenerate
  candidate overflow after the short path    overflow_short ("A"*638 x "A"*511 on the gpu, "A"*200 x "A"*150 on the emu)
  general-stage regrowth alone               overflow_general (MPCGPU_CAND_PER_ROW=1)
  fb_chain_kernel on lists                   short_bins, chains
  row blocks H = 7 / 4 / 1                   row_blocks (default, MPCGPU_FB_LONG_H=4, =1)
  dense_post_kernel with 16-bit keys         row_blocks, exit_long_min, mega, sequence
  per-pair calc_aln kernel choice            exit_*, row_blocks ("rows in LDS": more than 4096 columns), chunks
  more than one 256-pair chunk               chunks
  chunk halving (stage A split a chunk)      halving (MPCGPU_SCRATCH_GB=0)
  get_list_sparse: after the short path,     every short call (in list order), short_bins (a middle pair first), chunks (last
    earlier chunk, single-pair fallback        window, earlier chunk, then back), halving (the single-pair fallback)
  refusal without the row-list kernel        refusal
  Mega, and letters after it                 mega, sequence
  one context reused across calls            sequence, mega, every multi-call case
  degenerate pairs                           degenerate (identical, length 1, "ACDEFGHIKLMNPQRSTVWY" * k)
TEST INFRASTRUCTURE."""
import hashlib
import os
import subprocess
import sys

import numpy as np

import _golden as G
import _oracle as O
import _parity as P
from muscle_amd._lib import MpcGpu, MpcGpuError
from muscle_amd.synth import make_family

# ---- the dispatcher's limits ------------------------------------------------------------------------------------------------
PAIRS_SMALL_MAX = 64            # mpcgpu_joins.inc: mpcgpu_align_pairs  npairs <= 64 && MPCGPU_PAIRS_SMALL -> align_pairs_small
LONG_MIN = 64 * 12 + 1          # mpcgpu_stage_a.inc: stage_a_geom()  MPCGPU_FB_LONG_MIN, clamped to [2, 64 * HMAX + 1]
HMAX = 16                       # kernels_fb.h:47  MPC_HMAX
ALNW_MAXW = 512                 # kernels_aln.h:107  MPC_ALNW_MAXW: LY + 1 <= 512 for the one-wave alignment (mpcgpu_joins.inc: aln_wave_fits)
ALNW_ROWBYTES = 256             # kernels_aln.h:108  MPC_ALNW_ROWBYTES: (LX + 1) * 256 + 16 <= 160 KB (mpcgpu_joins.inc: aln_wave_fits, MPC_LDS_MAX)
LDS_BYTES = 160 * 1024
POST_ROWS_LDS = 150 * 1024      # mpcgpu_stage_a.inc: post_rows_fits()  the row-list finishing kernel's LDS arrays
POST_SORT_CAP = 1024            # mpcgpu_stage_a.inc: stage_a()  MPCGPU_POST_SORT_CAP default
CAND_PER_ROW = 12               # mpcgpu_stage_a.inc: stage_a_geom()  MPCGPU_CAND_PER_ROW
CAND_FLOOR = 1024               # mpcgpu_stage_a.inc: stage_a_geom()
CHUNK = 256                     # mpcgpu_joins.inc: mpcgpu_align_pairs  pairs per stage-A call of the general path
QUAD_MAXW = 4096                # mpcgpu_joins.inc: run_calc_aln  (W + 255) / 256 * 64 <= 1024 threads
LONG_H = 7                      # mpcgpu.cpp:381  MPC_LONG_H (MPCGPU_FB_LONG_H = 4: MPC_LONG_H_SMALL, 1: one row per lane)
WAVE, QUAD, LDSROWS = "one wave", "waves, rows in registers", "rows in LDS"
SHORT_FB = "[mpcgpu] align_pairs short list: fb H="

_HMM = None


def hmm():
    global _HMM
    if _HMM is None:
        s, t, m, i, thr = G.hmm_tables()
        _HMM = (O.make_hmm(s, t, m, i), (s, t, m, i, thr))
    return _HMM


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def env_int(env, name, default):
    v = env.get(name)
    return default if v is None or v == "" else int(v)


def long_min_of(env):
    return min(max(env_int(env, "MPCGPU_FB_LONG_MIN", LONG_MIN), 2), 64 * HMAX + 1)


def one_wave(LX, LY):
    return LY + 1 <= ALNW_MAXW and (LX + 1) * ALNW_ROWBYTES + 16 <= LDS_BYTES


def aln_class(LX, LY):
    """run_calc_aln's choice by size (mpcgpu_joins.inc: aln_wave_fits, run_calc_aln)"""
    if one_wave(LX, LY):
        return WAVE
    if (LY + 1 + 255) // 256 * 64 <= 1024:
        return QUAD
    return LDSROWS


def capc_of(lens, env):
    """the first candidate room per pair of a list, short path and stage A alike: max(k * longest sequence, 1024)"""
    Lmax = max(max(a, b) for a, b in lens)
    return max(max(env_int(env, "MPCGPU_CAND_PER_ROW", CAND_PER_ROW), 1) * Lmax, CAND_FLOOR)


def regrowths(lens, cand, env):
    """stage A's overflow retries on one batch (mpcgpu_stage_a.inc: stage_a()): the room doubles, up to LXmax * LYmax"""
    capc, n = capc_of(lens, env), 0
    full = max(a for a, _ in lens) * max(b for _, b in lens)
    while max(cand) > capc:
        capc = min(2 * capc, full)
        n += 1
    return n


def regrowths_each(lens, cand, env):
    """the overflow retries of a list that runs a pair per batch (MPCGPU_SCRATCH_GB=0; mpcgpu_ea.inc: ea_sublist()): only the batches
    that hold an overflowing list are redone, and the room grows for the rest of the list once a batch was redone"""
    capc, n = capc_of(lens, env), 0
    full = max(a for a, _ in lens) * max(b for _, b in lens)
    for k in cand:
        while k > capc:
            capc, n = min(2 * capc, full), n + 1
    return n


def predict(lens, env, cand=None):
    """the path of mpcgpu_align_pairs for pairs of these (LX, LY) under env: "short", "overflow" (short list whose candidate list
    overflowed: the general path redoes it; needs the oracle's candidate counts) or "general" (mpcgpu_joins.inc: align_pairs_small, mpcgpu_align_pairs)"""
    n = len(lens)
    if not (1 <= n <= PAIRS_SMALL_MAX and env_int(env, "MPCGPU_PAIRS_SMALL", 1) != 0):
        return "general"
    lm = long_min_of(env)
    if any(LX >= lm or not one_wave(LX, LY) for LX, LY in lens):
        return "general"
    LXm, LYm = max(a for a, _ in lens), max(b for _, b in lens)
    if (LXm + 2 + 2 * (LYm + 2)) * 4 + 8 + 8 * 1024 > POST_ROWS_LDS:
        return "general"
    if cand is not None and max(cand) > capc_of(lens, env):
        return "overflow"
    return "short"


def post_rows_ok(lens, env):
    """stage A takes the row-list finishing kernel (mpcgpu_stage_a.inc: post_rows_fits()), which the general path needs"""
    if env.get("MPCGPU_POST") == "sort":
        return False
    LXm, LYm = max(a for a, _ in lens), max(b for _, b in lens)
    return (LXm + 2 + 2 * (LYm + 2)) * 4 + 8 + 8 * max(env_int(env, "MPCGPU_POST_SORT_CAP", POST_SORT_CAP), 2) <= POST_ROWS_LDS


def chunks_of(n, env):
    """the general path's chunks [(q0, nq)]: 256 pairs; MPCGPU_SCRATCH_GB=0 gives stage A one pair per batch, so the first chunk
    halves down to one pair and every later chunk is one pair (mpcgpu_joins.inc: mpcgpu_align_pairs; mpcgpu_stage_a.inc: prepare_batch())"""
    size = 1 if env_int(env, "MPCGPU_SCRATCH_GB", 32) == 0 else CHUNK
    return [(q0, min(size, n - q0)) for q0 in range(0, n, size)]


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def ap_oracle(h, x, y, mega=None, path=True):
    """AlignPairFlat_SparsePost (alignpairflat.cpp:3-27) on the oracle: mega = (O.make_mega(...), profile of x, profile of y) or None
    -> dict(path, score, ea, off, val, cand: cells with Score >= MIN_SPARSE_SCORE, the candidate list the device keeps, rows: the
    cells of that list in each of the LX rows).
    path=False: the score alone (CalcAlnScoreFlat), as MPCFlat::CalcPosterior needs it (tests/_stage_a.py)"""
    if mega is None:
        F, B = O.fwd(h, x, y), O.bwd(h, x, y)
    else:
        g, px, py = mega
        F, B = O.fwd_mega(h, g, px, py), O.bwd_mega(h, g, px, py)
    LX, LY = len(x), len(y)
    Pd = O.post(F, B, LX, LY)
    del F, B
    sc, path = O.calc_aln(Pd) if path else (O.aln_score(Pd), None)
    off, val = O.sparse_from_post(Pd)
    return {"path": path, "score": np.float32(sc), "ea": np.float32(O.lib().orc_ea(sc, LX, LY)), "off": off, "val": val,
            "cand": int(np.count_nonzero(Pd)), "rows": np.count_nonzero(Pd, axis=1).astype(np.uint32)}


_MEMO = {}


def oracle_pair(seqs, x, y, mega=None):
    """ap_oracle of registry pair (x, y), remembered for the process (the tables reuse pairs across calls and environments)"""
    key = (seqs[x], seqs[y])
    if mega is not None:
        key += (mega["key"], hashlib.md5(mega["profs"][x].tobytes() + b"|" + mega["profs"][y].tobytes()).hexdigest())
    if key not in _MEMO:
        m = None if mega is None else (mega["g"], mega["profs"][x], mega["profs"][y])
        _MEMO[key] = ap_oracle(hmm()[0], seqs[x].encode(), seqs[y].encode(), m)
    return _MEMO[key]


# ---- the case table ---------------------------------------------------------------------------------------------------------
def related(lengths, seed):
    """sequences of exactly these lengths, cut from one family: related sequences, so the posteriors have real structure"""
    top = max(lengths)
    fam = make_family(len(lengths), top + top // 4 + 16, seed=seed)
    out = [s[:L] for s, L in zip(fam, lengths)]
    assert [len(s) for s in out] == list(lengths)
    return out


def with_mega(seqs, seed):
    m = P.random_mega(seqs, seed=seed)
    m["g"] = O.make_mega(m["alpha"], m["weight"], m["lp"], m["mx"])
    m["key"] = "random_mega %d" % seed
    return m


class Call:
    """one mpcgpu_align_pairs call: pairs of registry indices, the environment, the path it must take; sparse = None (every pair in
    list order), or the pairs to read first (then every pair in list order); chains = True (stage_a_info reports chains) / False /
    None; mega: the registry's profiles are active; refused: the call must fail"""

    def __init__(self, what, pairs, path, env=None, sparse=None, chains=None, mega=False, refused=False):
        self.what, self.pairs, self.path, self.env = what, list(pairs), path, dict(env or {})
        self.sparse, self.chains, self.mega, self.refused = sparse, chains, mega, refused


class Case:
    def __init__(self, name, seqs, calls, mega_seed=None, what=""):
        self.name, self.seqs, self.calls, self.what = name, seqs, calls, what
        self.mega = None if mega_seed is None else with_mega(seqs, mega_seed)

    def lens(self, call):
        return [(len(self.seqs[x]), len(self.seqs[y])) for x, y in call.pairs]

    def cells(self):
        """LX * LY over the distinct pairs the oracle computes for this case"""
        seen = set()
        for c in self.calls:
            for x, y in c.pairs:
                seen.add((x, y, c.mega))
        return sum(len(self.seqs[x]) * len(self.seqs[y]) for x, y, _ in seen)


def _grid(xl, yl, seed):
    """a registry of X sequences (lengths xl) and Y sequences (lengths yl), and every (X, Y) pair, X-major"""
    seqs = related(list(xl) + list(yl), seed)
    nx = len(xl)
    return seqs, [(a, nx + b) for a in range(nx) for b in range(len(yl))]


def cases(size):
    """the table: size "gpu" (production shapes) or "emu" (thin shapes: the same limits, a few residues on the other side)"""
    gpu = size == "gpu"
    out = []
    # short list, every rows-per-lane bin H = 1..10; runs with the same X, cut where LY + 1 < T = ceil(LX / H)
    xl = [1, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 512, 513, 576, 577, 638]
    yl = [1, 64, 511] if gpu else [1, 9, 64]
    seqs, pairs = _grid(xl, yl, 101)
    out.append(Case("short_bins", seqs, [
        Call("H = 1..10", pairs, "short", sparse=[len(pairs) // 2]),
        Call("MPCGPU_PAIRS_SMALL=0", pairs, "general", {"MPCGPU_PAIRS_SMALL": "0", "MPCGPU_FB_CHAIN_GRADE": "0"}, chains=True),
        Call("MPCGPU_PAIRS_SMALL=0 MPCGPU_FB_CHAIN=0", pairs, "general", {"MPCGPU_PAIRS_SMALL": "0", "MPCGPU_FB_CHAIN": "0"}, chains=False)]))
    # each exit from the short list, alone, beside the case just inside it; both orientations of the long pair
    t = 300 if gpu else 6
    seqs = related([t, 511, 512], 102)
    out.append(Case("exit_ly", seqs, [Call("LY 511", [(0, 1)], "short"), Call("LY 512", [(0, 2)], "general"),
                                      Call("511 x LY", [(1, 0)], "short"), Call("512 x LY", [(2, 0)], "short")]))
    seqs = related([638, 639, t if gpu else 5], 103)
    out.append(Case("exit_lx", seqs, [Call("LX 638", [(0, 2)], "short"), Call("LX 639", [(1, 2)], "general"),
                                      Call("Y 638", [(2, 0)], "general"), Call("Y 639", [(2, 1)], "general")]))
    seqs = related([90 if gpu else 14] * 12, 104)
    ordered = [(a, b) for a in range(12) for b in range(12) if a != b]
    out.append(Case("exit_pairs", seqs, [Call("64 pairs", ordered[:64], "short"), Call("65 pairs", ordered[:65], "general")]))
    seqs = related([768, 769, t], 105)
    out.append(Case("exit_long_min", seqs, [Call("LX 768", [(0, 2)], "general"), Call("LX 769", [(1, 2)], "general"),
                                            Call("Y 768", [(2, 0)], "general"),
                                            Call("Y 769", [(2, 1)], "general")]))
    # row blocks: LX 769, 1025, 2049 and a pair over 4096 columns ("rows in LDS"), both orientations, H = 7, 4, 1
    yl = [300, 4100] if gpu else [5, 4100]
    seqs = related([769, 1025, 2049, 800 if gpu else 4] + yl, 106)
    rb = [(0, 4), (4, 0), (1, 4), (4, 1), (2, 4), (4, 2), (3, 5), (5, 3)]
    out.append(Case("row_blocks", seqs, [Call("default", rb, "general"), Call("MPCGPU_FB_LONG_H=4", rb, "general", {"MPCGPU_FB_LONG_H": "4"}),
                                         Call("MPCGPU_FB_LONG_H=1", rb, "general", {"MPCGPU_FB_LONG_H": "1"})]))
    # the candidate list overflows: after the short path's kernels ran (then the general stage regrows), and in the general path alone
    a, b = (638, 511) if gpu else (200, 150)
    out.append(Case("overflow_short", ["A" * a, "A" * b], [Call("poly-A", [(0, 1)], "overflow"),
                                                           Call("poly-A, Y longer", [(1, 0)], "general" if gpu else "overflow")]))
    seqs = related([1100, 1040] if gpu else [700, 690], 107)
    env1 = {"MPCGPU_CAND_PER_ROW": "1"}
    out.append(Case("overflow_general", seqs, [Call("X longer", [(0, 1)], "general", env1), Call("Y longer", [(1, 0)], "general", env1)]))
    # chains on a list: one query x 8 hits (UClust::Search), runs cut by LY + 1 < T
    ql = [250, 200, 300, 180, 240, 64, 129, 230, 260, 210] if gpu else [40, 64, 65, 30, 129, 20, 50, 70, 33, 45]
    hl = [220, 30, 190, 260, 210, 20, 240, 200, 250, 180, 230, 15] if gpu else [40, 5, 36, 50, 44, 3, 60, 38, 55, 30, 42, 2]
    seqs = related(ql + hl, 108)
    rng = np.random.default_rng(8)
    pairs = [(q, len(ql) + int(h)) for q in range(len(ql)) for h in rng.permutation(len(hl))[:8]]
    out.append(Case("chains", seqs, [Call("80 pairs", pairs, "general", {"MPCGPU_FB_CHAIN_GRADE": "0"}, chains=True),
                                     Call("80 pairs, graded", pairs, "general")]))
    # chunks: 300 pairs, long and short mixed; get_list_sparse in the last window, an earlier chunk, then back
    sl = [60 if gpu else 10] * 16 + ([900, 600, 250] if gpu else [800, 600, 8])
    seqs = related(sl, 109)
    rng = np.random.default_rng(9)
    pairs = [tuple(int(v) for v in rng.choice(16, 2, replace=False)) for _ in range(300)]
    for q, p in ((7, (16, 18)), (100, (18, 17)), (260, (17, 18)), (299, (16, 0))):
        pairs[q] = p
    out.append(Case("chunks", seqs, [Call("300 pairs", pairs, "general", sparse=[299, 5, 262, 0])]))
    # chunk halving: no scratch budget, stage A one pair per batch; the single-pair fallback of get_list_sparse
    seqs = related([70 if gpu else 12] * 5 + [800 if gpu else 40], 110)
    pairs = [(a, b) for a in range(6) for b in range(6) if a != b][:20]
    out.append(Case("halving", seqs, [Call("20 pairs", pairs, "general", {"MPCGPU_SCRATCH_GB": "0", "MPCGPU_PAIRS_SMALL": "0"},
                                           sparse=[19, 3])]))
    # Mega: a short list, a general list with a row-block pair; then letters again on the same context
    seqs = related([150, 40, 300, 1, 90, 800 if gpu else 70, 200 if gpu else 30], 111)
    short = [(0, 1), (2, 0), (3, 4), (4, 2), (1, 1)]
    gen = [(5, 6), (6, 5), (0, 2), (5, 0)]
    genv = {} if gpu else {"MPCGPU_FB_LONG_MIN": "65", "MPCGPU_FB_LONG_H": "1"}
    out.append(Case("mega", seqs, [Call("Mega short", short, "short", mega=True), Call("Mega general", gen, "general", genv, mega=True),
                                   Call("letters short", short, "short"), Call("letters general", gen, "general", genv)], mega_seed=5))
    # one context in sequence: short H = 1, long general, short H = 10, Mega, letters
    seqs = related([40, 64, 1025 if gpu else 70, 300 if gpu else 30, 600, 400 if gpu else 12], 112)
    lenv = {} if gpu else {"MPCGPU_FB_LONG_MIN": "65", "MPCGPU_FB_LONG_H": "1"}
    out.append(Case("sequence", seqs, [Call("short H = 1", [(0, 1), (1, 0)], "short"), Call("long", [(2, 3), (3, 2), (0, 2)], "general", lenv),
                                       Call("short H = 10", [(4, 5), (4, 0)], "short"), Call("Mega", [(0, 1), (4, 5)], "short", mega=True),
                                       Call("letters", [(2, 3), (1, 4)], "general", lenv)], mega_seed=6))
    # refusal: the general path without the row-list finishing kernel; the short path does not read MPCGPU_POST
    seqs = related([120 if gpu else 20] * 4, 113)
    pairs = [(0, 1), (2, 3), (1, 2)]
    out.append(Case("refusal", seqs, [Call("MPCGPU_POST=sort, PAIRS_SMALL=0", pairs, "general", {"MPCGPU_POST": "sort", "MPCGPU_PAIRS_SMALL": "0"}, refused=True),
                                      Call("valid after", pairs, "general", {"MPCGPU_PAIRS_SMALL": "0"}),
                                      Call("MPCGPU_POST=sort, short list", pairs, "short", {"MPCGPU_POST": "sort"})]))
    # degenerate pairs
    k = [1, 5, 25] if gpu else [1, 3, 6]
    seqs = related([1, 1, 300 if gpu else 30], 114) + ["ACDEFGHIKLMNPQRSTVWY" * j for j in k]
    pairs = [(0, 0), (0, 1), (0, 2), (2, 0), (2, 2), (3, 3), (4, 5), (5, 4), (5, 5), (3, 5), (2, 5)]
    out.append(Case("degenerate", seqs, [Call("short", pairs, "short"), Call("general", pairs, "general", {"MPCGPU_PAIRS_SMALL": "0"})]))
    if not gpu:
        # the limits lowered by knobs (the GPU tables reach them at real sizes)
        seqs = related([64, 65, 130, 20], 115)
        knob = {"MPCGPU_FB_LONG_MIN": "65", "MPCGPU_FB_LONG_H": "1"}
        out.append(Case("exit_long_min_knob", seqs, [Call("LX 64", [(0, 3)], "short", knob), Call("LX 65", [(1, 3)], "general", knob),
                                                     Call("LX 130, both", [(2, 3), (3, 2), (2, 0)], "general", knob)]))
    return out


CASE_NAMES = [c.name for c in cases("emu")]
CASE_NAMES_GPU = [c.name for c in cases("gpu")]
MAX_GPU_CELLS = 60 * 10 ** 6  # the oracle's work over the GPU table


def case(size, name):
    return next(c for c in cases(size) if c.name == name)


# ---- running a case ---------------------------------------------------------------------------------------------------------
def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def list_sparse(g, q, LX):
    """mpcgpu_get_list_sparse of pair q of the last list -> (offsets, values)"""
    import ctypes as C
    nz = C.c_uint32()
    g._ck(g.L.mpcgpu_get_list_sparse(g.h, q, C.byref(nz), None, None))
    off = np.empty(LX + 1, np.uint32)
    val = np.empty(max(nz.value, 1) * 2, np.uint32)
    g._ck(g.L.mpcgpu_get_list_sparse(g.h, q, C.byref(nz), off.ctypes.data, val.ctypes.data))
    return off, val[:2 * nz.value].copy()


def expect(cs, call):
    """what a call must show: (path, {counter: launches or None}, fb bins of the short path)"""
    lens = cs.lens(call)
    wants = [oracle_pair(cs.seqs, x, y, cs.mega if call.mega else None) for x, y in call.pairs]
    path = predict(lens, call.env, [w["cand"] for w in wants])
    bins = sorted({(LX + 63) // 64 for LX, _ in lens})
    if path == "short":
        return path, {"fb": len(bins), "post": 1, "calc_aln": 1}, wants
    if path == "overflow":
        return path, {"post": 1 + (1 + regrowths(lens, [w["cand"] for w in wants], call.env)) + 1, "calc_aln": 2}, wants
    post = aln = 0
    for q0, nq in chunks_of(len(lens), call.env):
        sub = lens[q0:q0 + nq]
        aln += 1 if all(one_wave(*l) for l in sub) else nq
        post += 2 + regrowths(sub, [w["cand"] for w in wants[q0:q0 + nq]], call.env)
    if env_int(call.env, "MPCGPU_SCRATCH_GB", 32) == 0:
        post = None  # the halving stages of the first chunk run every pair of it again
    return path, {"post": post, "calc_aln": aln}, wants


def run_case(cs, lib_path=None, traced=False):
    """every call of the case on one context against the oracle and its path proofs; traced: print the markers the parent reads"""
    h, (s, t, m, i, thr) = hmm()
    g = MpcGpu(0, lib_path)
    try:
        g.set_hmm(s, t, m, i, thr)
        g.set_seqs_registry(cs.seqs)
        g.timers_enable(True)
        mega_on = False
        for k, call in enumerate(cs.calls):
            tag = (cs.name, k, call.what)
            if call.mega != mega_on:
                mg = cs.mega
                if call.mega:
                    g.set_mega(mg["alpha"], mg["weight"], mg["lp"], mg["mx"], mg["profs"])
                else:
                    g.set_mega(None, None, None, None, None)
                mega_on = call.mega
            assert predict(cs.lens(call), call.env) == ("short" if call.path == "overflow" else call.path), (tag, "predicted path")
            path, counts, wants = expect(cs, call)
            assert path == call.path, (tag, "the case does not reach its path", call.path, path)
            if call.refused:
                assert not post_rows_ok(cs.lens(call), call.env), tag
            xs, ys = [x for x, _ in call.pairs], [y for _, y in call.pairs]
            g.timers_reset()
            sa0 = g.stage_a_info()
            if traced:
                print("CALL %s|%d|%s" % (cs.name, k, call.path), flush=True)
                sys.stderr.flush()

            def run():
                try:
                    return g.align_pairs(xs, ys), None
                except MpcGpuError as e:
                    return None, str(e)
            res, err = with_env(call.env, run)
            sys.stderr.flush()
            if traced:
                print("END", flush=True)
            if call.refused:
                assert res is None and "mpcgpu_align_pairs" in err, (tag, "refusal", err)
                continue
            assert err is None, (tag, err)
            tm = g.timers_get()
            got = {key: tm[key][1] for key in ("fb", "post", "calc_aln")}
            for key, n in counts.items():
                assert n is None or got[key] == n, (tag, "launches of " + key, got, counts)
            if path == "overflow":
                assert got["fb"] > len({(LX + 63) // 64 for LX, _ in cs.lens(call)}), (tag, got)
            sa = g.stage_a_info()
            if path == "short":
                assert sa == sa0, (tag, "stage A ran on the short path", sa0, sa)
                if k == 0:
                    assert sa[0] == 0, (tag, sa)
            else:
                last = chunks_of(len(xs), call.env)[-1][1]
                assert sa[0] == last, (tag, "stage A pairs", sa, last)
                if call.chains is True:
                    assert sa[1] >= 2 and sa[2] >= 1, (tag, "no chains", sa)
                elif call.chains is False:
                    assert sa[1:] == (0, 0), (tag, "chains", sa)
            for q, ((p, sc, ea), w) in enumerate(zip(res, wants)):
                assert p == w["path"], (tag, q, call.pairs[q], "path")
                assert bits(sc) == bits(w["score"]) and bits(ea) == bits(w["ea"]), (tag, q, call.pairs[q], "score / EA", sc, w["score"], ea, w["ea"])
            order = list(call.sparse or []) + list(range(len(xs)))

            def sparse():
                for q in order:
                    off, val = list_sparse(g, q, len(cs.seqs[xs[q]]))
                    w = wants[q]
                    assert np.array_equal(off, w["off"]) and np.array_equal(val, w["val"]), (tag, q, call.pairs[q], "get_list_sparse")
            with_env(call.env, sparse)
    finally:
        g.close()
    if traced:
        print("OK case", flush=True)


def check_case_traced(size, name, lib_path=None, timeout=900):
    """run_case in a child process with MPCGPU_TRACE=1 (read once per process): the fb instantiations and the alignment kernel of
    every call, from the lines between its CALL and END markers"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MPCGPU_TRACE="1", PYTHONPATH=os.path.dirname(here) + os.pathsep + here)
    r = subprocess.run([sys.executable, "-u", os.path.join(here, "_align_pairs.py"), size, name, lib_path or ""], env=env, cwd=here,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout, text=True)
    out = r.stdout
    assert r.returncode == 0 and "OK case" in out, "exit %d\n%s" % (r.returncode, out[-4000:])
    cs = case(size, name)
    parts = out.split("CALL ")[1:]
    assert len(parts) == len(cs.calls), (name, len(parts))
    for call, part in zip(cs.calls, parts):
        head, body = part.split("\n", 1)
        body = body.split("\nEND\n", 1)[0]
        lines = [ln for ln in body.splitlines() if ln.startswith("[mpcgpu]")]
        tag = (name, head, call.what)
        if call.refused:
            continue
        lens = cs.lens(call)
        lm = long_min_of(call.env)
        short_h = sorted(int(ln[len(SHORT_FB):].split()[0]) for ln in lines if ln.startswith(SHORT_FB))
        fb_h = {int(ln.split("H=")[1].split()[0]) for ln in lines if ln.startswith("[mpcgpu] fb H=") or ln.startswith("[mpcgpu] fb chains H=")}
        chain_h = [ln for ln in lines if ln.startswith("[mpcgpu] fb chains H=")]
        rb_h = {int(ln.split("H=")[1].split()[0]) for ln in lines if ln.startswith("[mpcgpu] fb row blocks: H=")}
        aln = [ln.split("calc_aln ", 1)[1] for ln in lines if ln.startswith("[mpcgpu] calc_aln ")]
        bins = sorted({(LX + 63) // 64 for LX, _ in lens})
        if call.path in ("short", "overflow"):
            assert short_h == bins, (tag, "short-path bins", short_h, bins)
        else:
            assert short_h == [], (tag, "the short path ran", short_h)
        if call.path == "short":
            assert not fb_h and not rb_h and not aln, (tag, "stage A or a per-pair alignment ran", lines[:6])
            continue
        want_h = {(LX + 63) // 64 for LX, _ in lens if LX < lm}
        assert fb_h == want_h, (tag, "fb bins", sorted(fb_h), sorted(want_h))
        nochain = call.mega or call.env.get("MPCGPU_FB_CHAIN") == "0"
        if nochain:
            assert not chain_h, (tag, "fb_chain_kernel ran", chain_h[:3])
        long_h = env_int(call.env, "MPCGPU_FB_LONG_H", 0) or LONG_H
        want_rb = {long_h} if any(LX >= lm for LX, _ in lens) else set()
        assert rb_h == want_rb, (tag, "row blocks", rb_h, want_rb)
        want_aln = []
        for q0, nq in chunks_of(len(lens), call.env) if call.path == "general" else [(0, len(lens))]:
            sub = lens[q0:q0 + nq]
            if not all(one_wave(*l) for l in sub):
                want_aln += ["%d x %d: %s" % (LX, LY, aln_class(LX, LY)) for LX, LY in sub]
        assert aln == want_aln, (tag, "calc_aln kernels", aln[:8], want_aln[:8])
    return out


if __name__ == "__main__":
    run_case(case(sys.argv[1], sys.argv[2]), sys.argv[3] or None, traced=True)
