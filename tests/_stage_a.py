"""Path-pinned checks of all-pairs stage A (mpcgpu_calc_posteriors -> stage_a(), muscle_amd/csrc/mpcgpu_stage_a.inc) against the oracle,
bit for bit. Shared by tests/test_gpu_stage_a.py (production shapes), tests/test_emu_parity.py (the same rows, thin shapes and lowered
knobs) and tests/test_stage_a_table.py (the predictor alone, no device).

Every run of a case compares EA bits, nnz, offsets and values of every pair after stage A with the oracle (fwd, bwd, CalcPostFlat,
FromPost, EA per pair, as orc_pair_posterior composes them), then build_store and two cons_iter / cons_commit rounds with the oracle's
relax seeded from the same matrices (Run.deep; a run of fewer than three sequences stops after the store, as mpcflat.cpp:176 does).
A pair sub-range is read through its shard: the three ranges [0,k0) [k0,k1) [k1,N) are exported, imported as one store and compared.

predict() restates the dispatcher from sequence lengths, the pair range, the environment and the oracle's candidate counts: long_min
(stage_a_geom), the bin of every pair (build_chains, prepare_batch), the row-block instantiation (launch_fb_row_blocks), the first candidate
room and its doublings up to LXmax * LYmax (stage_a_geom, stage_a's overflow retry), the finishing kernel and its LDS bytes (post_rows_fits,
launch_post_rows, fill_post), per_pair / bmax / batches of equal size (prepare_batch), shard replacements (pack_batch), and from these the
order of launches (stage_a's loop) and the launch counts per timer
family (0: one per non-empty single bin, chain bin and the row-block bin, per batch and attempt; 1: one finishing kernel per attempt
and one pack per batch). Whether a pair under long_min runs in fb_chain_kernel or alone in fb_kernel depends on ChainPlan::vcap (chain_plan:
occupancy and free memory), which the host cannot restate: the predictor fixes the SUM per batch and bin, and exactly "all chained" /
"none chained" where Run.chain says so (MPCGPU_FB_CHAIN=0, Mega, or MPCGPU_FB_CHAIN_GRADE=0 with the default scratch budget and
lengths far inside the room). The batch budget is min(MPCGPU_SCRATCH_GB, 40 % of free memory): every run must batch the same way at
FREE_MIN and with unlimited memory (asserted), so the prediction does not depend on the box. Unforced, 4 rows per lane are chosen only
above cus * 8 resident waves: every run keeps at most 16 row-block pairs, so unforced means 7.

Proof of path. In process (timers on, no trace: the batches overlap as in production): timers_get() launch counts and stage_a_info().
In a child process with MPCGPU_TRACE=1: the "fb H=", "fb chains H=" + "fb chain members H=", "fb row blocks: H=", "post rows:" /
"post:", "stage A overflow:" and "stage A shard:" lines, parsed into launch groups, must equal the predicted sequence.

Where each path is reached (gpu: test_gpu_stage_a.py::test_stage_a_case[NAME], emu: test_emu_parity.py::test_emu_stage_a_case[NAME];
same names on both) and what proves it:
  bins H = 1..12, both edges of a class      bins_chain (default), bins_single (MPCGPU_FB_CHAIN=0), bins_mega: fb lines name each H
    LY = 1, LY + 1 < T, chainable Y            with the predicted pairs; chain members == pairs / no chain line
  bins 13..16                                bins_hi (MPCGPU_FB_LONG_MIN=1025; default, CHAIN=0, Mega): as above, no row-block line
  threshold 768 / 769, 1024 / 1025           threshold: 768 in bin 12, from 769 "fb row blocks: H=7 pairs= blocks<="
  row blocks 7 / 4 / 1, block edges,         row_blocks (default + Mega, MPCGPU_FB_LONG_H=4, =1): the row-block line; the long
    long sequence as X and as Y                sequence between two short ones
  finishing: row lists in LDS, HBM list      post_rows (natural: candidates above sort_cap; MPCGPU_POST_SORT_CAP=8; MPCGPU_POST_BATCH=3)
    dynamic LDS > 64 KB                      post_rows_big_lds ("post rows: ... lds=" above 65536; gpu: 12 000 columns, emu: an LDS
                                               list of 9000 entries)
    general kernel, forced / own condition   post_general (MPCGPU_POST=sort: lists in LDS; with MPCGPU_POST_SORT_CAP=8 through the sort
                                               scratch), post_general_own (gpu: one sequence of 18 300 residues, last: sort and srow
                                               scratch; emu: MPCGPU_POST_SORT_CAP=19000 exceeds the same LDS formula, 2100 columns keep
                                               srow in scratch): "post: sort_cap= lds="
  batches: one                               every case without MPCGPU_SCRATCH_GB
    one pair per batch                       batch_pairs (MPCGPU_SCRATCH_GB=0, 21 pairs, several bins and a row-block pair)
    three batches of many pairs              batch_three (MPCGPU_SCRATCH_GB=1, one long last sequence): batch= of every fb line
    sub-range inside rows' runs              subrange
  overflow: one / two doublings, natural     overflow_one, overflow_two, overflow_natural (poly-A 60 x 100): launch counts + the
                                               "stage A overflow:" line (old and new room, batch). (emu: overflow_one is poly-A
                                               60 x 100 against the FLOOR of 1024 that MPCGPU_CAND_PER_ROW=1 leaves; the knob itself
                                               sets the room in overflow_two, gpu and emu, and in overflow_one on the gpu)
    the clamp at LXmax * LYmax               overflow_clamp: needs a pair with more candidates than max(1024, LXmax * LYmax / 2), more
                                               than half of its cells. Under the amino-acid tables no pair comes near (poly-A 34 x 60:
                                               29 %); under block_hmm() poly-A 26 x 78 has 1352 of 2028: room 1024 -> 2028, not 2048
  overflow x batches                         overflow_first / _middle / _last (MPCGPU_SCRATCH_GB=0): "next batch queued and dropped" /
                                               "not queued"; later fb lines carry the doubled capc
    B recomputed                             overflow_rebatch_first / _middle / _last (MPCGPU_SCRATCH_GB=1, MPCGPU_CAND_PER_ROW=40, block_hmm()):
                                               the overflow line's "(B pairs)" against batch= of the redone fb lines: smaller
  shard growth                               shard_growth: "stage A shard: buffer replaced ... record words kept" with words > 0
  reuse                                      reuse: Mega, letters, smaller, larger extents on one context
TEST INFRASTRUCTURE."""
import functools
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _align_pairs as A
import _oracle as O
from _align_pairs import bits, capc_of, env_int, long_min_of, post_rows_ok, regrowths, related, with_env, with_mega
from muscle_amd._lib import MpcGpu

LONG_H, LONG_H_SMALL = 7, 4     # mpcgpu.cpp:381-382
SCRATCH_GB = 32                 # mpcgpu_stage_a.inc: scratch_budget()
BMAX = 1 << 22                  # mpcgpu_stage_a.inc: prepare_batch()
LDS_CAP = 150 * 1024            # mpcgpu_stage_a.inc: post_rows_fits(), launch_post_rows()
FREE_MIN = {"gpu": 64 << 30, "emu": 4 << 30}  # free device memory a run may count on: a quarter of an MI355X; tests/emu/hip_emu.h:233
MAX_LONG_PAIRS = 16             # mpcgpu_stage_a.inc: launch_fb_row_blocks() with cus >= 2
MAX_GPU_CELLS = 10 ** 9         # the oracle's DP cells over the GPU table


def next_pow2(v):
    p = 1
    while p < v:
        p *= 2
    return p


# ---- the oracle -------------------------------------------------------------------------------------------------------------
_MEMO = {}


def block_hmm():
    """PairHMM tables under which a pair aligns as ONE ungapped block of the shorter sequence that slides along the longer one: matches
    cost nothing, every gapped letter e^-2, leaving a long gap for a match e^-12 (so a second block is out), short gaps e^-30. Every offset
    is then equally likely and a poly-A pair of LX < LY stores LX * (LY - LX + 1) cells of P = 1 / (LY - LX + 1) each: the only inputs
    found that put more than half of a pair's cells above the threshold (the clamp of the candidate room needs that)."""
    s, t, m, i, thr = A.hmm()[1]
    t = np.array(t, np.float32).reshape(5, 5).copy()  # pairhmm.h:11-19: M, IX, IY, JX, JY
    t[0, 0] = 0
    t[0, 1] = t[0, 2] = -30
    t[0, 3] = t[0, 4] = 0
    t[1, 0] = t[2, 0] = t[1, 1] = t[2, 2] = -1
    t[3, 0] = t[4, 0] = -12
    t[3, 3] = t[4, 4] = 0
    return np.array([-12, -30, -30, 0, 0], np.float32), t.ravel(), np.zeros_like(m), np.full_like(i, -2.0), thr


_HMMS = {}


def hmm_of(name):
    """(oracle HMM, tables for set_hmm) of a case: None = the amino-acid tables every other test uses, "block" = block_hmm()"""
    if name not in _HMMS:
        _HMMS[name] = A.hmm() if name is None else (O.make_hmm(*block_hmm()[:4]), block_hmm())
    return _HMMS[name]


def _pair(key, x, y, mega, hmm=None):
    _MEMO[key] = A.ap_oracle(hmm_of(hmm)[0], x, y, mega, path=False)


def oracle_pairs(seqs, mega=None, hmm=None):
    """stage A of every pair (i < j) on the oracle -> [dict(ea, off, val, cand)], remembered by content for the process"""
    n = len(seqs)
    keys, todo = [], []
    for i in range(n):
        for j in range(i + 1, n):
            key = (hmm, seqs[i], seqs[j]) if mega is None else (hmm, seqs[i], seqs[j], mega["key"], mega["profs"][i].tobytes(), mega["profs"][j].tobytes())
            keys.append(key)
            if key not in _MEMO:
                _MEMO[key] = None
                todo.append((key, seqs[i].encode(), seqs[j].encode(), None if mega is None else (mega["g"], mega["profs"][i], mega["profs"][j]), hmm))
    hmm_of(hmm)  # (the tables and the oracle library are loaded before the threads start)
    O.sparse_from_post(np.zeros((1, 1), np.float32))
    todo.sort(key=lambda t: -len(t[1]) * len(t[2]))
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(lambda t: _pair(*t), todo))
    return [_MEMO[k] for k in keys]


def oracle_relax(seqs, want, iters=2):
    """the oracle's store seeded with the stage-A matrices, and `iters` ConsIter rounds -> stages as P.run_oracle lists them"""
    st = O.Store(seqs)
    for k, w in enumerate(want):
        st.set(k, w["off"], w["val"])
    stages = [[(w["off"], w["val"]) for w in want]]
    cur = st
    if len(seqs) >= 3:
        for _ in range(iters):
            cur = cur.cons_iter()
            stages.append([cur.get(k) for k in range(st.npairs)])
    return stages


# ---- the predictor ----------------------------------------------------------------------------------------------------------
def post_lds(LXmax, LYmax, capc, env):
    """("rows" | "sort", dynamic LDS bytes, list entries in LDS) of the finishing kernel (mpcgpu_stage_a.inc: post_rows_fits(), launch_post_rows(), fill_post())"""
    cap_env = max(env_int(env, "MPCGPU_POST_SORT_CAP", A.POST_SORT_CAP), 2)
    if post_rows_ok([(LXmax, LYmax)], env):
        fixed = ((LXmax + 2 + 2 * (LYmax + 2)) * 4 + 7) & ~7
        sort_cap = min(capc, cap_env)
        if fixed + sort_cap * 8 > LDS_CAP:
            sort_cap = (LDS_CAP - fixed) // 8
        return "rows", fixed + sort_cap * 8, sort_cap
    sort_cap = min(next_pow2(capc), next_pow2(cap_env))
    return "sort", sort_cap * 8 + min(LYmax + 1, 2048) * 8, sort_cap


def predict(lens, env, cand, nnz, mega=False, free=None, shard_cap=0):
    """stage A over pairs of these (LX, LY), in order -> dict(long_min, long_h, events, fam0 (lo, hi), fam1, batches, shard_cap ...).
    events, in the order the library reaches them: ("fb", first pair, B, capc, {H: pairs}, row-block pairs, blocks<=) per launch group,
    ("post", kind, lds), ("overflow", first pair, B, old room, new room, next batch dropped), ("shard", first pair, words kept)"""
    n = len(lens)
    lm = long_min_of(env)
    LXmax, LYmax = max(a for a, _ in lens), max(b for _, b in lens)
    full = LXmax * LYmax
    lh_env = env_int(env, "MPCGPU_FB_LONG_H", 0)
    long_h = 1 if lh_env == 1 else LONG_H_SMALL if lh_env == LONG_H_SMALL else LONG_H
    longs = [(a, b) for a, b in lens if a >= lm]
    LXlong = max([a for a, _ in longs], default=0)
    budget = env_int(env, "MPCGPU_SCRATCH_GB", SCRATCH_GB) << 30
    if free is not None:
        budget = min(budget, int(free * 0.4))
    hdr = (16 + n * 8 + 7) // 8 * 8

    def size(b0, capc):
        per_pair = capc * 8 + (LXmax + LYmax + 4 * capc) * 4 + 64
        bmax = min(max(1, budget // per_pair), BMAX)
        left = n - b0
        nbat = (left + bmax - 1) // bmax
        return (left + nbat - 1) // nbat

    def fb(b0, capc):
        B = size(b0, capc)
        sub = lens[b0:b0 + B]
        bins = {}
        for a, _ in sub:
            if a < lm:
                bins[(a + 63) // 64] = bins.get((a + 63) // 64, 0) + 1
        nl = sum(1 for a, _ in sub if a >= lm)
        return ("fb", b0, B, capc, bins, nl, (LXlong + 64 * long_h - 1) // (64 * long_h) if nl else 0)

    capc = capc_of(lens, env)
    ev, done, words, fam0, fam1, batches, retries = [], 0, 0, [0, 0], 0, [], 0
    chain_on = not mega and env_int(env, "MPCGPU_FB_CHAIN", 1) != 0

    def count(e):
        lo = len(e[4]) + (1 if e[5] else 0)
        fam0[0] += lo
        fam0[1] += lo + (len(e[4]) if chain_on else 0)  # a bin may split into a chain launch and a single-pair launch
    cur = fb(0, capc)
    ev.append(cur)
    count(cur)
    while done < n:
        B = cur[2]
        ev.append(("post",) + post_lds(LXmax, LYmax, capc, env)[:2])
        fam1 += 1
        nxt = None
        if done + B < n:
            nxt = fb(done + B, capc)
            ev.append(nxt)
            count(nxt)
        if max(cand[done:done + B]) > capc:
            assert capc < full, "candidate overflow at full capacity"
            new = min(2 * capc, full)
            ev.append(("overflow", done, B, capc, new, nxt is not None))
            capc = new
            retries += 1
            cur = fb(done, capc)
            ev.append(cur)
            count(cur)
            continue
        w = words + sum(a + b + 4 * z for (a, b), z in zip(lens[done:done + B], nnz[done:done + B]))
        per = w / (done + B)
        est = hdr + int(per * 1.05 * n + 1024) * 4
        if max(est, hdr + w * 4) > shard_cap:
            need = max(hdr + int(per * 1.15 * n + 1024) * 4, hdr + w * 4)
            shard_cap = max(need, shard_cap + shard_cap // 2)
            ev.append(("shard", done, words))
        fam1 += 1
        words = w
        batches.append((done, B, capc))
        done += B
        cur = nxt
    kind, lds, sort_cap = post_lds(LXmax, LYmax, capc, env)
    return {"long_min": lm, "long_h": long_h if longs else 0, "long_pairs": len(longs), "events": ev, "fam0": tuple(fam0), "fam1": fam1,
            "batches": batches, "retries": retries, "capc0": capc_of(lens, env), "capc": capc, "post": kind, "lds": lds, "sort_cap": sort_cap,
            "hbm_list": kind == "rows" and max(cand) > sort_cap, "sort_scratch": kind == "sort" and next_pow2(max(cand)) > sort_cap,
            "srow_scratch": kind == "sort" and LYmax + 1 > 2048, "shard_cap": shard_cap, "chain_on": chain_on,
            "kept": [e[2] for e in ev if e[0] == "shard" and e[2] > 0]}


# ---- the case table ---------------------------------------------------------------------------------------------------------
class Run:
    """one mpcgpu_calc_posteriors call. seqs: the sequences (None: those of the previous run, no set_seqs); rng = (k0, k1) or None;
    chain: "all" (every pair under long_min is a chain member) / "none" / None (the sum alone); deep: store + two relax rounds
    (False: stage A, store and one round); want: what predict() must say, checked on the CPU (tests/test_stage_a_table.py)"""

    def __init__(self, what, seqs=None, env=None, rng=None, mega=None, chain=None, deep=True, **want):
        self.what, self.seqs, self.env, self.rng, self.mega, self.chain, self.deep, self.want = what, seqs, dict(env or {}), rng, mega, chain, deep, want
        self.hmm = None


class Case:
    def __init__(self, name, runs, timeout=60, hmm=None):
        """timeout: seconds the traced child may take: a few times what it takes on the emulator, where it is slowest (measured: under 5 s
        on the device for every case; 10 - 25 s on the emulator for the bins and row-block cases, under 8 s for the others); hmm: hmm_of()"""
        self.name, self.runs, self.timeout, self.hmm = name, runs, timeout, hmm
        seqs = None
        for r in runs:
            r.hmm = hmm
            seqs = r.seqs = r.seqs if r.seqs is not None else seqs
            if r.mega is not None:
                r.mega = with_mega(r.seqs, r.mega)

    def cells(self, seen):
        tot = 0
        for r in self.runs:
            s = r.seqs
            for i in range(len(s)):
                for j in range(i + 1, len(s)):
                    key = (s[i], s[j], None if r.mega is None else r.mega["key"])
                    if key not in seen:
                        seen.add(key)
                        tot += len(s[i]) * len(s[j])
        return tot


GRADE0 = {"MPCGPU_FB_CHAIN_GRADE": "0"}
CHAIN0 = {"MPCGPU_FB_CHAIN": "0"}


def edges(hs):
    return [v for H in hs for v in (64 * (H - 1) + 1, 64 * H)]


def unrelated(lengths, seed):
    rng = np.random.default_rng(seed)
    return ["".join(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), L)) for L in lengths]


@functools.lru_cache(None)
def cases(size):
    """the table: size "gpu" (production shapes) or "emu" (the same rows: thin shapes, one long sequence per run, lowered knobs)"""
    gpu = size == "gpu"
    out = []
    # ---- bins: both edges of every rows-per-lane class; Y = 1 (and T - 2: too short to chain), 30, chainable lengths
    ys = [300, 30, 1, 62, 511] if gpu else [63, 1]
    groups = [edges(range(1, 13))] if gpu else [[v] for v in edges(range(1, 13))]
    sets = [related(g + ys, 201 + k) for k, g in enumerate(groups)]
    out.append(Case("bins_chain", [Run("edges %d" % len(s0[0]), s0, GRADE0, chain="all", bins=g) for g, s0 in zip(groups, sets)], timeout=120))
    out.append(Case("bins_single", [Run("edges %d, MPCGPU_FB_CHAIN=0" % len(s0[0]), s0, CHAIN0, chain="none", bins=g) for g, s0 in zip(groups, sets)], timeout=120))
    out.append(Case("bins_mega", [Run("edges %d, Mega" % len(s0[0]), s0, mega=7, chain="none", bins=g) for g, s0 in zip(groups, sets)], timeout=120))
    hi = {"MPCGPU_FB_LONG_MIN": "1025"}
    groups = [edges(range(13, 17))] if gpu else [[v] for v in edges(range(13, 17))]
    sets = [related(g + (ys[:3] if gpu else ys), 231 + k) for k, g in enumerate(groups)]
    runs = []
    for g, s0 in zip(groups, sets):
        runs += [Run("H 13..16", s0, dict(hi, **GRADE0), chain="all", bins=g, long_h=0), Run("H 13..16, CHAIN=0", None, dict(hi, **CHAIN0), chain="none", bins=g, long_h=0),
                 Run("H 13..16, Mega", None, hi, mega=8, chain="none", bins=g, long_h=0)]
    out.append(Case("bins_hi", runs, timeout=120))
    # ---- the row-block threshold
    tail = [300, 1] if gpu else [9, 1]
    sets = [related(g + tail, 241 + k) for k, g in enumerate([[768, 769, 1024, 1025]] if gpu else [[768], [769], [1024], [1025]])]
    out.append(Case("threshold", [Run("LX %s" % [len(x) for x in s0[:-2]], s0, GRADE0, long_h=None) for s0 in sets]))
    # ---- row blocks: block edges of each instantiation, the long sequence as Y (behind a short one) and as X (before one)
    rb = []
    for k, (lh, xs, env) in enumerate([(7, [896, 897, 1344, 1345], {}), (4, [1024, 1025, 1280, 1281], {"MPCGPU_FB_LONG_H": "4"}),
                                       (1, [128, 129, 192, 193], {"MPCGPU_FB_LONG_H": "1", "MPCGPU_FB_LONG_MIN": "65"})]):
        for g in ([xs] if gpu else [[v] for v in xs]):
            # (emu: the relax of a long sequence between two short ones takes the emulator 6 s a round; there the long sequence is a
            # column sequence in a run of two sequences, which ends with the store (mpcflat.cpp:176), and a row sequence before two short ones)
            s0 = related(([250] if gpu else []) + g + ([200] if gpu else [6, 5]), 251 + k)
            rb.append(Run("H = %d, LX %s" % (lh, g), s0, env, long_h=lh))
            if lh == 7:
                rb.append(Run("H = 7, Mega, LX %s" % g, None, env, mega=9, long_h=7))
            if not gpu:
                rb.append(Run("H = %d, LY %s" % (lh, g), related([6] + g, 255 + k), env, long_h=0))
    out.append(Case("row_blocks", rb, timeout=180))
    # ---- finishing kernels
    s0 = related([400] * 8, 261) if gpu else related([60] * 5, 261)
    out.append(Case("post_rows", [Run("row lists, natural", s0, {} if gpu else {"MPCGPU_POST_SORT_CAP": "64"}, post="rows", hbm_list=True),
                                  Run("MPCGPU_POST_SORT_CAP=8", None, {"MPCGPU_POST_SORT_CAP": "8"}, post="rows", hbm_list=True),
                                  Run("MPCGPU_POST_BATCH=3", None, {"MPCGPU_POST_BATCH": "3"}, post="rows"),
                                  Run("lists in LDS", related([90, 60, 70, 40], 262), {}, post="rows", hbm_list=False)]))
    shorts = [50, 60, 45] if gpu else [5, 6, 4]
    # (emu: the list itself is made long instead of the sequences: a room of 200 x 50 candidates, 9000 of them in LDS)
    s0, env = (related(shorts + [12000], 263), {}) if gpu else (related(shorts + [50], 263), {"MPCGPU_CAND_PER_ROW": "200", "MPCGPU_POST_SORT_CAP": "9000"})
    out.append(Case("post_rows_big_lds", [Run("LDS above 64 KB", s0, env, post="rows", lds_above=65536)]))
    s0 = related([80, 60, 70, 40] if gpu else [40, 20, 30, 10], 264)
    out.append(Case("post_general", [Run("MPCGPU_POST=sort", s0, {"MPCGPU_POST": "sort"}, post="sort", sort_scratch=False, srow_scratch=False),
                                     Run("MPCGPU_POST=sort, lists through scratch", None, {"MPCGPU_POST": "sort", "MPCGPU_POST_SORT_CAP": "8"}, post="sort",
                                         sort_scratch=True, srow_scratch=False)]))
    # (emu: the row-list kernel's LDS formula is exceeded by an LDS list of 19 000 entries instead of 18 300 columns; 2100 columns keep srow in scratch)
    if gpu:
        runs = [Run("LY 18 300", related(shorts + [18300], 265), {}, post="sort", sort_scratch=True, srow_scratch=True)]
    else:
        runs = [Run("LDS list of 19 000", related(shorts + [2100], 265), {"MPCGPU_POST_SORT_CAP": "19000"}, post="sort", sort_scratch=False, srow_scratch=True)]
    out.append(Case("post_general_own", runs))
    # ---- batches
    if gpu:
        s0, env = related([800, 70, 130, 200, 40, 300, 90], 271), {"MPCGPU_SCRATCH_GB": "0"}
    else:
        s0, env = related([130, 20, 70, 30, 9, 66, 12], 271), {"MPCGPU_SCRATCH_GB": "0", "MPCGPU_FB_LONG_MIN": "100", "MPCGPU_FB_LONG_H": "1"}
    out.append(Case("batch_pairs", [Run("one pair per batch", s0, env, nbatches=21, long_h=7 if gpu else 1)]))
    if gpu:
        s0, env = related([40 + 2 * k for k in range(40)] + [12000], 272), {"MPCGPU_SCRATCH_GB": "1"}
    else:
        s0, env = related([6 + k % 9 for k in range(24)] + [500], 272), {"MPCGPU_SCRATCH_GB": "1", "MPCGPU_CAND_PER_ROW": "800"}
    out.append(Case("batch_three", [Run("three batches", s0, env, deep=False, nbatches=3, min_batch=90)]))
    s0 = related([150, 90, 200, 60, 130, 170, 40, 110] if gpu else [30, 18, 40, 12, 26, 34, 8, 22], 273)
    out.append(Case("subrange", [Run("pairs [4, 17)", s0, GRADE0, rng=(4, 17))]))
    # ---- candidate overflow on one batch
    one = {"MPCGPU_CAND_PER_ROW": "1"}
    s0 = related([700, 690, 680], 281) if gpu else ["A" * 60, "A" * 100, "MKVLA"]  # (emu: the floor of 1024 against poly-A's 1627)
    out.append(Case("overflow_one", [Run("one doubling", s0, one, retries=1)]))
    out.append(Case("overflow_two", [Run("two doublings", ["A" * 150, "A" * 120, related([100], 282)[0]], one, retries=2)]))
    out.append(Case("overflow_clamp", [Run("the clamp", ["A" * 26, "A" * 20, "A" * 78], {}, retries=1, clamped=True)], hmm="block"))
    out.append(Case("overflow_natural", [Run("poly-A 60 x 100", ["A" * 60, "A" * 100] + related([80], 283), {}, retries=1)]))
    # ---- candidate overflow in the first, a middle and the last of many batches
    fam = related([80, 60, 70] if gpu else [30, 20, 25], 284)
    env = {"MPCGPU_SCRATCH_GB": "0"}
    out.append(Case("overflow_first", [Run("first batch", ["A" * 60, "A" * 100] + fam, env, retries=1, retry_at=0, dropped=True)]))
    out.append(Case("overflow_middle", [Run("middle batch", fam[:2] + ["A" * 60, "A" * 100] + fam[2:], env, retries=1, dropped=True)]))
    out.append(Case("overflow_last", [Run("last batch", fam + ["A" * 60, "A" * 100], env, retries=1, retry_at=9, dropped=False)]))
    # ---- the same with batches of many pairs, under block_hmm(): the room doubles, per_pair doubles, and the batch is redone SMALLER
    # (mpcgpu_stage_a.inc, stage_a()'s overflow retry: prepare_batch(.., done, cur) sizes it anew; the dropped next batch began at another pair). The room is
    # k x the longest sequence for every pair, a pair stores at most 100 cells per row, and a batch of B pairs under 1 GB has a room of about
    # 1 GB / 24 / B: so one dense pair of a x (a + 59) residues (60 equally likely offsets: 60 a candidates, P = 1 / 60) among short
    # poly-A sequences, whose pairs with the long ones store nothing (thousands of offsets)
    a, k, n = (3650, 40, 41) if gpu else (400, 40, 121)
    tiny = ["A" * (3 + q % 5) for q in range(n)]
    dense = ["A" * a, "A" * (a + 59)]
    env = {"MPCGPU_SCRATCH_GB": "1", "MPCGPU_CAND_PER_ROW": str(k), "MPCGPU_FB_LONG_H": "7"}
    mid = n * 3 // 10
    for where, s0, kw in (("first", dense + tiny, {"retry_at": 0, "dropped": True}), ("middle", tiny[:mid] + dense + tiny[mid:], {"dropped": True}),
                          ("last", tiny + dense, {"dropped": False})):
        out.append(Case("overflow_rebatch_" + where, [Run(where + " batch, B recomputed", s0, env, deep=False, retries=1, rebatch=True, forced_h=True, **kw)],
                        hmm="block", timeout=120))
    # ---- the shard buffer grows: sparse pairs first, dense ones last
    L, nr, nu = (150, 7, 10) if gpu else (24, 5, 7)
    # (related pairs are the sparse ones: a confident alignment stores little beside its diagonal; unrelated and poly-A pairs spread)
    s0 = related([L] * nr, 292) + unrelated([L] * nu, 291) + ["A" * L, "A" * (L - 10)]
    out.append(Case("shard_growth", [Run("sparse first, dense last", s0, {"MPCGPU_SCRATCH_GB": "0"}, kept=True)]))
    # ---- one context, run after run
    a = related([150, 90, 300, 40] if gpu else [40, 20, 70, 9], 293)
    b = related([60, 30, 45] if gpu else [12, 9, 10], 294)
    c = related([500, 800, 260, 100, 380] if gpu else [150, 200, 66, 30, 90], 295)
    lenv = {} if gpu else {"MPCGPU_FB_LONG_MIN": "129", "MPCGPU_FB_LONG_H": "1"}
    out.append(Case("reuse", [Run("Mega", a, {}, mega=10), Run("letters", None, {}), Run("smaller extents", b, {}), Run("larger extents", c, lenv)]))
    return out


CASE_NAMES = [c.name for c in cases("emu")]
assert CASE_NAMES == [c.name for c in cases("gpu")]


def case(size, name):
    return next(c for c in cases(size) if c.name == name)


def all_pairs(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def plan(run, size, shard_cap=0):
    """(oracle results of every pair, k0, k1, predict() of the run's range)"""
    want = oracle_pairs(run.seqs, run.mega, run.hmm)
    k0, k1 = run.rng or (0, len(want))
    lens = [(len(run.seqs[i]), len(run.seqs[j])) for i, j in all_pairs(len(run.seqs))][k0:k1]
    cand, nnz = [w["cand"] for w in want[k0:k1]], [int(w["off"][-1]) for w in want[k0:k1]]
    pr = predict(lens, run.env, cand, nnz, run.mega is not None, FREE_MIN[size], shard_cap)
    return want, k0, k1, lens, pr


def lanes_t(LX):
    """T of kernels_fbc.h: the lanes that own rows, ceil(LX / H)"""
    H = (LX + 63) // 64
    return (LX + H - 1) // H


def check_plan(run, size):
    """the run is on the path it claims and predictable on any box (no device): tests/test_stage_a_table.py"""
    want, k0, k1, lens, pr = plan(run, size)
    tag = (size, run.what)
    cand, nnz = [w["cand"] for w in want[k0:k1]], [int(w["off"][-1]) for w in want[k0:k1]]
    roomy = predict(lens, run.env, cand, nnz, run.mega is not None, None)
    assert roomy["events"] == pr["events"], (tag, "the batches depend on free memory")
    assert pr["long_pairs"] <= MAX_LONG_PAIRS or run.want.get("forced_h"), (tag, "row-block instantiation not predictable")
    lm = pr["long_min"]
    w = run.want
    if w.get("bins"):
        hs = {(a + 63) // 64 for a, _ in lens if a < lm}
        for v in w["bins"]:  # every edge length is a row sequence
            assert any(a == v for a, _ in lens), (tag, "edge", v)
        for a, b in lens:
            assert a < lm, tag
        edge_pairs = [(a, b) for a, b in lens if a in w["bins"]]
        assert any(b == 1 for _, b in edge_pairs), (tag, "no Y of one residue")
        if any(lanes_t(a) > 3 for a, _ in edge_pairs):
            assert any(b + 1 < lanes_t(a) for a, b in edge_pairs), (tag, "no Y too short to chain")
        assert hs, tag
    if "long_h" in w:
        want_h = w["long_h"]
        if want_h is None:  # threshold: by length alone
            want_h = LONG_H if any(a >= 769 for a, _ in lens) else 0
        assert pr["long_h"] == want_h, (tag, "row-block instantiation", pr["long_h"])
    if "post" in w:
        assert pr["post"] == w["post"], (tag, pr["post"])
    for key in ("hbm_list", "sort_scratch", "srow_scratch", "retries"):
        if key in w:
            assert pr[key] == w[key], (tag, key, pr[key], max(cand), pr["capc0"], pr["sort_cap"])
    if "lds_above" in w:
        assert pr["lds"] > w["lds_above"], (tag, pr["lds"])
    if "nbatches" in w:
        assert len(pr["batches"]) == w["nbatches"], (tag, pr["batches"])
        assert min(b for _, b, _ in pr["batches"]) >= w.get("min_batch", 1), (tag, pr["batches"])
    if w.get("retries"):
        # far from the edge: the room is exceeded by the stated number of doublings, neither fewer nor more, with a margin of 10 %
        full = max(a for a, _ in lens) * max(b for _, b in lens)
        room = pr["capc0"]
        top = max(cand)
        assert regrowths(lens, cand, run.env) == w["retries"] or len(pr["batches"]) > 1, tag
        last = min(room * 2 ** (w["retries"] - 1), full)
        assert top > last * 1.1, (tag, "not far above the room", top, last)
        if w.get("clamped"):
            assert pr["capc"] == full and full < 2 * last, (tag, pr["capc"], full)
        else:
            assert top * 1.1 < min(2 * last, full) or pr["capc"] == min(2 * last, full) and top <= pr["capc"], (tag, top, last)
        ov = [e for e in pr["events"] if e[0] == "overflow"]
        if w.get("rebatch"):  # the redone batch is smaller than the one that overflowed, and both hold many pairs
            at = pr["events"].index(ov[0])
            redo = pr["events"][at + 1]
            assert redo[0] == "fb" and redo[1] == ov[0][1] and 50 <= redo[2] < ov[0][2], (tag, "B not recomputed", ov[0], redo[:4])
            assert len(pr["batches"]) >= 3, (tag, pr["batches"])
        if "retry_at" in w:
            assert ov[0][1] == w["retry_at"], (tag, ov)
        if "dropped" in w:
            assert ov[0][5] == w["dropped"], (tag, ov)
            if len(pr["batches"]) > 2 and "retry_at" not in w:
                assert 0 < ov[0][1] < pr["batches"][-1][0], (tag, "not a middle batch", ov)
    else:
        assert pr["retries"] == 0 or "retries" in w, (tag, "an overflow the case does not state", pr["retries"])
    if w.get("kept"):
        assert pr["kept"], (tag, "the shard buffer is never replaced with records in it")
    return pr


# ---- running a case ---------------------------------------------------------------------------------------------------------
def _ctx(lib_path, run):
    s, t, m, i, thr = hmm_of(run.hmm)[1]
    g = MpcGpu(0, lib_path)
    g.set_hmm(s, t, m, i, thr)
    _load(g, run)
    return g


def _load(g, run):
    g.set_seqs(run.seqs)
    if run.mega is not None:
        mg = run.mega
        g.set_mega(mg["alpha"], mg["weight"], mg["lp"], mg["mx"], mg["profs"])


def _same_stage(tag, got, want):
    assert len(got) == len(want), tag
    for k, ((o1, v1), (o2, v2)) in enumerate(zip(got, want)):
        assert np.array_equal(o1, o2), (tag, "pair", k, "offsets")
        assert np.array_equal(v1, v2), (tag, "pair", k, "values")


def _relax(tag, g, run, want):
    """the store the shard became, and the relax rounds, against the oracle"""
    stages = oracle_relax(run.seqs, want, 2 if run.deep else 1)
    _same_stage(tag + ("store",), g.get_sparse_range(), stages[0])
    for r, st in enumerate(stages[1:]):
        g.cons_iter()
        g.cons_commit()
        _same_stage(tag + ("relax round", r + 1), g.get_sparse_range(), st)


def run_case(cs, size, lib_path=None, traced=False, relax=True):
    """every run of the case on one context: path proofs in process, stage A, store and relax against the oracle. traced: print the
    markers check_output reads; relax=False: stop after stage A (a traced child whose parent compared the rest in process)"""
    g, prev, shard_cap, mems = None, None, 0, []
    try:
        for k, run in enumerate(cs.runs):
            tag = (cs.name, k, run.what)
            want, k0, k1, lens, pr = plan(run, size, shard_cap)
            shard_cap = pr["shard_cap"]
            if g is None:
                g = _ctx(lib_path, run)
                g.timers_enable(True)
            elif run.seqs is not prev.seqs or (run.mega is None) != (prev.mega is None):
                _load(g, run)
            prev = run
            g.timers_reset()
            if traced:
                print("RUN %s|%d" % (cs.name, k), flush=True)
                sys.stderr.flush()
            with_env(run.env, lambda: g.calc_posteriors(k0, k1))
            sys.stderr.flush()
            tm = g.timers_get()
            sa = g.stage_a_info()
            if traced:
                print("END fb=%d post=%d" % (tm["fb"][1], tm["post"][1]), flush=True)
            lo, hi = pr["fam0"]
            if run.chain is not None or not pr["chain_on"]:
                hi = lo
            assert lo <= tm["fb"][1] <= hi, (tag, "launches of family 0", tm["fb"][1], pr["fam0"])
            assert tm["post"][1] == pr["fam1"], (tag, "launches of family 1", tm["post"][1], pr["fam1"])
            assert sa[0] == k1 - k0, (tag, "stage_a_info", sa)
            if run.chain == "none":
                assert sa[1:] == (0, 0), (tag, "chains", sa)
            ea = g.get_ea(k0, k1)
            nnz = g.get_nnz(k0, k1)
            sub = want[k0:k1]
            assert np.array_equal(bits(ea), bits(np.array([w["ea"] for w in sub], np.float32))), (tag, "EA")
            assert np.array_equal(nnz, np.array([int(w["off"][-1]) for w in sub], np.uint32)), (tag, "nnz")
            if not relax:
                continue
            if run.rng is None:
                with_env(run.env, g.build_store)
                _relax(tag, g, run, want)
            else:
                mems.append(_subrange(tag, g, run, want, k0, k1, lib_path))
    finally:
        if g is not None:
            g.close()
        for mem in mems:
            mem.free()
    if traced:
        print("OK case %s" % cs.name, flush=True)


def _subrange(tag, g, run, want, k0, k1, lib_path):
    """the shard of [k0, k1) between the shards of [0, k0) and [k1, N) of two other contexts: imported as one store, then as any run"""
    from _pair_order import DevMem
    N = len(want)
    others = [_ctx(lib_path, run), _ctx(lib_path, run)]
    mem = DevMem(lib_path)
    try:
        others[0].calc_posteriors(0, k0)
        others[1].calc_posteriors(k1, N)
        parts = [others[0], g, others[1]]
        sizes = [p.shard_info()[0] for p in parts]
        buf = mem.alloc(sum(sizes))
        at = 0
        for p, nb in zip(parts, sizes):
            p.shard_export(buf + at)
            at += nb
        g.store_import([0, k0, k1], [k0, k1, N], sizes, buf)
        assert np.array_equal(bits(g.get_ea()), bits(np.array([w["ea"] for w in want], np.float32))), (tag, "EA after import")
        _relax(tag, g, run, want)
    finally:
        for p in others:
            p.close()
    return mem  # the store of g adopted the buffer: released after g is closed


# ---- the traced child -------------------------------------------------------------------------------------------------------
def _num(ln, key):
    return int(ln.split(key, 1)[1].split()[0].rstrip(",:"))


def parse_trace(lines):
    """[mpcgpu] lines of one run -> events as predict() lists them; an "fb" group sums single pairs and chain members per bin and
    also carries ({H: single pairs}, {H: chain members})"""
    ev, grp = [], None

    def close():
        nonlocal grp
        if grp is not None:
            ev.append(grp)
        grp = None

    def group():
        nonlocal grp
        if grp is None:
            grp = {"single": {}, "chain": {}, "rb": 0, "blocks": 0, "B": set(), "capc": set(), "rb_h": 0, "lines": 0}
        return grp
    for ln in lines:
        if ln.startswith("[mpcgpu] fb row blocks: H="):
            d = group()
            d["rb_h"], d["rb"], d["blocks"] = _num(ln, "H="), _num(ln, "pairs="), _num(ln, "blocks<=")
            d["lines"] += 1
        elif ln.startswith("[mpcgpu] fb H="):
            d = group()
            d["single"][_num(ln, "H=")] = _num(ln, "pairs=")
            d["B"].add(_num(ln, "batch="))
            d["capc"].add(_num(ln, "capc="))
            d["lines"] += 1
        elif ln.startswith("[mpcgpu] fb chains H="):
            group()["lines"] += 1
        elif ln.startswith("[mpcgpu] fb chain members H="):
            d = group()
            d["chain"][_num(ln, "H=")] = _num(ln, "pairs=")
            d["B"].add(_num(ln, "batch="))
            d["capc"].add(_num(ln, "capc="))
        elif ln.startswith("[mpcgpu] post rows:"):
            close()
            ev.append(("post", "rows", _num(ln, "lds=")))
        elif ln.startswith("[mpcgpu] post: sort_cap="):
            close()
            ev.append(("post", "sort", _num(ln, "lds=")))
        elif ln.startswith("[mpcgpu] stage A overflow:"):
            close()
            ev.append(("overflow", _num(ln, "at pair "), _num(ln, "("), _num(ln, "capc "), _num(ln, "-> "), "queued and dropped" in ln))
        elif ln.startswith("[mpcgpu] stage A shard:"):
            close()
            ev.append(("shard", _num(ln, "at pair "), _num(ln, "B, ")))
    close()
    return ev


def check_trace(tag, run, pr, lines, counts):
    got = parse_trace(lines)
    want = pr["events"]
    assert len(got) == len(want), (tag, "trace events", [e if isinstance(e, tuple) else "fb" for e in got], [e[0] for e in want])
    nfb = 0
    for e, w in zip(got, want):
        if w[0] != "fb":
            assert e == w, (tag, "trace event", e, w)
            continue
        assert isinstance(e, dict), (tag, "expected fb launches", e, w)
        _, b0, B, capc, bins, nl, blocks = w
        tot = {H: e["single"].get(H, 0) + e["chain"].get(H, 0) for H in set(e["single"]) | set(e["chain"])}
        assert tot == bins, (tag, "fb bins of the batch at pair %d" % b0, e, bins)
        if run.chain == "all":
            assert e["chain"] == bins and not e["single"], (tag, "pairs outside fb_chain_kernel", e)
        if run.chain == "none" or not pr["chain_on"]:
            assert e["single"] == bins and not e["chain"], (tag, "fb_chain_kernel ran", e)
        assert e["B"] <= {B} and e["capc"] <= {capc}, (tag, "batch size / room", e, B, capc)
        assert (e["rb"], e["blocks"], e["rb_h"]) == (nl, blocks, pr["long_h"] if nl else 0), (tag, "row blocks", e, w)
        nfb += e["lines"]
    assert counts == (nfb, pr["fam1"]), (tag, "launch counters against trace lines", counts, nfb, pr["fam1"])


def _child(size, names, lib_path, relax):
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MPCGPU_TRACE="1", PYTHONPATH=os.path.dirname(here) + os.pathsep + here)
    return subprocess.Popen([sys.executable, "-u", os.path.join(here, "_stage_a.py"), size, ",".join(names), lib_path or "", "1" if relax else "0"],
                            env=env, cwd=here, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def check_output(size, name, out):
    """the traced output of one case: the launch groups, finishing kernels, retries and shard replacements of every run, from the
    lines between its RUN and END markers, against predict()"""
    cs = case(size, name)
    assert "OK case %s\n" % name in out, out[-4000:]
    parts = out.split("RUN %s|" % name)[1:]
    assert len(parts) == len(cs.runs), (name, len(parts))
    shard_cap = 0
    for k, (run, part) in enumerate(zip(cs.runs, parts)):
        body, end = part.split("\n", 1)[1].split("\nEND ", 1)
        counts = tuple(int(x.split("=")[1]) for x in end.split("\n", 1)[0].split())
        pr = plan(run, size, shard_cap)[4]
        shard_cap = pr["shard_cap"]
        check_trace((name, k, run.what), run, pr, [ln for ln in body.splitlines() if ln.startswith("[mpcgpu]")], counts)


def check_case_traced(size, name, lib_path=None):
    """run_case(relax=False) in a child process of its own with MPCGPU_TRACE=1 (read once per process), under the case's timeout"""
    p = _child(size, [name], lib_path, False)
    try:
        out = p.communicate(timeout=case(size, name).timeout)[0]
    except subprocess.TimeoutExpired:
        p.kill()
        raise AssertionError("%s: the traced child ran longer than %d s\n%s" % (name, case(size, name).timeout, p.communicate()[0][-4000:]))
    assert p.returncode == 0, "exit %d\n%s" % (p.returncode, out[-4000:])
    check_output(size, name, out)
    return out


EMU_CHILDREN = 4


@functools.lru_cache(None)
def emu_table(lib_path):
    """The emulator twin runs every case ONCE, traced, comparisons included (run_case(traced=True, relax=True)): the emulator executes a
    stream in order, so an untraced run beside it would repeat the same launches and see nothing more. The table is spread over
    EMU_CHILDREN child processes that run side by side (cases dealt out by their run counts), each under the sum of its cases' timeouts;
    a case that fails is reported and the child goes on. -> {case name: its output}"""
    names = sorted(CASE_NAMES, key=lambda n: -len(case("emu", n).runs))
    shares = [names[k::EMU_CHILDREN] for k in range(EMU_CHILDREN)]
    procs = [_child("emu", sh, lib_path, True) for sh in shares]
    out = {}
    for sh, p in zip(shares, procs):
        try:
            text = p.communicate(timeout=sum(case("emu", n).timeout for n in sh))[0]
        except subprocess.TimeoutExpired:
            p.kill()
            text = p.communicate()[0] + "\nTIMEOUT\n"
        for n, part in zip(sh, text.split("CASE ")[1:]):
            out[n] = part
    return out


def check_case_emu(name, lib_path):
    out = emu_table(lib_path).get(name)
    assert out is not None and out.startswith(name + "\n"), "the child did not reach %s" % name
    check_output("emu", name, out)


if __name__ == "__main__":
    import traceback
    failed = 0
    for _name in sys.argv[2].split(","):
        print("CASE %s" % _name, flush=True)
        try:
            run_case(case(sys.argv[1], _name), sys.argv[1], sys.argv[3] or None, traced=True, relax=sys.argv[4] == "1")
        except Exception:
            traceback.print_exc(file=sys.stdout)
            print("FAILED case %s" % _name, flush=True)
            failed += 1
    sys.exit(1 if failed else 0)
