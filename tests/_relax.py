"""Path-pinned checks of the store build and the consistency relax (build_var_store in mpcgpu_store.inc, mpcgpu_cons_iter in
mpcgpu_exchange.inc, the band tile cutter and the launches in mpcgpu_relax.inc) against the oracle, bit for bit. Shared by
tests/test_gpu_relax.py (hardware: the hand-scheduled merges), tests/test_emu_relax.py (the same rows on the emulator) and
tests/test_relax_table.py (what the inputs are claimed to be, from the oracle's matrices alone, no device).

Every run of a case compares EA, the store after the build and the store after every iteration with P.run_oracle, 0 ulp. A run is
one store on the case's context: set_seqs, stage A, build_store under the run's environment, then the run's script: a list of
iterations, each a list of pair ranges relaxed before ONE commit (None: the full range). Proof of path: relax_info() (store
description, tile description, kernel=), store_info()["window_bytes"], the launch counter of the relax family in timers_get(), and the
MPCGPU_TRACE lines of the run. MPCGPU_TRACE is read once per process: every case runs in a child process of its own, traced, under
its own timeout; after a child that died of a signal or ran into its timeout no further child is started (GPU table).

Where each path is reached (gpu: test_gpu_relax.py::test_relax_case[NAME], emu: test_emu_relax.py::test_emu_relax_case[NAME]):
 store build (build_var_store)
  narrow rows: window records                store_windows: "+ window records", window_bytes > 0, MpcRbWinAsm
  rows too wide for the 125 % rule           store_wide (BASE: the 3-residue and the unrelated 70-residue sequence): the trace line
                                               "no window records (rows too wide", cell order "pairs" in the launch line
  MPCGPU_RELAX_FORM=walk                     store_walk: no window line at all, MpcRbBlocksAsm
  MPCGPU_RELAX_WIN_PCT forced                store_win_pct (BASE at 100000 %): windows although 154 % of the blocks
  MPCGPU_RELAX_SMALL_PAIRS=40                small_pairs: n = 40 relax_var_kernel and no "band index"; n = 41 band; n = 40 with
                                               MPCGPU_RELAX_TILES=band: band; n = 40 with a primary budget one pair does not fit
                                               (two 300-residue sequences, MPCGPU_RELAX_LDS_KB=11): band index built, relax_band_kernel runs
  var_mixed                                  var_mixed (TILES=pairs, LDS 4 KB / 8 KB): "second launch", 2 launches per iteration
  slabs (MPCGPU_RELAX=gather, a sequence above MPC_RV_MAXLEN, a record over 4095 blocks): pinned in tests/test_gpu_parity.py
                                               (test_relax_gather_equals_tiled and the long-sequence tests), not repeated here
 mpcgpu_cons_iter, two iterations each
  band refuses with windows                  iter_drop_windows: "MpcRbBlocks", window_bytes 0 afterwards, "+ window records" gone
  band refuses: relax_var at iteration time  iter_to_var: relax_var_kernel in both iterations, one cut attempt only (band_ok false)
  band refuses, pairs do not fit: slabs      iter_to_slabs: relax_fallback, relax_kernel in the getters and the second iteration
  split ranges                               split_ranges: [0,k) [k,N) one commit; the full range (the cached cut is of another range);
                                               an empty range. (A range of pairs without a cell: the oracle stores a cell for every
                                               pair tried, down to 3 residues against 70 unrelated ones: no case)
 cutter (choose_shape, fit_or_split, split_tail)
  forced shape, out-of-range values          shape_forced ("band tiles forced: 4x2"), shape_out_of_range (0,4 and 9,9: "is not a shape")
  route 2 taken / refused into route 3       route2, route3_fill ("one band per 8x8 super-tile: ... taken" / "refused", then
                                               "taken, the slots are filled")
  route 3 because nothing was cut            route3_uncut: n = 65 > 64, "taken, nothing was cut"
  route 3 refused, route 4 in either mode    route4_two_steps, route4_one_step: "not taken, searching", the description's mode
  exact worst step, halved by band / Y / X   fit_exact ("need the exact worst step"), halve_band_y_x (the "halves ... by band, by Y, by X" line)
  first-piece limit (MPC_RB_MAXFIRST)        pinned NOWHERE with a witness: it needs 64 KB of first pieces in one step of a tile. The
                                               "halves" trace line counts such tiles; no test asserts that count above 0
  "rows of pair do not fit" (return 2)       iter_to_var, iter_to_slabs, iter_drop_windows: the trace line
  split_tail, a half without a cell          split_tail: SHAPE=1,1, tiles >= 24 x (CUs / 4) (gpu: 57 sequences, 1596 pairs against 1536
                                               on 256 CUs, asserted from the device's count; emu: 2 CUs, 24), "cut in two by rows",
                                               ">= 1 halves without a cell dropped"
  stride-8 pricing (>= 724 sequences)        stays with test_rdrp1000_sampled_reference_pin; stores in segments and > 64 GiB with
                                               their own tests (tests/test_gpu_parity.py): no case here
 kernels
  four merges x two staging modes            merge_{win,blocks}_{asm,cxx}_{two,one}: kernel= names the merge, the description the mode
  cell-order blocks that do not divide       order3_win, order3_blocks: "cell order=blocks of 3 rows"
 context reuse                               reuse: window -> walk (20 KB, 80 KB) -> whole-record (small pairs) -> slabs (gather) -> window with other
                                               n and longest length on one context, each relaxed twice; relax_info of every store ==
                                               that of a fresh context
TEST INFRASTRUCTURE."""
import functools
import os
import subprocess
import sys

import numpy as np

import _golden as G
import _parity as P
from muscle_amd._lib import MpcGpu
from muscle_amd.synth import make_family

CUS = {"gpu": 256, "emu": 2}    # MI355X; tests/emu/hip_emu.h
SMALL = "40"                    # what the drop-in binary sets MPCGPU_RELAX_SMALL_PAIRS to (hostcxx/mpcflat_gpu.cpp)
MAX_GPU_CELLS = 25 * 10 ** 5    # the oracle's DP cells over the GPU table (tests/test_relax_table.py)


def tail_threshold(cus):
    """split_tail (mpcgpu_relax.inc): tiles from which the tail is cut, and the resident workgroups of an XCD"""
    per_xcd = max(cus * 2 // 8, 1)
    return per_xcd * 8 * 3, per_xcd


# ---- inputs -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def base():
    """the set of test_emu_relax_band_tiles: ragged lengths 3 .. 75, rows wider than 31 columns, pairs without a cell"""
    return tuple(make_family(7, 75, seed=11) + make_family(3, 18, seed=5) + [make_family(1, 70, seed=9)[0], "MKV"])


@functools.lru_cache(None)
def narrow():
    """eight related sequences of one length: narrow rows (window records by the 125 % rule), steps of about equal size"""
    return tuple(make_family(8, 75, seed=11))


@functools.lru_cache(None)
def shorts(n, seed=41):
    """n related sequences of 9 .. 14 residues"""
    fam = make_family(n, 14, seed=seed)
    return tuple(s[:9 + k % 6] for k, s in enumerate(fam))


HEAD, HEAD2 = "MKVLAGHC", "TEYNDRFIMKVLAGHC"  # split_tail: a row sequence whose first index band alone aligns with its partner


@functools.lru_cache(None)
def tail_set(size):
    """SHAPE=1,1 makes one tile per pair: sequences of 17 .. 24 residues (>= 2 index bands of 8 rows), enough of them to pass the
    threshold, and one pair in a tail position whose rows from the middle on hold no cell: X = HEAD + 16 x W against Y = HEAD"""
    n = 57 if size == "gpu" else 8
    fam = make_family(n, 24, seed=43)
    seqs = [s[:17 + k % 8] for k, s in enumerate(fam)]
    x, y = tail_pair(size)
    seqs[x] = HEAD + "W" * 16
    seqs[y] = HEAD
    x, y = tail_pair2(size)
    seqs[x] = HEAD2 + "P" * 8
    seqs[y] = HEAD2
    return tuple(seqs)


def tail_pair(size):
    return (2, 40) if size == "gpu" else (0, 4)


def tail_pair2(size):
    """a second tail pair with cells in its first TWO index bands of three: cut one band too late, its second half would be dropped too"""
    return (3, 10) if size == "gpu" else (1, 2)


def tail_tiles(seqs, cus):
    """split_tail restated for one tile per pair: (pair, mid row) of every tile it cuts in two"""
    n = len(seqs)
    xs = [i for i in range(n) for _ in range(i + 1, n)]
    nt = len(xs)
    need, per_xcd = tail_threshold(cus)
    if nt < need:
        return []
    chunk = (nt + 7) // 8
    out = []
    for c0 in range(0, nt, chunk):
        c1 = min(c0 + chunk, nt)
        for t in range(c1 - per_xcd if c1 - c0 > per_xcd else c0, c1):
            hb = (len(seqs[xs[t]]) + 7) // 8
            if hb >= 2:
                out.append((t, hb // 2 * 8))
    return out


def tail_dropped(seqs, cus, shift=0):
    """halves without a cell among those of tail_tiles, from the oracle's matrices (shift: were they cut that many rows further down)"""
    st = oracle(seqs)[0][0]
    return sum((st[t][0][mid + shift] == 0) + (st[t][0][-1] == st[t][0][mid + shift]) for t, mid in tail_tiles(seqs, cus))


@functools.lru_cache(None)
def oracle(seqs, iters=2):
    return P.run_oracle(list(seqs), iters=iters)


# ---- the case table ---------------------------------------------------------------------------------------------------------
class Run:
    """one store on the case's context. env: in force for build_store and the relax; script: iterations, each a list of ranges
    ((k0, k1), None = full, "lo" / "hi" = the halves, "empty" = [k, k)) relaxed before one commit; mode: None or
    "gather" (MPCGPU_RELAX=gather). Witnesses: store / store_not (relax_info after the build), win (window_bytes > 0 after the
    build), then per iteration it[k] = dict(has, lacks, win, fallback, launches); trace / no_trace: substrings of the run's
    [mpcgpu] lines; claims: what tests/test_relax_table.py checks of the inputs"""

    def __init__(self, what, seqs, env=None, script=None, store=(), store_not=(), win=None, it=None, trace=(), no_trace=(), **claims):
        self.what, self.seqs, self.env = what, tuple(seqs), dict(env or {})
        self.script = script if script is not None else [[None], [None]]
        self.store, self.store_not, self.win, self.trace, self.no_trace, self.claims = store, store_not, win, trace, no_trace, claims
        self.it = it if it is not None else [{}] * len(self.script)
        assert len(self.it) == len(self.script)


class Case:
    def __init__(self, name, runs, timeout=120, fresh=False):
        """timeout: seconds the traced child may take (a few times what the slowest case takes on the emulator: 2 - 20 s a case there, measured; the
        device figure is not measured);
        fresh: every run again on a context of its own, relax_info equal"""
        self.name, self.runs, self.timeout, self.fresh = name, runs, timeout, fresh

    def cells(self, seen):
        tot = 0
        for r in self.runs:
            if r.seqs not in seen:
                seen.add(r.seqs)
                tot += sum(len(a) * len(b) for i, a in enumerate(r.seqs) for b in r.seqs[i + 1:])
        return tot


BAND = dict(has=("relax_band_kernel", "band tiles"))
WIN, BLOCKS = "MpcRbWinAsm", "MpcRbBlocksAsm"


def both(**kw):
    return [dict(kw), dict(kw)]


@functools.lru_cache(None)
def cases(size):
    B, N = base(), narrow()
    out = []
    add = lambda name, *runs, **kw: out.append(Case(name, list(runs), **kw))
    # ---- store build
    add("store_windows", Run("narrow rows", N, {}, store=("band index", "+ window records"), win=True, it=both(has=BAND["has"] + (WIN, "+ window records"), win=True, launches=1),
                             trace=("cell order=blocks of 8 rows",), no_trace=("no window records",), narrow=True))
    add("store_wide", Run("rows too wide", B, {}, store=("band index",), store_not=("window records",), win=False, it=both(has=BAND["has"] + (BLOCKS,), win=False, launches=1),
                          trace=("no window records (rows too wide", "cell order=pairs"), span_gt31=True))
    add("store_walk", Run("FORM=walk", N, {"MPCGPU_RELAX_FORM": "walk"}, store=("band index",), store_not=("window records",), win=False,
                          it=both(has=BAND["has"] + (BLOCKS,), win=False), trace=("cell order=pairs",), no_trace=("window records",), narrow=True))
    add("store_win_pct", Run("WIN_PCT=100000", B, {"MPCGPU_RELAX_WIN_PCT": "100000"}, store=("+ window records",), win=True,
                             it=both(has=BAND["has"] + (WIN,), win=True), no_trace=("no window records",), span_gt31=True))
    s40, s41 = shorts(40), shorts(41)
    sp = {"MPCGPU_RELAX_SMALL_PAIRS": SMALL}
    var = dict(has=("relax_var_kernel",), lacks=("band index", "band tiles"), win=False, launches=1)
    add("small_pairs",
        Run("n = 40", s40, sp, store=("relax_var_kernel",), store_not=("band index", "second launch"), win=False, it=both(**var), no_trace=("band tiles", "relax band"), n_le_small=True),
        Run("n = 41", s41, sp, store=("band index",), it=both(**BAND), trace=("relax band:",), n_gt_small=True),
        Run("n = 40, TILES=band", s40, dict(sp, MPCGPU_RELAX_TILES="band"), store=("band index",), it=both(**BAND), trace=("relax band:",), n_le_small=True),
        # (two records of the 300-residue pair, 2 x 5952 B, against a staging buffer of 11 KB - 512 B: the store's trace line says "relax_var
        # fallback for the largest pairs" exactly when the primary geometry does not fit; band tiles of 8 rows fit the 8.5 KB they get)
        Run("n = 40, a pair does not fit the primary budget", shorts(38) + tuple(make_family(2, 300, seed=11)), dict(sp, MPCGPU_RELAX_LDS_KB="11", MPCGPU_RELAX_LDS_KB_1024="24"),
            store=("band index",), store_not=("second launch", "relax_var_kernel"), it=both(has=BAND["has"], lacks=("second launch", "relax_var")),
            trace=("relax_var fallback for the largest pairs", "relax band:"), no_trace=("no band tile fits",), n_le_small=True),
        timeout=240)
    mixed = {"MPCGPU_RELAX_TILES": "pairs", "MPCGPU_RELAX_LDS_KB": "4", "MPCGPU_RELAX_LDS_KB_1024": "8"}
    add("var_mixed", Run("two geometries", tuple(make_family(4, 12, seed=31) + make_family(3, 60, seed=32) + make_family(3, 30, seed=33)), mixed,
                         store=("relax_var_kernel", "second launch"), store_not=("band index",), win=False,
                         it=both(has=("second launch", "+ 1 x 1024", "relax_var_kernel"), launches=2), trace=("primary buf=", "fallback buf=")))
    # ---- mpcgpu_cons_iter's fallbacks
    nofit = "do not fit (slots"
    add("iter_drop_windows", Run("LDS 9 KB, windows forced", B, {"MPCGPU_RELAX_WIN_PCT": "100000", "MPCGPU_RELAX_LDS_KB": "9"}, store=("+ window records",), win=True,
                                 it=both(has=BAND["has"] + (BLOCKS,), lacks=("window records",), win=False, launches=1, fallback=False),
                                 trace=(nofit, "windows dropped, the walk is cut"), trace_once=("windows dropped",), span_gt31=True))
    add("iter_to_var", Run("LDS 8 KB, 16 KB for one workgroup", B, {"MPCGPU_RELAX_LDS_KB": "8", "MPCGPU_RELAX_LDS_KB_1024": "16"}, store=("band index",), win=False,
                           it=both(has=("relax_var_kernel", "tiles:"), lacks=("band tiles",), fallback=False),
                           trace=(nofit, "no band tile fits: whole-record tiles"), trace_once=("no band tile fits", nofit)))
    add("iter_to_slabs", Run("LDS 8 KB", B, {"MPCGPU_RELAX_LDS_KB": "8"}, store=("band index",), win=False,
                             it=both(has=("CSR slabs", "kernel=relax_kernel"), lacks=("band", "relax_var"), fallback=True, launches=1),
                             trace=(nofit, "no band tile fits: CSR slabs"), trace_once=("no band tile fits", nofit)))
    add("split_ranges", Run("halves, full, empty", B, {}, script=[["lo", "hi"], [None, "empty"]], store=("band index",),
                            it=[dict(has=BAND["has"], launches=2, cuts=2), dict(has=BAND["has"], launches=1, cuts=1)]))
    # ---- the cutter
    add("shape_forced", Run("SHAPE=4,2", B, {"MPCGPU_RELAX_SHAPE": "4,2", "MPCGPU_RELAX_SLOTS": "2"}, it=both(has=("of <= 4x2 pairs",)), trace=("band tiles forced: 4x2",),
                            no_trace=("one band per 8x8",)))
    add("shape_out_of_range", Run("SHAPE=0,4", B, {"MPCGPU_RELAX_SHAPE": "0,4"}, it=both(has=("of <= 8x8 pairs",)), trace=("MPCGPU_RELAX_SHAPE=0,4 is not a shape", "one band per 8x8"),
                                  no_trace=("band tiles forced",)),
        Run("SHAPE=9,9", B, {"MPCGPU_RELAX_SHAPE": "9,9"}, it=both(has=("of <= 8x8 pairs",)), trace=("MPCGPU_RELAX_SHAPE=9,9 is not a shape", "one band per 8x8"),
            no_trace=("band tiles forced",)))
    add("route2", Run("12 sequences", B, {}, it=both(has=("3 band tiles of <= 8x8 pairs (0 split)",)), trace=("one band per 8x8 super-tile: 3 tiles, taken",),
                      no_trace=("two steps resident:",), n_le_64=True))
    add("route3_fill", Run("three sequences of 300, SLOTS=1", tuple(make_family(3, 300, seed=61)), {"MPCGPU_RELAX_SLOTS": "1"}, it=both(has=("of <= 8x8 pairs",)), supertile_cells_gt=1024,
                           trace=("refused (a super-tile over the slots", "taken, the slots are filled"), no_trace=("searching",), n_le_64=True))
    add("route3_uncut", Run("65 sequences", shorts(65, 47), {}, it=both(has=("of <= 8x8 pairs (0 split)",)), trace=("taken, nothing was cut",), no_trace=("one band per 8x8", "searching"),
                            n_gt_64=True), timeout=300)
    add("route4_two_steps", Run("LDS 9 KB", B, {"MPCGPU_RELAX_LDS_KB": "9", "MPCGPU_RELAX_FORM": "walk"}, it=both(has=("(two steps resident)",)),
                                trace=("not taken, searching", "one step resident = ")))
    add("route4_one_step", Run("LDS 9 KB, steps of equal size", N, {"MPCGPU_RELAX_LDS_KB": "9"}, it=both(has=("(one step resident)",)), trace=("not taken, searching",)))
    add("fit_exact", Run("LDS 12 KB, SHAPE=2,2,5", B, {"MPCGPU_RELAX_LDS_KB": "12", "MPCGPU_RELAX_SHAPE": "2,2,5"}, it=both(has=BAND["has"]), trace=("need the exact worst step",)))
    add("halve_band_y_x", Run("LDS 20 KB", B, {"MPCGPU_RELAX_LDS_KB": "20"}, it=both(has=BAND["has"]), halves=("band",)),
        Run("LDS 9 KB", B, {"MPCGPU_RELAX_LDS_KB": "9", "MPCGPU_RELAX_FORM": "walk"}, it=both(has=BAND["has"]), halves=("Y", "X")))
    x, y = tail_pair(size)
    add("split_tail", Run("SHAPE=1,1", tail_set(size), {"MPCGPU_RELAX_SHAPE": "1,1"}, it=both(has=("of <= 1x1 pairs",)), trace=("cut in two by rows",), tail=(x, y)))
    # ---- the kernels: four merges, both staging modes, on one small input
    for fam, form in (("win", {"MPCGPU_RELAX_WIN_PCT": "100000"}), ("blocks", {"MPCGPU_RELAX_FORM": "walk"})):
        for merge in ("asm", "cxx"):
            for mode, shape in (("two", "2,2,8"), ("one", "2,2,18")):  # 512 blocks of 1120: the next step beside the current one; all 1120
                env = dict(form, MPCGPU_RELAX_SHAPE=shape, MPCGPU_RELAX_LDS_KB="20")
                if merge == "cxx":
                    env["MPCGPU_RELAX_MERGE"] = "cxx"
                kn = "MpcRb%s%s>" % ("Win" if fam == "win" else "Blocks", merge.capitalize())
                add("merge_%s_%s_%s" % (fam, merge, mode), Run("%s, %s steps resident" % (kn, mode), B, env, it=both(has=(kn, "(%s step%s resident)" % (mode, "s" if mode == "two" else "")), launches=1)))
    o3 = {"MPCGPU_RELAX_ORDER": "3", "MPCGPU_RELAX_SHAPE": "8,8", "MPCGPU_RELAX_SLOTS": "1"}
    add("order3_win", Run("ORDER=3, windows", B, dict(o3, MPCGPU_RELAX_WIN_PCT="100000"), it=both(has=(WIN,)), trace=("cell order=blocks of 3 rows",)))
    add("order3_blocks", Run("ORDER=3, walk", B, dict(o3, MPCGPU_RELAX_FORM="walk"), it=both(has=(BLOCKS,)), trace=("cell order=blocks of 3 rows",)))
    # ---- one context, store after store
    s9 = shorts(9, 53)
    add("reuse",
        Run("windows", N, {}, store=("+ window records",), win=True, it=both(has=(WIN,), win=True)),
        # (the same kernel with a small and then the default staging area: the occupancy query is cached by kernel AND LDS size, and the
        # larger launch needs its own hipFuncSetAttribute)
        Run("walk, LDS 20 KB", N, {"MPCGPU_RELAX_FORM": "walk", "MPCGPU_RELAX_LDS_KB": "20"}, store_not=("window records",), win=False, it=both(has=(BLOCKS,), win=False),
            trace=("lds=20480 B", "asked at 20480 B"), trace_once=("asked at",)),
        Run("walk", N, {"MPCGPU_RELAX_FORM": "walk"}, store_not=("window records",), win=False, it=both(has=(BLOCKS,), win=False), trace=("lds=81920 B", "asked at 81920 B"),
            trace_once=("asked at",)),
        Run("whole records", s9, sp, store=("relax_var_kernel",), store_not=("band index",), win=False, it=both(**var)),
        Run("slabs", B, {"MPCGPU_RELAX": "gather"}, store=("CSR slabs",), win=False, it=both(has=("kernel=relax_kernel",), fallback=False, win=False)),
        Run("windows, other n and longest length", tuple(make_family(6, 90, seed=57)), {}, store=("+ window records",), win=True,
            it=both(has=(WIN,), win=True)),
        fresh=True, timeout=240)
    return out


CASE_NAMES = [c.name for c in cases("emu")]
assert CASE_NAMES == [c.name for c in cases("gpu")]
FALLBACK_CASES = ["iter_drop_windows", "iter_to_var", "iter_to_slabs"]


def case(size, name):
    return next(c for c in cases(size) if c.name == name)


# ---- what the inputs are claimed to be (no device) -------------------------------------------------------------------------
def pair_index(n, x, y):
    return x * n - x * (x + 1) // 2 + (y - x - 1)


def row_spans(stage):
    """(cells, widest row span in columns) over every row of every pair of a stage"""
    cells = span = 0
    for o, v in stage:
        cols = v[1::2]
        for i in range(len(o) - 1):
            if o[i + 1] > o[i]:
                cells += int(o[i + 1] - o[i])
                span = max(span, int(cols[o[i + 1] - 1]) - int(cols[o[i]]) + 1)
    return cells, span


def check_claims(run, size):
    st = oracle(run.seqs)[0][0]
    n, cl, tag = len(run.seqs), run.claims, (size, run.what)
    nnz = [len(v) // 2 for _, v in st]
    cells, span = row_spans(st)
    rows = sum(len(a) * (n - 1 - i) for i, a in enumerate(run.seqs))
    # every store here is of one segment, every sequence far below MPC_RV_MAXLEN, every pair within relax_var's 16 x 1024 cell slots
    assert max(len(s) for s in run.seqs) < 4095 and max(nnz) <= 13 * 1024, tag
    if cl.get("span_gt31"):  # the escape of the window descriptor's 5-bit span field
        assert span > 31, (tag, span)
    if cl.get("narrow"):
        assert span <= 31 and cells / rows < 4, (tag, span, cells / rows)
    if cl.get("n_le_64"):
        assert n <= 64, tag
    if cl.get("n_gt_64"):
        assert n > 64, tag
    if cl.get("n_le_small"):
        assert n == int(SMALL), tag
    if cl.get("n_gt_small"):
        assert n == int(SMALL) + 1, tag
    if "supertile_cells_gt" in cl:  # n <= 8: ONE super-tile, whose cells (every pair rounded up to whole waves) pass the slot budget of route 2
        assert n <= 8 and sum((z + 63) // 64 * 64 for z in nnz) > cl["supertile_cells_gt"] * int(run.env.get("MPCGPU_RELAX_SLOTS", 13)), (tag, sum(nnz))
    if "tail" in cl:
        need, per_xcd = tail_threshold(CUS[size])
        assert all(z > 0 for z in nnz), (tag, "a pair without a cell: tiles != pairs")
        assert all(len(s) >= 17 for s in run.seqs if s not in (HEAD, HEAD2)), tag
        nt = len(nnz)
        assert nt >= need, (tag, nt, need)
        x, y = cl["tail"]
        k = pair_index(n, x, y)
        chunk = (nt + 7) // 8
        c0 = k // chunk * chunk
        c1 = min(c0 + chunk, nt)
        assert c1 - per_xcd <= k < c1, (tag, "not a tail tile", k, c0, c1)
        o, v = st[k]
        hb = (len(run.seqs[x]) + 7) // 8
        mid = hb // 2 * 8
        assert hb >= 2 and o[mid] > 0 and o[-1] == o[mid], (tag, "the rows from %d on hold cells" % mid, list(o))
        x, y = tail_pair2(size)
        k = pair_index(n, x, y)
        o, v = st[k]
        assert (k, 8) in tail_tiles(run.seqs, CUS[size]) and o[8] > 0 and o[16] > o[8] and o[-1] == o[16], (tag, "second tail pair", list(o))
        # the count the trace line must state tells a cut one index band too late from the right one
        assert 1 <= tail_dropped(run.seqs, CUS[size]) != tail_dropped(run.seqs, CUS[size], 8), tag


# ---- running a case (in the traced child) ----------------------------------------------------------------------------------
def _with_env(env, fn):
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


def _ranges(it, npairs):
    out = []
    for r in it:
        if r is None:
            out.append((0, npairs))
        elif r == "lo":
            out.append((0, npairs // 2))
        elif r == "hi":
            out.append((npairs // 2, npairs))
        elif r == "empty":
            out.append((npairs // 3, npairs // 3))
        else:
            out.append(r)
    return out


def _same_stage(tag, got, want):
    assert len(got) == len(want), tag
    for k, ((o1, v1), (o2, v2)) in enumerate(zip(got, want)):
        assert np.array_equal(o1, o2), (tag, "pair", k, "offsets")
        assert np.array_equal(v1, v2), (tag, "pair", k, "values")


def _subs(tag, text, has=(), lacks=()):
    for s in has:
        assert s in text, (tag, "missing", s, text)
    for s in lacks:
        assert s not in text, (tag, "unexpected", s, text)


def run_store(g, cs, k, run, marks=True):
    """one run on context g -> the relax_info texts after the build and after every iteration"""
    tag = (cs.name, k, run.what)
    stages, ea = oracle(run.seqs, len(run.script))
    infos = []

    def body():
        g.set_seqs(list(run.seqs))
        g.calc_posteriors()
        assert np.array_equal(P.bits(g.get_ea()), P.bits(ea)), (tag, "EA")
        g.build_store()
        info, fb = g.relax_info()
        infos.append(info)
        _subs(tag + ("store",), info, run.store, run.store_not)
        if run.win is not None:
            assert (g.store_info()["window_bytes"] > 0) == run.win, (tag, "window_bytes", g.store_info())
        _same_stage(tag + ("store",), g.get_sparse_range(), stages[0])
        for q, (it, w) in enumerate(zip(run.script, run.it)):
            g.timers_reset()
            for k0, k1 in _ranges(it, g.npairs):
                g.cons_iter(k0, k1)
            launches = g.timers_get()["relax"][1]
            g.cons_commit()
            info, fb = g.relax_info()
            infos.append(info)
            _subs(tag + ("iteration", q), info, w.get("has", ()), w.get("lacks", ()))
            if w.get("win") is not None:
                assert (g.store_info()["window_bytes"] > 0) == w["win"], (tag, "iteration", q, "window_bytes", g.store_info())
            if w.get("fallback") is not None:
                assert fb == w["fallback"], (tag, "iteration", q, "relax_fallback", fb)
            if w.get("launches") is not None:
                assert launches == w["launches"], (tag, "iteration", q, "launches of the relax family", launches)
            if marks:
                sys.stderr.flush()
                print("ITER %d launches=%d" % (q, launches), flush=True)
            _same_stage(tag + ("iteration", q), g.get_sparse_range(), stages[q + 1])
            assert np.array_equal(P.bits(g.get_ea()), P.bits(ea)), (tag, "EA after iteration", q)
    env = dict(run.env)
    _with_env(env, body)
    return infos


def run_case(cs, size, lib_path=None):
    g = MpcGpu(0, lib_path)
    try:
        g.set_hmm(*G.hmm_tables())
        g.timers_enable(True)
        if cs.name == "split_tail":
            print("CUS threshold=%d pairs=%d" % (tail_threshold(CUS[size])[0], len(cs.runs[0].seqs) * (len(cs.runs[0].seqs) - 1) // 2), flush=True)
        shared = []
        for k, run in enumerate(cs.runs):
            print("RUN %s|%d" % (cs.name, k), flush=True)
            shared.append(run_store(g, cs, k, run))
            sys.stderr.flush()
            print("END", flush=True)
    finally:
        g.close()
    if cs.fresh:
        for k, run in enumerate(cs.runs):
            f = MpcGpu(0, lib_path)
            try:
                f.set_hmm(*G.hmm_tables())
                f.timers_enable(True)
                alone = run_store(f, cs, k, run, marks=False)
            finally:
                f.close()
            assert alone == shared[k], (cs.name, k, run.what, "relax_info on a fresh context differs", alone, shared[k])
    print("OK case %s" % cs.name, flush=True)


# ---- the parent: children, trace lines -------------------------------------------------------------------------------------
def _child(size, names, lib_path):
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MPCGPU_TRACE="1", PYTHONPATH=os.path.dirname(here) + os.pathsep + here)
    return subprocess.Popen([sys.executable, "-u", os.path.join(here, "_relax.py"), size, ",".join(names), lib_path or ""],
                            env=env, cwd=here, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _count(lines, sub):
    return sum(1 for ln in lines if sub in ln)


def check_output(size, name, out):
    """the traced output of one case: the child's own comparisons passed, and every run's [mpcgpu] lines name its path"""
    cs = case(size, name)
    assert "OK case %s\n" % name in out, out[-6000:]
    parts = out.split("RUN %s|" % name)[1:]
    assert len(parts) >= len(cs.runs), (name, len(parts))
    for k, (run, part) in enumerate(zip(cs.runs, parts)):
        tag = (name, k, run.what)
        body = part.split("\nEND\n", 1)[0]
        lines = [ln for ln in body.splitlines() if ln.startswith("[mpcgpu]")]
        text = "\n".join(lines)
        _subs(tag + ("trace",), text, run.trace, run.no_trace)
        for s in run.claims.get("trace_once", ()):  # the state the first iteration left is what the second ran on: no second attempt
            assert _count(lines, s) == 1, (tag, "lines with", s, _count(lines, s))
        its = body.split("\nITER ")
        for q, w in enumerate(run.it):
            if "cuts" in w:  # cuts of the tile list during this iteration
                assert _count(its[q].splitlines(), "band tiles: cut, checked and uploaded") == w["cuts"], (tag, "iteration", q, "cuts")
        if run.claims.get("halves"):
            got = {"band": 0, "Y": 0, "X": 0}
            for ln in lines:
                if "band tiles: round" in ln and " halves " in ln:
                    f = ln.split(" halves ", 1)[1].split()
                    got["band"] += int(f[0])
                    got["Y"] += int(f[4])
                    got["X"] += int(f[7])
            for d in run.claims["halves"]:
                assert got[d] > 0, (tag, "no tile halved by", d, got)
        if "tail" in run.claims:
            ln = next(ln for ln in lines if "cut in two by rows" in ln)
            f = ln.split("tail of ", 1)[1].split()
            tiles, cus, cut, dropped = int(f[0]), int(f[3]), int(f[5]), int(f[11])
            if size == "emu":
                assert cus == CUS[size], (tag, cus)
            need, per_xcd = tail_threshold(cus)  # as the library computes it from the device's count
            assert tiles >= need, (tag, "below the threshold", tiles, need)
            # one tile per pair (check_claims): the last per_xcd tiles of each of the 8 chunks, where the row sequence has two index bands
            n = len(run.seqs)
            want = tail_tiles(run.seqs, cus)
            assert tiles == n * (n - 1) // 2 and cut == len(want) and dropped == tail_dropped(run.seqs, cus) >= 1, (tag, ln, len(want), tail_dropped(run.seqs, cus))
            desc = next(ln for ln in lines if ln.startswith("[mpcgpu] relax band:") and "band tiles of <=" in ln)
            assert desc.split("relax band: ", 1)[1].split()[0] == str(tiles + cut - dropped), (tag, ln, desc)


_DEAD = {}
GPU_FAULT_TEXT = ("illegal memory access", "hipErrorIllegalAddress", "hipErrorLaunchFailure", "unspecified launch failure", "HSA_STATUS_ERROR")


def check_case(size, name, lib_path=None):
    """the case in a child process of its own with MPCGPU_TRACE=1, under the case's timeout; after a child that died of a signal or
    hung, nothing more is started on that library"""
    key = lib_path or "device"
    assert key not in _DEAD, "not started: the child of %s %s" % _DEAD.get(key, ("", ""))
    cs = case(size, name)
    p = _child(size, [name], lib_path)
    try:
        out = p.communicate(timeout=cs.timeout)[0]
    except subprocess.TimeoutExpired:
        p.kill()
        _DEAD[key] = (name, "ran longer than %d s" % cs.timeout)
        raise AssertionError("%s: the traced child ran longer than %d s\n%s" % (name, cs.timeout, p.communicate()[0][-4000:]))
    if p.returncode < 0 or p.returncode in (134, 139):
        _DEAD[key] = (name, "died with status %d" % p.returncode)
    elif p.returncode and any(s in out for s in GPU_FAULT_TEXT):  # a fault the runtime reported as an error: the child ended by itself
        _DEAD[key] = (name, "reported a GPU fault")
    assert p.returncode == 0, "exit %d\n%s" % (p.returncode, out[-6000:])
    check_output(size, name, out)
    return out


EMU_CHILDREN = 4


@functools.lru_cache(None)
def emu_table(lib_path, sched=None):
    """the emulator twin: the table dealt out to EMU_CHILDREN child processes that run side by side, each under the sum of its cases'
    timeouts; a case that fails is reported and the child goes on. sched: EMU_SCHED for FALLBACK_CASES alone. -> {name: output}"""
    names = FALLBACK_CASES if sched else CASE_NAMES
    nch = min(EMU_CHILDREN, len(names))
    shares = [names[k::nch] for k in range(nch)]
    if sched:
        os.environ["EMU_SCHED"] = sched
    try:
        procs = [_child("emu", sh, lib_path) for sh in shares]
    finally:
        os.environ.pop("EMU_SCHED", None)
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


def check_case_emu(name, lib_path, sched=None):
    out = emu_table(lib_path, sched).get(name)
    assert out is not None and out.startswith(name + "\n"), "the child did not reach %s" % name
    check_output("emu", name, out)


if __name__ == "__main__":
    import traceback
    failed = 0
    for _name in sys.argv[2].split(","):
        print("CASE %s" % _name, flush=True)
        try:
            run_case(case(sys.argv[1], _name), sys.argv[1], sys.argv[3] or None)
        except Exception:
            traceback.print_exc(file=sys.stdout)
            print("FAILED case %s" % _name, flush=True)
            failed += 1
    sys.exit(1 if failed else 0)
