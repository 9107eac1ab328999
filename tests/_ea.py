"""post_ea_kernel (muscle_amd/csrc/kernels_postea.h: the EA of a list of pairs and nothing else, what CalcEADistMx keeps of AlignPairFlat)
through mpcgpu_ea_scores — shared by tests/test_ea_table.py (the inputs are what the table claims, on the CPU), tests/test_emu_ea.py
(the emulator build) and tests/test_gpu_ea.py (the device).

Every case compares ea_scores at 0 ulp with two things: the CPU oracle's EA of every pair (AlignPairFlat on the oracle, tests/_align_pairs.py)
and mpcgpu_calc_posteriors + mpcgpu_get_ea of the same sequences on a SECOND context. Every case states its route and the checker
asserts it: pairs, batches, regrowths and finishing launches from ea_info, the finishing launches again in the "post" family of
mpcgpu_timers_get (the kernel's time is attributed), and the launches of the forward/backward family where the rule fixes them — one per
rows-per-lane bin of a batch plus one for its row-block pairs (mpcgpu_stage_a.inc: every pair below 769 rows goes to the chain kernel
of its bin, or with structure profiles to fb_kernel of its bin).

A note on "tiny": under the amino-acid tables a 1 x 1 pair always keeps its one cell (P = 1) and no pair of lengths 1, 1, 2 has an empty
candidate list (test_ea_table asserts what the lists do hold: 1, 2 and 1 candidates, min(L1, L2) = 1).

The paths of post_ea_kernel and ea_sublist beyond the first pair of a workgroup and the first batch of a list (what each input is, is
proved on the CPU in tests/test_ea_table.py from the oracle's candidate and row counts and the host formulas restated here):
  persistent, persistent_small             561 pairs in one batch, the last sequence long (9800 / 600 positions) and a column only: with
                                           smem above 76 KB the launcher's grid is at most one workgroup per CU, so on 256 CUs every
                                           workgroup finishes two or three pairs — long then short and short then long both occur
                                           (test_gpu_ea asserts B > CUs * (152 KB // smem) with the device's CU count). The emulator
                                           (2 CUs) runs the _small forms; the full ones take 30 .. 110 s there
  persistent_overflow(_small)              the same list with a poly-A pair at position 10 that overflows the first room (one candidate
                                           per position of the long sequence): its workgroup reports it and goes on with good pairs
  sort_cap_8, sort_cap_mixed,              MPCGPU_POST_SORT_CAP below every list (chaining's), at the count of bin_edges' middle list
    persistent_sort_mixed(_small)          (11 lists in LDS, one of exactly the cap, 10 in the slot), and at the middle count of the
                                           persistent list: one workgroup alternates between LDS and its slot of sort_scratch
  post_batch_1, post_batch_3 (+ _polya)    MPCGPU_POST_BATCH on bin_edges' and regrowth's sequences: rows of more than `batch` cells,
                                           for 3 also rows of exactly 3, of a multiple of 3 and of none; the floats again at the default
  row_over_64                              no variable: "A" * 78 x "A" * 141 has a row of 65 cells (the smallest LX * LY found among the
                                           poly-A pairs of 40 .. 130 x LX .. 200 positions); run again in three passes of 32
  batches_regrowth (+ _reversed, _twice)   a pair per batch (MPCGPU_SCRATCH_GB=0), the overflowing poly-A pair in the middle of the
                                           list: the next batch's sweeps are queued when the overflow is found. _twice: 1627 and then
                                           3318 candidates against a first room of 1024 — two doublings, three if the room fell back
TEST INFRASTRUCTURE."""
import functools
import os

import numpy as np

import _align_pairs as A
import _golden as G
import _oracle as O
from muscle_amd._lib import MpcGpu, MpcGpuError
from muscle_amd.synth import make_family

LONG_MIN = A.LONG_MIN  # 769: row sequences from here on take the row-block sweeps
BIN_EDGE_LENS = [63, 64, 65, 128, 129, 512, 513]
INT_MAX = 2 ** 31 - 1
# "persistent": 33 sequences of 20 .. 45 positions and, LAST, one of 9800 — all pairs are 561 pairs in one batch, and (i, 33), the last
# pair of every row i of the all-pairs order, has the long sequence as its column: list positions 32, 64, 95, ... 560
PERSIST_N, PERSIST_LONG, PERSIST_LONG_SMALL = 34, 9800, 600
PERSIST_SORT_CAP = 53     # the candidate count of the middle pair of "persistent" by that count (test_ea_table: 285 lists up to it, 276 beyond)
PERSIST_SORT_CAP_SMALL = 57  # ... of "persistent_small"
MIXED_SORT_CAP = 160      # ... of "bin_edges" (11 lists up to it, 10 beyond)
OVERFLOW_POLYA, OVERFLOW_POLYA_SMALL = (300, 400), (60, 100)  # 11 860 candidates against a first room of 9800; 1627 against 1024
OVERFLOW_AT = 10          # list position of the overflowing pair: its workgroup goes on with positions 10 + grid, 10 + 2 grid, ...
ROW_OVER_64 = (78, 141)   # smallest LX * LY among the poly-A pairs up to 400 x 400 whose posterior has a row of more than 64 cells
BATCHES_REGROW = {"batches_regrowth": 1, "batches_regrowth_reversed": 1, "batches_regrowth_twice": 2}
POST_EA_LDS_PER_CU = 152 * 1024  # mpcgpu_ea.inc: launch_post_ea()  pocc <= 152 KB / smem


def all_pairs(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def persistent_seqs(long_len):
    lens = [20 + (7 * k) % 26 for k in range(PERSIST_N - 1)] + [long_len]
    return A.related(lens, 54)


def pairs_of(c):
    return c["pairs"] or all_pairs(len(c["seqs"]))


def lens_of(c):
    return [(len(c["seqs"][x]), len(c["seqs"][y])) for x, y in pairs_of(c)]


def post_ea_smem(lens, env):
    """mpcgpu_ea.inc: launch_post_ea() — the LDS of a workgroup of post_ea_kernel: the three arrays per position
    (mpcgpu_stage_a.inc: post_rows_fixed_lds()) and the sorted list of min(capc, MPCGPU_POST_SORT_CAP) entries, cut to 150 KB
    (capc is at least 1024, and a forced cap below it is what the minimum takes)"""
    LXm, LYm = max(a for a, _ in lens), max(b for _, b in lens)
    fixed = ((LXm + 2 + 2 * (LYm + 2)) * 4 + 7) & ~7
    cap = min(A.capc_of(lens, env), max(A.env_int(env, "MPCGPU_POST_SORT_CAP", A.POST_SORT_CAP), 2))
    if fixed + cap * 8 > A.POST_ROWS_LDS:
        cap = (A.POST_ROWS_LDS - fixed) // 8
    return fixed + cap * 8, cap


def grid_bound(c, cus):
    """the largest grid launch_post_ea gives the case's (one) batch on a device of `cus` CUs: min(B, CUs * pocc), pocc <= 152 KB / smem"""
    lens = lens_of(c)
    return min(len(lens), cus * max(POST_EA_LDS_PER_CU // post_ea_smem(lens, c["env"])[0], 1))


def expected_regrowths(name):
    """what ea_info must report as regrowths: the restated host formula on the oracle's candidate counts"""
    c = case(name)
    cand = [w["cand"] for w in oracle(name)]
    return (A.regrowths_each if c["each"] else A.regrowths)(lens_of(c), cand, c["env"])


@functools.lru_cache(maxsize=None)
def mega5():
    """the profiles of the committed bb11001.mega, at most the first 5 — the file holds 4 (tests/golden/mega_bb11001.npz is the parsed file)"""
    m = G.mega("mega_bb11001")
    out = {"seqs": m["seqs"][:5], "alpha": m["alpha"], "weight": m["weight"], "lp": m["lp"], "mx": m["mx"], "profs": m["profs"][:5],
           "key": "bb11001[:5]"}
    out["g"] = O.make_mega(m["alpha"], m["weight"], m["lp"], m["mx"])
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(seqs, pairs: list of (x, y) or None for all pairs, env, mega, and what the route must be: batches (None: one),
    regrow (at least that many), long (row-block pairs); each: a pair per batch, exact: regrow is the number the restated host
    formula gives and ea_info must report exactly it, same_as: the case whose oracle floats, in its list order, this list must
    repeat, rerun: an environment under which the same list is run once more and must give the same floats)"""
    c = {"pairs": None, "env": {}, "mega": None, "batches": 1, "regrow": 0, "each": False, "exact": False, "same_as": None, "rerun": None}
    if name == "tiny_n2":
        c["seqs"] = ["MKV", "MRVL"]
    elif name == "tiny_1_1_2":  # min(L1, L2) = 1
        c["seqs"] = ["W", "P", "WP"]
    elif name in ("bin_edges", "bin_edges_reversed"):
        c["seqs"] = A.related(BIN_EDGE_LENS, 41)
        if name == "bin_edges_reversed":
            c["pairs"] = all_pairs(len(BIN_EDGE_LENS))[::-1]
    elif name == "chaining":  # row 0 against 1 .. 5: one chain
        c["seqs"] = A.related([70, 66, 71, 69, 75, 68], 42)
        c["pairs"] = [(0, k) for k in range(1, 6)]
    elif name == "no_chain":  # each sequence once: no two pairs share a row
        c["seqs"] = A.related([70, 66, 71, 69, 75, 68], 42)
        c["pairs"] = [(0, 1), (2, 3), (4, 5)]
    elif name == "row_blocks":  # one row-block pair, 769 x 70, beside short pairs
        c["seqs"] = A.related([769, 70, 40, 50], 43)
        c["pairs"] = [(1, 2), (0, 1), (2, 3), (1, 3)]
    elif name == "batches":  # one pair per batch: 66 batches
        c["seqs"] = make_family(12, 60, seed=44)
        c["env"] = {"MPCGPU_SCRATCH_GB": "0"}
        c["batches"] = 66
    elif name == "regrowth":  # poly-A 60 x 100 keeps 1627 cells, more than the first room of 1200
        c["seqs"] = ["A" * 60, "A" * 100] + A.related([80], 45)
        c["regrow"] = 1
    elif name == "mega":
        m = mega5()
        c["seqs"], c["mega"] = m["seqs"], m
    # ---- the persistent loop: more pairs in one batch than workgroups fit the device, of different shapes
    elif name in ("persistent", "persistent_sort_mixed", "persistent_small", "persistent_sort_mixed_small"):
        small = name.endswith("_small")
        c["seqs"] = persistent_seqs(PERSIST_LONG_SMALL if small else PERSIST_LONG)
        c["exact"] = True
        if "sort_mixed" in name:  # one workgroup alternates between the LDS list and its scratch slot
            c["env"] = {"MPCGPU_POST_SORT_CAP": str(PERSIST_SORT_CAP_SMALL if small else PERSIST_SORT_CAP)}
            c["same_as"] = "persistent_small" if small else "persistent"
    elif name in ("persistent_overflow", "persistent_overflow_small"):  # the poly-A pair overflows, its workgroup goes on
        small = name.endswith("_small")
        c["seqs"] = persistent_seqs(PERSIST_LONG_SMALL if small else PERSIST_LONG) + ["A" * a for a in (OVERFLOW_POLYA_SMALL if small else OVERFLOW_POLYA)]
        c["pairs"] = all_pairs(PERSIST_N)
        c["pairs"].insert(OVERFLOW_AT, (PERSIST_N, PERSIST_N + 1))
        c["env"] = {"MPCGPU_CAND_PER_ROW": "1"}  # a first room of one candidate per position of the long sequence (1024 at the least)
        c["regrow"], c["exact"] = 1, True
    # ---- the sorted list in LDS (c <= sort_cap) or in the workgroup's scratch slot
    elif name == "sort_cap_8":  # every list beyond the LDS entries
        c.update(case("chaining"), env={"MPCGPU_POST_SORT_CAP": "8"}, exact=True, same_as="chaining")
    elif name == "sort_cap_mixed":  # the cap is the candidate count of a middle pair: lists on both sides, and one of exactly the cap
        c.update(case("bin_edges"), env={"MPCGPU_POST_SORT_CAP": str(MIXED_SORT_CAP)}, exact=True, same_as="bin_edges")
    # ---- the multi-pass EA row (a row of more than `batch` cells) in the FULL = false instantiation
    elif name in ("post_batch_1", "post_batch_3"):
        c.update(case("bin_edges"), env={"MPCGPU_POST_BATCH": name[-1]}, exact=True, same_as="bin_edges", rerun={})
    elif name in ("post_batch_1_polya", "post_batch_3_polya"):
        c.update(case("regrowth"), env={"MPCGPU_POST_BATCH": name.split("_")[2]}, exact=True, same_as="regrowth", rerun={})
    elif name == "row_over_64":  # no variable: the smallest poly-A pair with a row of more than 64 candidates (65, in 78 x 141)
        c["seqs"] = ["A" * ROW_OVER_64[0], "A" * ROW_OVER_64[1]] + A.related([90], 48)
        c["regrow"], c["exact"] = 1, True
        c["rerun"] = {"MPCGPU_POST_BATCH": "32"}  # ... and the same floats with the row in three passes
    # ---- an overflow found while the next batch's sweeps are queued: a pair per batch, the poly-A pair(s) inside the list
    elif name in ("batches_regrowth", "batches_regrowth_reversed", "batches_regrowth_twice"):
        c["seqs"] = A.related([70, 66, 90, 85, 75], 49) + ["A" * 60, "A" * 100]
        c["pairs"] = [(0, 1), (2, 3), (1, 4), (5, 6), (0, 3), (2, 4), (1, 2)]
        c["env"] = {"MPCGPU_SCRATCH_GB": "0"}
        if name == "batches_regrowth_twice":  # 60 x 100 (1627 candidates), two batches on, 100 x 150 (3318): a first room of 1024 doubles twice
            c["seqs"] = c["seqs"] + ["A" * 150]
            c["pairs"] = [(0, 1), (2, 3), (5, 6), (1, 4), (0, 3), (6, 7), (2, 4), (1, 2)]
            c["env"]["MPCGPU_CAND_PER_ROW"] = "1"
        if name == "batches_regrowth_reversed":
            c["pairs"] = c["pairs"][::-1]
            c["same_as"] = "batches_regrowth"
        c["batches"], c["each"], c["exact"] = len(c["pairs"]), True, True
        c["regrow"] = BATCHES_REGROW[name]
    else:
        raise KeyError(name)
    return c


CASES_BASE = ["tiny_n2", "tiny_1_1_2", "bin_edges", "bin_edges_reversed", "chaining", "no_chain", "row_blocks", "batches", "regrowth", "mega"]
# the persistent loop, both sides of the sort cap, the multi-pass row, an overflow between batches
CASES_PATHS = ["persistent_small", "persistent_overflow_small", "persistent_sort_mixed_small", "sort_cap_8", "sort_cap_mixed", "post_batch_1", "post_batch_3",
               "post_batch_1_polya", "post_batch_3_polya", "row_over_64", "batches_regrowth", "batches_regrowth_reversed",
               "batches_regrowth_twice"]
CASES_DEVICE = ["persistent", "persistent_overflow", "persistent_sort_mixed"]  # sized for a device of up to 256 CUs
CASES = CASES_BASE + CASES_PATHS + CASES_DEVICE

_MEMO = {}


def oracle(name):
    """the oracle's AlignPairFlat of every pair of the case, in list order: [dict(ea, cand, ...)], computed once per distinct pair"""
    c = case(name)
    seqs, m = c["seqs"], c["mega"]
    out = []
    for x, y in (c["pairs"] or all_pairs(len(seqs))):
        key = (seqs[x], seqs[y], None if m is None else (m["key"], x, y))
        if key not in _MEMO:
            _MEMO[key] = A.ap_oracle(A.hmm()[0], seqs[x].encode(), seqs[y].encode(), None if m is None else (m["g"], m["profs"][x], m["profs"][y]), path=False)
        out.append(_MEMO[key])
    return out


def fb_launches(c):
    """launches of the forward/backward family of a one-batch call without regrowth: one per rows-per-lane bin, one for the row-block pairs"""
    seqs = c["seqs"]
    rows = [len(seqs[x]) for x, _ in (c["pairs"] or all_pairs(len(seqs)))]
    return len({(L + 63) // 64 for L in rows if L < LONG_MIN}) + (1 if any(L >= LONG_MIN for L in rows) else 0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def context(c, lib_path=None, registry=True):
    s, t, m, i, thr = G.hmm_tables()
    g = MpcGpu(0, lib_path)
    g.set_hmm(s, t, m, i, thr)
    (g.set_seqs_registry if registry else g.set_seqs)(c["seqs"])
    if c["mega"] is not None:
        mg = c["mega"]
        g.set_mega(mg["alpha"], mg["weight"], mg["lp"], mg["mx"], mg["profs"])
    return g


_STAGE = {}


def stage_ea(c, lib_path=None):
    """mpcgpu_calc_posteriors + mpcgpu_get_ea of the case's sequences on a context of its own (never the one ea_scores ran on), under
    no variable of the case: all pairs in InitPairs order, computed once per library and registry"""
    m = c["mega"]
    key = (lib_path, tuple(c["seqs"]), None if m is None else m["key"])
    if key not in _STAGE:
        g2 = context(c, lib_path, registry=False)
        try:
            g2.calc_posteriors()
            _STAGE[key] = g2.get_ea().copy()
        finally:
            g2.close()
        _STAGE[key].setflags(write=False)
    return _STAGE[key]


def run(c, lib_path=None, env=None):
    """ea_scores of the case's list under env (default: the case's) -> (floats, ea_info, timers)"""
    pairs = pairs_of(c)
    g = context(c, lib_path)
    try:
        g.timers_reset()
        s1, s2 = (None, None) if c["pairs"] is None else ([x for x, _ in pairs], [y for _, y in pairs])
        got = A.with_env(c["env"] if env is None else env, lambda: g.ea_scores(s1, s2))
        return got, g.ea_info(), g.timers_get()
    finally:
        g.close()


def check_case(name, lib_path=None):
    c = case(name)
    n = len(c["seqs"])
    pairs = pairs_of(c)
    want = np.array([w["ea"] for w in oracle(name)], np.float32)
    got, info, timers = run(c, lib_path)
    print(name, "ea", got[:6], "info", info, "fb launches", timers["fb"][1], "post launches", timers["post"][1])
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert len(bad) == 0, (name, "against the oracle", bad[:10], got[bad[:10]], want[bad[:10]])
    # ... and the stage's own EA: all pairs on a second context, read at the InitPairs number of every pair of the list
    stage = stage_ea(c, lib_path)
    num = {p: k for k, p in enumerate(all_pairs(n))}
    ref2 = stage[[num[p] for p in pairs]]
    bad = np.nonzero(bits(got) != bits(ref2))[0]
    assert len(bad) == 0, (name, "against calc_posteriors + get_ea", bad[:10], got[bad[:10]], ref2[bad[:10]])
    # ---- the route
    assert info[0] == len(pairs), info
    assert info[1] == c["batches"], info
    assert info[2] >= c["regrow"] and (c["regrow"] or info[2] == 0), info
    if c["exact"]:
        assert info[2] == c["regrow"] == expected_regrowths(name), (info, c["regrow"], expected_regrowths(name))
    assert info[3] == info[1] + info[2], info
    assert timers["post"][1] == info[3], (timers, info)
    if c["batches"] == 1 and not c["regrow"]:
        assert timers["fb"][1] == fb_launches(c), (timers, fb_launches(c))
    else:
        assert timers["fb"][1] >= info[3], (timers, info)
    if name == "bin_edges_reversed":  # pair by pair what the all-pairs call gave
        assert np.array_equal(bits(got[::-1]), bits(np.array([w["ea"] for w in oracle("bin_edges")], np.float32)))
    if c["same_as"]:  # float for float what the other case's list gives (the reversed list: its floats reversed)
        other = np.array([w["ea"] for w in oracle(c["same_as"])], np.float32)
        assert np.array_equal(bits(got[::-1] if name.endswith("_reversed") else got), bits(other)), (name, c["same_as"])
    if c["rerun"] is not None:  # the same list under the other environment (unset: the default batch of 64 cells)
        assert all(k not in os.environ for k in c["env"]), "the caller's environment forces what the case leaves to the default"
        again, ainfo, _ = run(c, lib_path, c["rerun"])
        assert ainfo[:3] == info[:3], (ainfo, info)
        assert np.array_equal(bits(got), bits(again)), (name, c["rerun"], got, again)


def check_inert(lib_path=None):
    """mpcgpu_ea_scores beside a store: the epoch stays, and mpcgpu_align_alns on the store gives the bytes it gave before. A registry
    of its own on the store's context would itself drop the store (mpcgpu_set_seqs_registry moves the epoch by its contract), so the
    check has two halves: (a) the call on the store's context, with another pair list than the store's — epoch equal across it, the
    join equal after it; (b) the call on ANOTHER registry — epoch equal across the call — then the first registry and its store put
    back, and the join again."""
    seqs = make_family(6, 50, seed=46)
    other = A.related([33, 90, 41, 64], 47)
    c = {"seqs": seqs, "mega": None}
    g = context(c, lib_path, registry=False)
    try:
        def join():
            maps = [np.arange(len(s), dtype=np.uint32) for s in seqs]
            C = max(len(s) for s in seqs)
            return g.align_alns([0, 1, 2], [3, 4, 5], maps[:3], maps[3:], C, C)
        g.calc_posteriors()
        g.build_store()
        epoch, before = g.store_epoch(), join()
        ea_all = g.get_ea().copy()
        got = g.ea_scores([4, 0, 2], [5, 3, 3])
        assert g.store_epoch() == epoch
        num = {p: k for k, p in enumerate(all_pairs(6))}
        assert np.array_equal(bits(got), bits(ea_all[[num[(4, 5)], num[(0, 3)], num[(2, 3)]]]))
        assert np.array_equal(bits(g.ea_scores()), bits(ea_all))
        assert g.store_epoch() == epoch
        assert join() == before
        assert np.array_equal(bits(g.get_ea()), bits(ea_all))
        # (b)
        g.set_seqs_registry(other)
        e1 = g.store_epoch()
        got = g.ea_scores()
        assert g.store_epoch() == e1 and g.ea_info()[0] == 6
        h = A.hmm()[0]
        want = np.array([A.ap_oracle(h, other[x].encode(), other[y].encode(), None, path=False)["ea"] for x, y in all_pairs(4)], np.float32)
        assert np.array_equal(bits(got), bits(want))
        g.set_seqs(seqs)
        g.calc_posteriors()
        g.build_store()
        assert join() == before
    finally:
        g.close()


def check_refusals(lib_path=None):
    """refused by name, before any device work (the launch counters of both families stay 0), and a valid call succeeds after each"""
    seqs = ["MKVLAAGIVGL", "MKVLSAGIVAL", "A" * 25000, "C" * 25000]
    assert 25000 * 25000 * 5 + 100 > INT_MAX
    g = context({"seqs": seqs, "mega": None}, lib_path)
    want = A.ap_oracle(A.hmm()[0], seqs[0].encode(), seqs[1].encode(), None, path=False)["ea"]
    try:
        def refused(fn, *words):
            g.timers_reset()
            epoch = g.store_epoch()
            try:
                fn()
            except MpcGpuError as e:
                assert all(w in str(e) for w in words), str(e)
            else:
                raise AssertionError("accepted: %s" % (words,))
            t = g.timers_get()
            assert t["fb"][1] == 0 and t["post"][1] == 0, t
            assert g.store_epoch() == epoch
            got = g.ea_scores([0], [1])  # the context stays usable
            assert bits(got)[0] == bits(want), (got, want)
            assert g.ea_info() == (1, 1, 0, 1)
        L = g.L
        out = np.zeros(8, np.float32)
        refused(lambda: g._ck(L.mpcgpu_ea_scores(g.h, 5, None, None, out.ctypes.data)), "mpcgpu_ea_scores", "6 pairs", "not 5")
        refused(lambda: g.ea_scores([0, 4], [1, 1]), "mpcgpu_ea_scores", "out of range", "pair 1")
        refused(lambda: g.ea_scores([0, 1], [1, 4]), "mpcgpu_ea_scores", "out of range", "pair 1")
        refused(lambda: g.ea_scores([0, 2], [1, 3]), "mpcgpu_ea_scores", "LX=25000", "LY=25000", "INT_MAX")
        refused(lambda: g.ea_scores(), "mpcgpu_ea_scores", "INT_MAX")
        s1 = np.zeros(1, np.uint32)
        refused(lambda: g._ck(L.mpcgpu_ea_scores(g.h, 1, s1.ctypes.data, None, out.ctypes.data)), "mpcgpu_ea_scores", "both")
        refused(lambda: g.ea_scores([0], [2]), "mpcgpu_ea_scores", "LDS arrays", "25000")  # within INT_MAX, beyond the row-list arrays
    finally:
        g.close()
