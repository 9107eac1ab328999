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


def all_pairs(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


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
    regrow (at least that many), long (row-block pairs))"""
    c = {"pairs": None, "env": {}, "mega": None, "batches": 1, "regrow": 0}
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
    else:
        raise KeyError(name)
    return c


CASES = ["tiny_n2", "tiny_1_1_2", "bin_edges", "bin_edges_reversed", "chaining", "no_chain", "row_blocks", "batches", "regrowth", "mega"]

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


def check_case(name, lib_path=None):
    c = case(name)
    n = len(c["seqs"])
    pairs = c["pairs"] or all_pairs(n)
    want = np.array([w["ea"] for w in oracle(name)], np.float32)
    g = context(c, lib_path)
    try:
        g.timers_reset()
        s1, s2 = (None, None) if c["pairs"] is None else ([x for x, _ in pairs], [y for _, y in pairs])
        got = A.with_env(c["env"], lambda: g.ea_scores(s1, s2))
        info = g.ea_info()
        timers = g.timers_get()
    finally:
        g.close()
    print(name, "ea", got[:6], "info", info, "fb launches", timers["fb"][1], "post launches", timers["post"][1])
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert len(bad) == 0, (name, "against the oracle", bad[:10], got[bad[:10]], want[bad[:10]])
    # ... and the stage's own EA: all pairs on a second context, read at the InitPairs number of every pair of the list
    g2 = context(c, lib_path, registry=False)
    try:
        g2.calc_posteriors()
        stage = g2.get_ea().copy()
    finally:
        g2.close()
    num = {p: k for k, p in enumerate(all_pairs(n))}
    ref2 = stage[[num[p] for p in pairs]]
    bad = np.nonzero(bits(got) != bits(ref2))[0]
    assert len(bad) == 0, (name, "against calc_posteriors + get_ea", bad[:10], got[bad[:10]], ref2[bad[:10]])
    # ---- the route
    assert info[0] == len(pairs), info
    assert info[1] == c["batches"], info
    assert info[2] >= c["regrow"] and (c["regrow"] or info[2] == 0), info
    assert info[3] == info[1] + info[2], info
    assert timers["post"][1] == info[3], (timers, info)
    if c["batches"] == 1 and not c["regrow"]:
        assert timers["fb"][1] == fb_launches(c), (timers, fb_launches(c))
    else:
        assert timers["fb"][1] >= info[3], (timers, info)
    if name == "bin_edges_reversed":  # pair by pair what the all-pairs call gave
        assert np.array_equal(bits(got[::-1]), bits(np.array([w["ea"] for w in oracle("bin_edges")], np.float32)))


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
