"""post_wide_ea_kernel (muscle_amd/csrc/kernels_postwea.h: the EA of a pair with a workgroup per pair) through mpcgpu_ea_scores under
MPCGPU_EA_WIDE=1 — shared by tests/test_ea_wide_table.py (the inputs are what the table claims, on the CPU), tests/test_emu_ea_wide.py
(the emulator build) and tests/test_gpu_ea_wide.py (the device).

mpcgpu_ea_scores splits its list (muscle_amd/csrc/mpcgpu_ea.inc): a pair whose longer sequence has at least MPCGPU_EA_WIDE_MIN positions
(unset: wide_min_default(), 12 115) is WIDE and finishes in post_wide_ea_kernel, the others in post_ea_kernel; the narrow sub-list runs
first, each sub-list has its own geometry, batches and candidate room, and the floats go back into the caller's order.

Every numeric case compares ea_scores at 0 ulp with the CPU oracle's EA of every pair (AlignPairFlat on the oracle, tests/_align_pairs.py)
and, where the all-pairs stage of the case's sequences is affordable (`stage`: no long sequences, every pair x < y), with
mpcgpu_calc_posteriors + mpcgpu_get_ea on a SECOND context. Every case states its route and the checker asserts it from ea_info,
ea_wide_info and the launch counter of the "post" family. No list holds a pair of two long sequences: a long sequence meets partners of
11 to 70 positions, a few hundred thousand DP cells on the oracle. TEST INFRASTRUCTURE."""
import functools
import os

import numpy as np

import _align_pairs as A
import _ea
import _oracle as O
from muscle_amd._lib import MpcGpuError
from muscle_amd.synth import make_family

POST_ROWS_LDS = A.POST_ROWS_LDS
SORT_CAP = A.POST_SORT_CAP
WIDE = {"MPCGPU_EA_WIDE": "1"}


def post_rows_fits(LX, LY, sort_cap=SORT_CAP):
    """mpcgpu_stage_a.inc: post_rows_fits()"""
    return (LX + 2 + 2 * (LY + 2)) * 4 + 8 + 8 * sort_cap <= POST_ROWS_LDS


def wide_min_default(sort_cap=SORT_CAP):
    """mpcgpu_ea.inc: ea_wide_min_default() — the smallest m for which post_rows_fits(m, m, sort_cap) is false"""
    m = 1
    while post_rows_fits(m, m, sort_cap):
        m += 1
    return m


def forced(wide_min, **more):
    env = dict(WIDE, MPCGPU_EA_WIDE_MIN=str(wide_min))
    env.update(more)
    return env


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(seqs, pairs: list of (x, y) or None for all pairs, env, mega, stage: the second context's all-pairs stage is affordable,
    batches: "one" (a batch per sub-list) or "each" (a batch per pair))"""
    c = {"pairs": None, "env": dict(WIDE), "mega": None, "stage": True, "batches": "one"}
    if name == "edge":  # 12 114 stays narrow, 12 115 goes wide: once as the column (11 x 12 115), once as the row (12 115 x 40)
        c["seqs"] = A.related([12114, 12115, 11, 40], 51)
        c["pairs"] = [(2, 0), (2, 1), (0, 3), (1, 3)]
        c["stage"] = False
    elif name == "long_keys":  # 16 + 16 bits of the row-block key, 22 + 4 bits of the short one: four radix passes each
        c["seqs"] = A.related([40000, 11], 52)
        c["pairs"] = [(0, 1), (1, 0)]
        c["stage"] = False
    elif name in ("lds_forced", "lds_forced_0", "lds_forced_64"):  # pairs around 100 x 60 wide, 40 x 45 narrow
        c["seqs"] = A.related([100, 60, 97, 63, 40, 45], 53)
        c["pairs"] = [(0, 1), (2, 3), (4, 5), (0, 3), (1, 2), (3, 5)]
        c["env"] = forced(50)
        if name != "lds_forced":
            c["env"]["MPCGPU_POSTW_LDS"] = name.split("_")[-1]
    elif name == "regrowth":  # poly-A 60 x 100 keeps 1627 cells, more than the first room of 1200 (tests/_ea.py)
        c["seqs"] = _ea.case("regrowth")["seqs"]
        c["env"] = forced(1)
    elif name in ("batches", "batches_reversed"):  # one pair per batch; the median length splits the list into both sub-lists
        c["seqs"] = make_family(12, 60, seed=44)
        c["env"] = forced(sorted(len(s) for s in c["seqs"])[6], MPCGPU_SCRATCH_GB="0")
        c["batches"] = "each"
        if name == "batches_reversed":
            c["pairs"] = _ea.all_pairs(12)[::-1]
            c["stage"] = False  # (y, x) lists are not what the all-pairs stage holds; "batches" has the second reference
    elif name == "mega":
        m = _ea.mega5()
        c["seqs"], c["mega"] = m["seqs"], m
        c["env"] = forced(1)
    elif name == "persistent":  # 561 pairs in one batch: more than the 256 CUs x 2 workgroups of 1024 threads a device keeps resident
        c["seqs"] = make_family(34, 30, seed=54)
        c["env"] = forced(1)
    elif name == "tiny":  # 1 x 1, 1 x 2, 1 x 2
        c["seqs"] = ["W", "P", "WP"]
        c["env"] = forced(1)
    else:
        raise KeyError(name)
    return c


CASES_FORCED = ["lds_forced", "lds_forced_0", "lds_forced_64", "regrowth", "batches", "batches_reversed", "mega", "persistent", "tiny"]
CASES = ["edge", "long_keys"] + CASES_FORCED

_MEMO = {}


def pairs_of(c):
    return c["pairs"] or _ea.all_pairs(len(c["seqs"]))


def lens_of(c):
    return [(len(c["seqs"][x]), len(c["seqs"][y])) for x, y in pairs_of(c)]


def wide_min_of(c):
    return int(c["env"].get("MPCGPU_EA_WIDE_MIN", wide_min_default()))


def is_wide(c):
    """per pair of the list: does it go to post_wide_ea_kernel"""
    m = wide_min_of(c)
    return [max(a, b) >= m for a, b in lens_of(c)]


def oracle(name):
    """the oracle's AlignPairFlat of every pair of the case, in list order, computed once per distinct pair"""
    c = case(name)
    seqs, m = c["seqs"], c["mega"]
    out = []
    for x, y in pairs_of(c):
        key = (seqs[x], seqs[y], None if m is None else (m["key"], x, y))
        if key not in _MEMO:
            _MEMO[key] = A.ap_oracle(A.hmm()[0], seqs[x].encode(), seqs[y].encode(), None if m is None else (m["g"], m["profs"][x], m["profs"][y]), path=False)
        out.append(_MEMO[key])
    return out


def route(name):
    """-> (ea_info, ea_wide_info) the case must report: each sub-list is one batch, or a batch per pair under MPCGPU_SCRATCH_GB=0, and
    a batch is redone while the longest candidate list of the SUB-LIST overflows its room (the room of a sub-list follows its own
    longest sequence; with a batch per pair only the batches that hold such a list are redone)"""
    c = case(name)
    lens, wide, cand = lens_of(c), is_wide(c), [w["cand"] for w in oracle(name)]
    tot = []
    for flag in (False, True):
        sub = [k for k in range(len(lens)) if wide[k] == flag]
        if not sub:
            tot.append((0, 0, 0))
            continue
        sl, sc = [lens[k] for k in sub], [cand[k] for k in sub]
        if c["batches"] == "each":
            tot.append((len(sub), len(sub), A.regrowths_each(sl, sc, c["env"])))
        else:
            tot.append((len(sub), 1, A.regrowths(sl, sc, c["env"])))
    (pn, bn, rn), (pw, bw, rw) = tot
    return (pn + pw, bn + bw, rn + rw, bn + bw + rn + rw), (pw, bw, rw, bw + rw)


def run(c, lib_path=None, env=None):
    """ea_scores of the case's list under env (default: the case's) -> (floats, ea_info, ea_wide_info, timers)"""
    pairs = pairs_of(c)
    g = _ea.context(c, lib_path)
    try:
        g.timers_reset()
        s1, s2 = (None, None) if c["pairs"] is None else ([x for x, _ in pairs], [y for _, y in pairs])
        got = A.with_env(c["env"] if env is None else env, lambda: g.ea_scores(s1, s2))
        return got, g.ea_info(), g.ea_wide_info(), g.timers_get()
    finally:
        g.close()


def without(names):
    """the variables unset for the length of a call (a case that needs the library's defaults must not inherit the caller's)"""
    return {k: os.environ.pop(k) for k in names if k in os.environ}


def check_case(name, lib_path=None):
    c = case(name)
    n = len(c["seqs"])
    pairs = pairs_of(c)
    want = np.array([w["ea"] for w in oracle(name)], np.float32)
    got, info, winfo, timers = run(c, lib_path)
    print(name, "ea", got[:6], "info", info, "wide", winfo, "fb launches", timers["fb"][1], "post launches", timers["post"][1])
    bad = np.nonzero(_ea.bits(got) != _ea.bits(want))[0]
    assert len(bad) == 0, (name, "against the oracle", bad[:10], got[bad[:10]], want[bad[:10]])
    if c["stage"]:  # the stage's own EA: all pairs on a second context, read at the InitPairs number of every pair of the list
        g2 = _ea.context(c, lib_path, registry=False)
        try:
            g2.calc_posteriors()
            stage = g2.get_ea().copy()
        finally:
            g2.close()
        num = {p: k for k, p in enumerate(_ea.all_pairs(n))}
        ref2 = stage[[num[p] for p in pairs]]
        bad = np.nonzero(_ea.bits(got) != _ea.bits(ref2))[0]
        assert len(bad) == 0, (name, "against calc_posteriors + get_ea", bad[:10], got[bad[:10]], ref2[bad[:10]])
    # ---- the route
    want_info, want_wide = route(name)
    assert info == want_info and winfo == want_wide, (name, info, want_info, winfo, want_wide)
    assert winfo[0] == sum(is_wide(c)) > 0, (name, winfo)
    assert info[3] == info[1] + info[2] and winfo[3] == winfo[1] + winfo[2], (info, winfo)
    assert timers["post"][1] == info[3], (timers, info)
    assert timers["fb"][1] >= info[3], (timers, info)
    if name == "regrowth":
        assert winfo[2] >= 1, winfo
    if name == "batches_reversed":  # pair by pair what the list in InitPairs order gave
        assert np.array_equal(_ea.bits(got[::-1]), _ea.bits(np.array([w["ea"] for w in oracle("batches")], np.float32)))
    if name.startswith("lds_forced") or name == "mega":  # the same list by the row-list route: MPCGPU_EA_WIDE unset
        env = {k: v for k, v in c["env"].items() if not k.startswith("MPCGPU_EA_WIDE")}
        old = without(["MPCGPU_EA_WIDE", "MPCGPU_EA_WIDE_MIN"])
        try:
            rows, rinfo, rwide, _ = run(c, lib_path, env)
        finally:
            os.environ.update(old)
        assert rwide == (0, 0, 0, 0) and rinfo[0] == len(pairs), (rinfo, rwide)
        assert np.array_equal(_ea.bits(got), _ea.bits(rows)), (name, got, rows)


def check_inert(lib_path=None):
    """mpcgpu_ea_scores with wide pairs beside a store: the epoch stays, and mpcgpu_align_alns on the store gives the bytes it gave
    before (the first half of tests/_ea.py: check_inert, every pair forced wide, then a list that splits)"""
    seqs = make_family(6, 50, seed=46)
    g = _ea.context({"seqs": seqs, "mega": None}, lib_path, registry=False)
    try:
        def join():
            maps = [np.arange(len(s), dtype=np.uint32) for s in seqs]
            C = max(len(s) for s in seqs)
            return g.align_alns([0, 1, 2], [3, 4, 5], maps[:3], maps[3:], C, C)
        g.calc_posteriors()
        g.build_store()
        epoch, before = g.store_epoch(), join()
        ea_all = g.get_ea().copy()
        num = {p: k for k, p in enumerate(_ea.all_pairs(6))}
        got = A.with_env(forced(1), lambda: g.ea_scores([4, 0, 2], [5, 3, 3]))
        assert g.ea_wide_info() == (3, 1, 0, 1) and g.ea_info() == (3, 1, 0, 1)
        assert g.store_epoch() == epoch
        assert np.array_equal(_ea.bits(got), _ea.bits(ea_all[[num[(4, 5)], num[(0, 3)], num[(2, 3)]]]))
        split = sorted(len(s) for s in seqs)[3]
        nwide = sum(max(len(seqs[x]), len(seqs[y])) >= split for x, y in _ea.all_pairs(6))
        assert 0 < nwide <= 15
        got = A.with_env(forced(split), lambda: g.ea_scores())
        assert g.ea_wide_info()[0] == nwide and g.ea_info()[0] == 15
        assert np.array_equal(_ea.bits(got), _ea.bits(ea_all))
        assert g.store_epoch() == epoch
        assert join() == before
        assert np.array_equal(_ea.bits(g.get_ea()), _ea.bits(ea_all))
    finally:
        g.close()


def check_refusals(lib_path=None):
    """with MPCGPU_EA_WIDE=1 the envelope of a dense posterior is still refused by name before any device work (the launch counters of
    both families stay 0), the last call's reports stay, and a valid call succeeds afterwards"""
    seqs = ["MKVLAAGIVGL", "MKVLSAGIVAL", "A" * 25000, "C" * 25000]
    g = _ea.context({"seqs": seqs, "mega": None}, lib_path)
    want = A.ap_oracle(A.hmm()[0], seqs[0].encode(), seqs[1].encode(), None, path=False)["ea"]

    def body():
        for fn, words in ((lambda: g.ea_scores([0, 2], [1, 3]), ("mpcgpu_ea_scores", "LX=25000", "LY=25000", "INT_MAX")),
                          (lambda: g.ea_scores(), ("mpcgpu_ea_scores", "INT_MAX"))):
            got = g.ea_scores([0], [1])
            assert _ea.bits(got)[0] == _ea.bits(want) and g.ea_info() == (1, 1, 0, 1) and g.ea_wide_info() == (1, 1, 0, 1)
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
            assert g.ea_info() == (1, 1, 0, 1) and g.ea_wide_info() == (1, 1, 0, 1)
    try:
        A.with_env(forced(1), body)
    finally:
        g.close()



# ---- the drop-in: `muscle_gpu -super5` on consensus sequences beyond the row-list arrays -------------------------------------------
DROPIN_NAME = "super5_wide_4x12200"
DROPIN_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ea_wide_md5.json")
DROPIN_CLUSTERS = 4  # what the reference's UCLUST makes of the input (see dropin_input)


def dropin_input():
    """four sequences of 12 200 positions: two near-identical pairs (a handful of substitutions, no gaps) from two unrelated
    ancestors. At this length the reference's own EA of even such a pair is far below UCLUST's thresholds (0.99, then 0.7: in
    float32 the posteriors of a 12 200 x 12 200 pair fall under the sparse threshold along most of the path), so -super5 leaves
    every sequence a cluster of its own and CalcEADistMx sees all SIX pairs of four consensus sequences of 12 200 positions — every
    one of them beyond the row-list arrays."""
    kw = {"p_del": 0.0, "p_ins": 0.0, "p_sub": 0.0005}
    a, b = make_family(2, 12200, seed=61, **kw), make_family(2, 12200, seed=62, **kw)
    seqs = [a[0], b[0], a[1], b[1]]
    assert len(set(seqs)) == 4 and all(len(s) == 12200 for s in seqs)
    return seqs
