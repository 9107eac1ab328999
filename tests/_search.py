"""mpcgpu_search_pairs (muscle_amd/csrc/mpcgpu_search.inc, kernels_search.h: the loop of UClust::Search, uclust.cpp:44-54, for a list of
queries) — shared by tests/test_gpu_search.py (the device) and tests/test_emu_search.py (the emulator build of the same sources).

Every case is checked twice, at 0 ulp: against the CPU oracle (AlignPairFlat on the oracle, tests/_align_pairs.py: EA of every pair, and
for every group the first candidate whose EA reaches min_ea with its path and score) and against mpcgpu_align_pairs of the same pairs on a
FRESH context. Every case states its route and the checker asserts it from mpcgpu_search_info: groups, pairs, chunks, chunks on the general
route — and out[2], the pairs whose dense posterior and trace-back ran, equals the number of accepted groups: an implementation that traces
every pair fails there.

A case's threshold is the EA of one of its own pairs (the oracle's bits), so both sides of the comparison EA >= min_ea occur, and the groups
are laid out from the pairs below ("lo") and at or above it ("hi"):
  sizes            groups of 0, 1, 2, 8, 9, 65 and 130 candidates: the hit at position 0, in the middle, last, absent; 65 with its only hit in
                   lane 0 of the second stride; 130 with hits at 100 and 129 (the lowest lane of the second stride wins) and at 3
  threshold        four candidates of rising EA: min_ea = the bits of the third (accepted: position 2), then nextafter above them (position 3)
  chunks           40 groups of 8 under MPCGPU_SEARCH_CHUNK=100: cuts inside group 12 (its hit before the cut: the rest enters the next chunk
                   with nothing to try), between groups 24 and 25, and inside group 37 (its hit behind the cut); the answers equal the uncut run's
  chunks_default   60 groups of 9 = 540 pairs: two chunks at the default size, the cut inside group 56
  row_block        a group whose row sequence has 800 positions (against 60): a row-block pair, so its chunk takes the general route
  overflow         the poly-A pair of tests/_ea.py's regrowth cases (60 x 100 keeps 1627 cells, the first room is 1200): the fused chunk overflows and
                   is run again on the general route
                   (pinned: against the same call under MPCGPU_SEARCH_FUSED=0 the launch counters hold one more finishing launch, one more
                   alignment launch and more forward/backward launches — the fused attempt ran and was thrown away)
  general_raw      ten groups under MPCGPU_SEARCH_FUSED=0 MPCGPU_POST_WIDE=1: the finishing kernel is post_wide_kernel (mpcgpu_post_info says),
                   so the picked pairs' matrices come from the raw candidate lists through dense_post_raw_pick_kernel
  general          the groups of "chunks" under MPCGPU_SEARCH_FUSED=0: every chunk on the general route, the same answers
  mega             the committed structure profiles tests/golden/mega_synth_6x40_s2.npz through mpcgpu_set_mega
TEST INFRASTRUCTURE."""
import ctypes
import functools

import numpy as np

import _align_pairs as A
import _ea as E
import _golden as G
import _oracle as O
from muscle_amd._lib import MpcGpu, MpcGpuError
from muscle_amd.synth import make_family

NONE = 0xffffffff
CASES = ["sizes", "threshold", "chunks", "chunks_default", "row_block", "overflow", "general", "general_raw", "mega"]
bits = A.bits


def pool_seqs(L, seed):
    """ten related sequences of 20 .. L positions and six unrelated ones: pairs on both sides of any threshold in between"""
    lens = [L - (3 * k) % (L // 3) for k in range(10)]
    return A.related(lens, seed) + [make_family(1, L - k, seed=seed + 100 + k)[0] for k in range(6)]


class Pool:
    """all ordered pairs of a registry with the oracle's EA, split at the median pair's EA"""

    def __init__(self, seqs, mega=None):
        self.seqs, self.mega = seqs, mega
        n = len(seqs)
        self.pairs = [(x, y) for x in range(n) for y in range(n) if x != y]
        self.ea = np.array([A.oracle_pair(seqs, x, y, mega)["ea"] for x, y in self.pairs], np.float32)
        order = np.argsort(self.ea, kind="stable")
        self.thr = np.float32(self.ea[order[len(order) // 2]])
        self.lo = [self.pairs[k] for k in order if not self.ea[k] >= self.thr]
        self.hi = [self.pairs[k] for k in order if self.ea[k] >= self.thr]
        assert len(self.lo) >= 8 and len(self.hi) >= 8
        self._l = self._h = 0

    def group(self, size, hits):
        """a group of `size` candidates with pairs at or above the threshold exactly at the positions `hits`"""
        out = []
        for t in range(size):
            if t in hits:
                out.append(self.hi[self._h % len(self.hi)])
                self._h += 1
            else:
                out.append(self.lo[self._l % len(self.lo)])
                self._l += 1
        return out


def chunk_groups(p):
    groups = []
    for g in range(40):
        hits = {12: (2,), 37: (6,), 24: (7,), 25: (0,)}.get(g, () if g % 5 == 4 else ((g * 3) % 8, 7))
        groups.append(p.group(8, hits))
    return groups


@functools.lru_cache(maxsize=None)
def case(name, size):
    """-> dict(seqs, mega, calls: [dict(groups, min_ea, env, chunks, general)])"""
    gpu = size == "gpu"
    c = {"mega": None}
    if name == "sizes":
        p = Pool(pool_seqs(60 if gpu else 28, 71))
        groups = [p.group(0, ()), p.group(1, (0,)), p.group(1, ()), p.group(2, (1,)), p.group(8, (0, 3, 5)), p.group(8, (3, 5)), p.group(8, (7,)),
                  p.group(8, ()), p.group(9, (8,)), p.group(65, (64,)), p.group(65, ()), p.group(130, (100, 129)), p.group(130, (3,)), p.group(0, ())]
        c.update(seqs=p.seqs, calls=[dict(groups=groups, min_ea=p.thr, env={}, chunks=1, general=0)])
    elif name == "threshold":
        p = Pool(pool_seqs(90 if gpu else 30, 72))
        k = np.argsort(p.ea, kind="stable")
        pick = [int(k[len(k) // 5]), int(k[2 * len(k) // 5]), int(k[3 * len(k) // 5]), int(k[4 * len(k) // 5])]
        e = p.ea[pick]
        assert e[0] < e[1] < e[2] < e[3]
        groups = [[p.pairs[q] for q in pick]]
        up = np.nextafter(e[2], np.float32(np.inf), dtype=np.float32)
        assert up <= e[3]
        c.update(seqs=p.seqs, calls=[dict(groups=groups, min_ea=e[2], env={}, chunks=1, general=0, accepted=[2]),
                                     dict(groups=groups, min_ea=up, env={}, chunks=1, general=0, accepted=[3])])
    elif name in ("chunks", "general"):
        p = Pool(pool_seqs(50 if gpu else 28, 73))
        groups = chunk_groups(p)
        if name == "chunks":
            c.update(seqs=p.seqs, calls=[dict(groups=groups, min_ea=p.thr, env={"MPCGPU_SEARCH_CHUNK": "100"}, chunks=4, general=0),
                                         dict(groups=groups, min_ea=p.thr, env={}, chunks=1, general=0)])
        else:
            c.update(seqs=p.seqs, calls=[dict(groups=groups, min_ea=p.thr, env={"MPCGPU_SEARCH_FUSED": "0", "MPCGPU_SEARCH_CHUNK": "100"}, chunks=4, general=4)])
    elif name == "chunks_default":
        p = Pool(pool_seqs(40 if gpu else 28, 74))
        groups = [p.group(9, {56: (8,), 55: (0,)}.get(g, () if g % 4 == 3 else (g % 9,))) for g in range(60)]
        c.update(seqs=p.seqs, calls=[dict(groups=groups, min_ea=p.thr, env={}, chunks=2, general=0)])
    elif name == "row_block":
        seqs = A.related([800, 60, 45, 70, 52], 75)
        e = [A.oracle_pair(seqs, x, y)["ea"] for x, y in [(0, 1), (2, 3), (4, 1)]]
        groups = [[(2, 3), (0, 1), (4, 1)], [(4, 1)], [(0, 1)]]
        c.update(seqs=seqs, calls=[dict(groups=groups, min_ea=np.float32(min(e[0], e[2])), env={}, chunks=1, general=1),
                                   dict(groups=[[(2, 3)], [(4, 1), (2, 3)]], min_ea=np.float32(e[1]), env={}, chunks=1, general=0)])
    elif name == "overflow":
        seqs = ["A" * 60, "A" * 100] + A.related([80], 45) + A.related([70, 66], 76)
        e = A.oracle_pair(seqs, 0, 1)["ea"]
        groups = [[(2, 0), (0, 1), (3, 4)], [(3, 4), (4, 3)], [(0, 1)]]
        c.update(seqs=seqs, calls=[dict(groups=groups, min_ea=np.float32(e), env={}, chunks=1, general=1),
                                   dict(groups=groups, min_ea=np.float32(e), env={"MPCGPU_SEARCH_FUSED": "0"}, chunks=1, general=1)])
    elif name == "general_raw":
        p = Pool(pool_seqs(50 if gpu else 28, 73))
        groups = chunk_groups(p)[:10]
        c.update(seqs=p.seqs, calls=[dict(groups=groups, min_ea=p.thr, env={"MPCGPU_SEARCH_FUSED": "0", "MPCGPU_POST_WIDE": "1"}, chunks=1, general=1, post_kernel=2)])
    elif name == "mega":
        m = G.mega("mega_synth_6x40_s2")
        m["g"] = O.make_mega(m["alpha"], m["weight"], m["lp"], m["mx"])
        m["key"] = "mega_synth_6x40_s2"
        n = len(m["seqs"])
        pairs = [(x, y) for x in range(n) for y in range(n) if x != y]
        ea = np.array([A.oracle_pair(m["seqs"], x, y, m)["ea"] for x, y in pairs], np.float32)
        thr = np.float32(np.sort(ea)[len(ea) // 2])
        groups = [pairs[0:8], pairs[8:9], [], pairs[9:20], pairs[20:30]]
        c.update(seqs=m["seqs"], mega=m, calls=[dict(groups=groups, min_ea=thr, env={}, chunks=1, general=0)])
    else:
        raise KeyError(name)
    return c


def context(c, lib_path=None):
    return E.context({"seqs": c["seqs"], "mega": c["mega"]}, lib_path)


def want_of(c, call):
    """the oracle's answer: (accepted, hits, ea)"""
    acc, hits, ea = [], [], []
    for g in call["groups"]:
        w = [A.oracle_pair(c["seqs"], x, y, c["mega"]) for x, y in g]
        ea += [x["ea"] for x in w]
        t = next((k for k, x in enumerate(w) if np.float32(x["ea"]) >= np.float32(call["min_ea"])), None)
        acc.append(t)
        hits.append(None if t is None else (w[t]["path"], np.float32(w[t]["score"])))
    return acc, hits, np.array(ea, np.float32)


_AP = {}


def align_pairs_fresh(c, call, lib_path):
    """mpcgpu_align_pairs of the call's distinct pairs on a fresh context -> {(x, y): (path, score, ea)}"""
    todo = sorted({p for g in call["groups"] for p in g} - {p for p in _AP.get((lib_path, id(c)), {})})
    have = _AP.setdefault((lib_path, id(c)), {})
    if todo:
        g2 = context(c, lib_path)
        try:
            for p, r in zip(todo, g2.align_pairs([x for x, _ in todo], [y for _, y in todo])):
                have[p] = r
        finally:
            g2.close()
    return have


def same_hits(got, want, what):
    assert len(got) == len(want), what
    for g, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), (what, g, a, b)
        if a is not None:
            assert a[0] == b[0], (what, g, "path")
            assert bits(a[1]) == bits(b[1]), (what, g, "score", a[1], b[1])


def check_call(c, call, g, lib_path, what):
    groups = call["groups"]
    g.timers_reset()
    acc, hits, ea = A.with_env(call["env"], lambda: g.search_pairs(groups, call["min_ea"]))
    info, timers = g.search_info(), g.timers_get()
    if "post_kernel" in call:  # the finishing kernel of the call's last stage
        assert g.post_info()[0] == call["post_kernel"], g.post_info()
    print(what, "accepted", acc[:16], "info", info)
    wacc, whits, wea = want_of(c, call)
    assert np.array_equal(bits(ea), bits(wea)), (what, "ea against the oracle", np.nonzero(bits(ea) != bits(wea))[0][:10])
    assert acc == wacc, (what, acc, wacc)
    if "accepted" in call:
        assert acc == call["accepted"], (what, acc)
    same_hits(hits, whits, what + " against the oracle")
    ap = align_pairs_fresh(c, call, lib_path)
    flat = [p for grp in groups for p in grp]
    assert np.array_equal(bits(ea), bits(np.array([ap[p][2] for p in flat], np.float32))), (what, "ea against mpcgpu_align_pairs")
    same_hits(hits, [None if t is None else ap[grp[t]][:2] for grp, t in zip(groups, acc)], what + " against mpcgpu_align_pairs")
    # ---- the route, and the saving: dense posteriors and trace-backs for the accepted groups alone
    n_acc = sum(t is not None for t in acc)
    assert info[:5] == (len(groups), len(flat), n_acc, call["chunks"], call["general"]), (what, info, n_acc)
    try:  # refused by name after a search
        nz = ctypes.c_uint32()
        g._ck(g.L.mpcgpu_get_list_sparse(g.h, 0, ctypes.byref(nz), None, None))
    except MpcGpuError as e:
        assert "mpcgpu_get_list_sparse" in str(e), str(e)
        assert not flat or "mpcgpu_search_pairs" in str(e), str(e)
    else:
        raise AssertionError("mpcgpu_get_list_sparse accepted after mpcgpu_search_pairs")
    return acc, hits, ea, timers


def check_case(name, size, lib_path=None):
    c = case(name, size)
    results = []
    for k, call in enumerate(c["calls"]):
        g = context(c, lib_path)  # a fresh context per call
        try:
            assert g.search_info() == (0, 0, 0, 0, 0, 0)
            results.append(check_call(c, call, g, lib_path, "%s[%d]" % (name, k)))
        finally:
            g.close()
    if name == "overflow":  # the fused route ran, saw the overflow flag and handed nothing out before the general route ran
        t_both, t_general = results[0][3], results[1][3]
        print("overflow: launches fused + general", {k: v[1] for k, v in t_both.items() if v[1]}, "general alone", {k: v[1] for k, v in t_general.items() if v[1]})
        assert t_both["post"][1] == t_general["post"][1] + 1 and t_both["calc_aln"][1] == t_general["calc_aln"][1] + 1
        assert t_both["fb"][1] > t_general["fb"][1]
    if name == "chunks":  # the result does not depend on the cut
        assert results[0][0] == results[1][0] and np.array_equal(bits(results[0][2]), bits(results[1][2]))
        same_hits(results[0][1], results[1][1], "chunks: cut against uncut")


def check_sequence(size, lib_path=None):
    """one context runs accepted / refused / accepted calls (fused, general, fused) and equals fresh contexts"""
    c = case("row_block", size)
    g = context(c, lib_path)
    try:
        check_call(c, c["calls"][1], g, lib_path, "sequence[fused]")
        e0 = g.store_epoch()
        try:
            g.search_pairs([[(0, 99)]], 0.5)
        except MpcGpuError as e:
            assert "mpcgpu_search_pairs" in str(e) and "out of range" in str(e), str(e)
        else:
            raise AssertionError("accepted")
        assert g.store_epoch() == e0
        check_call(c, c["calls"][0], g, lib_path, "sequence[general]")
        assert g.store_epoch() == e0 + 1
        check_call(c, c["calls"][1], g, lib_path, "sequence[fused again]")
        got = g.align_pairs([2, 4], [3, 1])  # and mpcgpu_align_pairs after it, with its sparse matrices
        for (x, y), r in zip([(2, 3), (4, 1)], got):
            w = A.oracle_pair(c["seqs"], x, y)
            assert r[0] == w["path"] and bits(r[1]) == bits(w["score"]) and bits(r[2]) == bits(w["ea"])
    finally:
        g.close()


def check_refusals(lib_path=None):
    """every refusal is made before any device work: the epoch stays, mpcgpu_search_info stays, the pre-filled outputs come back
    untouched, no kernel is launched, and a following mpcgpu_align_pairs gives what a fresh context gives"""
    seqs = ["MKVLAAGIVGL", "MKVLSAGIVAL", "MKILSAGVVAL", "A" * 25000, "C" * 25000]
    assert 25000 * 25000 * 5 + 100 > E.INT_MAX
    c = {"seqs": seqs, "mega": None}
    w01, w02 = A.oracle_pair(seqs, 0, 1), A.oracle_pair(seqs, 0, 2)
    g = MpcGpu(0, lib_path)
    try:
        L = g.L
        u32 = lambda *v: np.array(v, np.uint32)
        first, s1, s2 = u32(0, 2), u32(0, 0), u32(1, 2)

        def raw(first=first, s1=s1, s2=s2, stride=64, null=None, ng=1):
            paths, plen, acc = np.full(256, 0x5a, np.uint8), np.full(4, 77, np.uint32), np.full(4, 78, np.uint32)
            sc, ea = np.full(4, -3.0, np.float32), np.full(8, -4.0, np.float32)
            arg = {"first": first.ctypes.data, "s1": s1.ctypes.data, "s2": s2.ctypes.data, "paths": paths.ctypes.data, "plen": plen.ctypes.data,
                   "acc": acc.ctypes.data, "sc": sc.ctypes.data, "ea": ea.ctypes.data}
            if null:
                arg[null] = None
            rc = L.mpcgpu_search_pairs(g.h, ng, arg["first"], arg["s1"], arg["s2"], 0.1, stride, arg["paths"], arg["plen"], arg["acc"], arg["sc"], arg["ea"])
            untouched = (paths == 0x5a).all() and (plen == 77).all() and (acc == 78).all() and (sc == -3.0).all() and (ea == -4.0).all()
            return rc, untouched, (paths, plen, acc, sc, ea)

        def refused(words, **kw):
            g.timers_reset()
            epoch, info = g.store_epoch(), g.search_info()
            rc, untouched, _ = raw(**kw)
            assert rc != 0, ("accepted", words)
            msg = L.mpcgpu_last_error(g.h).decode()
            assert all(w in msg for w in ("mpcgpu_search_pairs",) + words), msg
            assert untouched, words
            t = g.timers_get()
            assert all(t[f][1] == 0 for f in t), t
            assert g.store_epoch() == epoch and g.search_info() == info

        refused(("mpcgpu_set_seqs",))  # no sequences
        s, t, m, i, thr = G.hmm_tables()
        g.set_hmm(s, t, m, i, thr)
        g.set_seqs_registry(seqs)
        for null in ("first", "s1", "s2", "paths", "plen", "acc"):
            refused(("NULL",), null=null)
        refused(("group_first[0]", "not 0"), first=u32(1, 2))
        refused(("not ascending", "group 1"), first=u32(0, 2, 1), ng=2)
        refused(("out of range", "pair 1"), s1=u32(0, 5))
        refused(("out of range", "pair 0"), s2=u32(9, 1))
        refused(("path_stride 21", "pair 0"), stride=21)
        refused(("LX=25000", "LY=25000", "INT_MAX"), s1=u32(0, 3), s2=u32(1, 4), stride=50000)
        # ... and the context is as good as new: a search with NULL scores / ea, then mpcgpu_align_pairs
        rc, _, (paths, plen, acc, sc, ea) = raw(null="sc")
        assert rc == 0 and acc[0] == 0 and bits(ea[:2]).tolist() == [int(bits(w01["ea"])), int(bits(w02["ea"]))] and (sc == -3.0).all()
        assert paths[:plen[0]].tobytes().decode() == w01["path"]
        rc, _, (paths, plen, acc, sc, ea) = raw(null="ea")
        assert rc == 0 and acc[0] == 0 and bits(sc[0]) == bits(w01["score"]) and (ea == -4.0).all()
        refused(("out of range",), s1=u32(0, 5))
        got = g.align_pairs([0, 0], [1, 2], sparse=True)
        g2 = context(c, lib_path)
        try:
            fresh = g2.align_pairs([0, 0], [1, 2], sparse=True)
        finally:
            g2.close()
        for a, b in zip(got[0], fresh[0]):
            assert a[0] == b[0] and bits(a[1]) == bits(b[1]) and bits(a[2]) == bits(b[2])
        for (o1, v1), (o2, v2) in zip(got[1], fresh[1]):
            assert np.array_equal(o1, o2) and np.array_equal(v1, v2)
    finally:
        g.close()
