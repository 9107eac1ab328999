"""A record store in SEGMENTS (muscle_amd/csrc/kernels_store.h: StoreParams::pad_zbase) on a dozen short sequences: the test hook
MPCGPU_STORE_SEG_BLOCKS lowers the segment limit so far that the store splits, and every kernel then runs what it runs on a store beyond
2^32 blocks — own allocations, 64-bit bases per Z slab, record ends that are not "the next table entry". Shared by
tests/test_gpu_store_segments.py (the HIP library) and tests/test_emu_store_segments.py (the emulator build of the same sources).

The hook is read from the environment, so every case runs in a fresh child process: this file as a script,
`python _store_segments.py MODE OUT [LIB]`, which pickles what it saw into OUT. The parent compares with the oracle (computed once) and
with the record sizes it derives from the oracle's stage-0 matrices: the segments the host-only planner cuts from those sizes are the
segments the library must report."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOOK = "MPCGPU_STORE_SEG_BLOCKS"
# ("long": the long form of the block records, kernels_store.h: no window records, MpcRbSegmented<MpcRbLongCxx>)
FORMS = {"windows": {"MPCGPU_RELAX_WIN_PCT": "100000"}, "walk": {"MPCGPU_RELAX_FORM": "walk"}, "long": {"MPCGPU_RELAX_LONG": "1"}}
MERGE = {"windows": "MpcRbSegmented<MpcRbWin", "walk": "MpcRbSegmented<MpcRbBlocks", "long": "MpcRbSegmented<MpcRbLongCxx"}


def family():
    """13 ragged sequences of 3..120 residues: two families, a fragment and an unrelated sequence"""
    from muscle_amd.synth import make_family
    f = make_family(5, 110, seed=11) + make_family(4, 45, seed=5) + make_family(2, 30, seed=7) + [make_family(1, 70, seed=9)[0], "MKV"]
    # small Z slabs between large ones: any two neighbours together pass the largest slab, so that a limit of exactly that slab puts
    # a segment boundary after EVERY Z (Ref.limits)
    return [f[i] for i in (1, 6, 11, 10, 4, 9, 2, 5, 3, 12, 0, 8, 7)]


def record_sizes(seqs, stage0):
    """(blocks, windows): the n x n record sizes in 16-byte blocks, Z-major, of the block records and the window records
    (kernels_store.h: var_size_kernel, win_size_kernel), from the sparse matrices of all pairs in InitPairs order"""
    n = len(seqs)
    lens = [len(s) for s in seqs]
    pidx = {}
    for x in range(n):
        for y in range(x + 1, n):
            pidx[(x, y)] = len(pidx)
    blocks = np.zeros((n, n), np.uint32)  # [Z][A]
    wins = np.zeros((n, n), np.uint32)
    for Z in range(n):
        for A in range(n):
            LA = lens[A]
            if A == Z:
                ovf, vals = 0, LA
            else:
                o, v = stage0[pidx[(min(A, Z), max(A, Z))]]
                o = np.asarray(o, np.int64)
                cols = np.asarray(v[1::2], np.int64)
                rows = np.repeat(np.arange(len(o) - 1), np.diff(o))
                mine, other = (rows, cols) if A < Z else (cols, rows)  # row of M(A,Z), its column
                cnt = np.bincount(mine, minlength=LA)
                lo = np.full(LA, 1 << 30)
                hi = np.full(LA, -1)
                np.minimum.at(lo, mine, other)
                np.maximum.at(hi, mine, other)
                ovf = int(np.maximum((cnt + 1) // 2 - 1, 0).sum())
                vals = int(np.where(cnt > 0, hi - lo + 1, 0).sum()) + LA
            blocks[Z, A] = LA + ovf
            wins[Z, A] = (LA + 1 + 3) // 4 + (vals + 3) // 4 + 1
    return blocks.ravel(), wins.ravel()


def slabs(sizes, n):
    return np.asarray(sizes, np.int64).reshape(n, n).sum(axis=1)


def seg_counts(info):
    """(segments of the block records, of the window records) as mpcgpu_relax_info words them; 1 where it names none"""
    b = re.search(r"in (\d+) segments of whole Z slabs", info)
    w = re.search(r"of the blocks\) in (\d+) segments", info)
    return (int(b.group(1)) if b else 1, int(w.group(1)) if w else 1)


def child(mode, env, lib_path, tmp_path, timeout=600):
    """one case in a fresh process -> what it pickled"""
    out = os.path.join(str(tmp_path), "seg_%s_%d.pkl" % (mode, abs(hash(tuple(sorted(env.items())))) % 10 ** 8))
    e = dict(os.environ)
    e.update(env)
    e["PYTHONPATH"] = os.pathsep.join([ROOT, HERE] + ([e["PYTHONPATH"]] if e.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, out] + ([lib_path] if lib_path else []), env=e, timeout=timeout,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "child %s %s failed (%d):\n%s" % (mode, env, r.returncode, r.stdout[-3000:])
    with open(out, "rb") as f:
        return pickle.load(f)


# ---- the child -----------------------------------------------------------------------------------------------------------
def _join_cases(seqs):
    import _buildpost as BP
    rng = np.random.default_rng(17)
    n = len(seqs)
    groups = [(list(range(0, n, 2)), list(range(1, n, 2))), ([n - 1, 2], [0, 5, n - 2]), ([4], [1])]
    out = []
    for grp1, grp2 in groups:
        rows1, C1 = BP.random_msa(seqs, grp1, rng)
        rows2, C2 = BP.random_msa(seqs, grp2, rng)
        w = rng.uniform(0.2, 1.5, n).astype(np.float32)
        out.append((grp1, grp2, [BP.pos_to_col(r) for r in rows1], [BP.pos_to_col(r) for r in rows2], C1, C2, w[:len(grp1)], w[:len(grp2)]))
    return out


def _main(mode, out, lib_path):
    import _pair_order as PO
    import _parity as P
    from muscle_amd._lib import MpcGpu, MpcGpuError, plan_partition
    seqs = family()
    res = {}
    if mode == "stages":
        info = {}
        res["stages"], res["ea"] = P.run_lib(seqs, lib_path=lib_path, info=info)
        res["info"], res["fallback"], res["window_bytes"] = info["relax_info"], info["relax_fallback"], info["store_info"]["window_bytes"]
    elif mode == "pairs":  # MPCGPU_RELAX_TILES=pairs on a store in segments: refused by name
        try:
            P.run_lib(seqs, lib_path=lib_path)
            res["error"] = None
        except MpcGpuError as e:
            res["error"] = str(e)
    elif mode == "joins":  # two committed iterations, then BuildPost in both device forms and the weighted AlignAlns
        g = PO.new_ctx(lib_path, seqs)
        PO.run_on(g)
        res["info"], res["fallback"] = g.relax_info()
        res["joins"] = []
        for grp1, grp2, m1, m2, C1, C2, w1, w2 in _join_cases(seqs):
            for bp in ("rows", "sort"):
                with PO.Env({"MPCGPU_BP": bp}):
                    post = g.build_post(grp1, grp2, m1, m2, C1, C2)
                    postw = g.build_post(grp1, grp2, m1, m2, C1, C2, w1, w2)
                    path, sc = g.align_alns(grp1, grp2, m1, m2, C1, C2, w1, w2)
                    res["joins"].append((bp, post.copy(), postw.copy(), path, np.float32(sc), g.last_post(C1, C2).copy()))
        g.close()
    elif mode == "partial":  # two contexts, the block partition, partial stores, store_complete, joins: _pair_order's own check
        rects, _ = plan_partition([len(s) for s in seqs], 2, lib_path)
        assert len(rects), "the partition of two ranks cuts blocks at this size"
        infos = []
        orig = MpcGpu.store_import_part

        def spy(self, *a, **k):
            orig(self, *a, **k)
            infos.append(self.relax_info())
        MpcGpu.store_import_part = spy
        PO.check_partial_exchange(lib_path, seqs, rects, seed=3, joins=1)
        res["infos"] = infos
    elif mode == "lifetime":  # another n on the same context after a store in segments, and the first one again
        g = PO.new_ctx(lib_path, seqs)
        res["runs"] = []
        for sub in (seqs, seqs[2:9], seqs):
            g.set_seqs(sub)
            st, ea = PO.run_on(g)
            res["runs"].append((st, ea, g.relax_info()))
        g.close()
    else:
        raise SystemExit("unknown mode " + mode)
    with open(out, "wb") as f:
        pickle.dump(res, f)


# ---- the checks (parent) ---------------------------------------------------------------------------------------------------
class Ref:
    """the oracle's run of the family, its record sizes and the two limits of case 1, computed once per module"""

    def __init__(self):
        import _parity as P
        from muscle_amd._lib import plan_store_segments
        self.seqs = family()
        self.n = len(self.seqs)
        self.want = P.run_oracle(self.seqs)
        self.blocks, self.wins = record_sizes(self.seqs, self.want[0][0])
        self.plan = lambda sizes, limit: plan_store_segments(self.n, sizes, limit)
        sb, sw = slabs(self.blocks, self.n), slabs(self.wins, self.n)
        # "every": the smallest limit that still holds the largest slab of either copy; "few": three to four slabs of blocks
        self.limits = {"every": int(max(sb.max(), sw.max())), "few": int(3.6 * np.median(sb))}
        self.limits_walk = {"every": int(sb.max()), "few": self.limits["few"]}

    def expect(self, limit, windows):
        nb = len(self.plan(self.blocks, limit)[1])
        return (nb, len(self.plan(self.wins, limit)[1]) if windows else 1)


def check_stages(ref, got, plain, form, limit, what):
    """a segmented run of case 1 == the oracle == the run without the hook, on band tiles, in the segments the planner cuts"""
    import _parity as P
    P.assert_same((got["stages"], got["ea"]), ref.want, what + " vs oracle")
    P.assert_same((got["stages"], got["ea"]), (plain["stages"], plain["ea"]), what + " vs one segment")
    assert seg_counts(plain["info"]) == (1, 1) and "MpcRbSegmented" not in plain["info"], plain["info"]
    want = ref.expect(limit, form == "windows")
    assert seg_counts(got["info"]) == want, (what, want, got["info"])
    assert want[0] > 1 and got["fallback"] == 0, (what, got["info"])
    assert "relax_band_kernel" in got["info"] and MERGE[form] in got["info"], got["info"]
    assert ("band-long" in got["info"]) == ("band-long" in plain["info"]) == (form == "long"), (got["info"], plain["info"])
    if form == "long":  # no window records, with the hook and without it
        for run in (got, plain):
            assert "window records" not in run["info"] and run["window_bytes"] == 0, (what, run["info"], run["window_bytes"])


def same_joins(a, b, count=6):
    """the joins of two runs of the child's "joins" mode: form, path, score and the three matrices of each, bit for bit"""
    import _parity as P
    assert len(a["joins"]) == len(b["joins"]) == count
    for (bp, post, postw, path, sc, last), (bp2, post2, postw2, path2, sc2, last2) in zip(a["joins"], b["joins"]):
        assert bp == bp2 and path == path2 and P.bits(sc) == P.bits(sc2), (bp, path, path2)
        for x, y in ((post, post2), (postw, postw2), (last, last2)):
            assert np.array_equal(P.bits(x), P.bits(y)), bp


def check_lifetime(ref, got, form):
    """the child's "lifetime" mode: all sequences, seven of them, all again on one context, each equal to the oracle, in segments"""
    import _parity as P
    subs = (ref.seqs, ref.seqs[2:9], ref.seqs)
    wants = (ref.want, P.run_oracle(subs[1]), ref.want)
    for (st, ea, (info, fallback)), want, sub in zip(got["runs"], wants, subs):
        P.assert_same((st, ea), want, "n = %d" % len(sub))
        assert seg_counts(info)[0] > 1 and fallback == 0, info
        if form == "long":
            assert "band-long" in info and MERGE["long"] in info and "window records" not in info, info


if __name__ == "__main__":
    _main(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
