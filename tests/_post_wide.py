"""post_wide_kernel (muscle_amd/csrc/kernels_postw.h: the finishing kernel with a workgroup per pair — radix sort, row-start table, EA
over the whole workgroup) — shared by tests/test_emu_post_wide.py (the emulator build, workgroups of 128) and
tests/test_gpu_post_wide.py (the device, workgroups of 1024). Every comparison is 0 ulp / byte-equal.

A  candidate lists through mpcgpu_post_scores(kernel = 2) against the oracle's dense CalcAlnScoreFlat / FromPost, and the same lists
   through kernel 1 (post_kernel); post_info() after each call. Each shape with the default LDS buffers and with MPCGPU_POSTW_LDS=0
   (keys ping-pong through the global slots, DP rows in the global slot; the row-start table is global either way).
B  a whole stage (calc_posteriors, build_store, two cons_iter) under MPCGPU_POST_WIDE=1 against the oracle, and the shard's bytes
   against the stage under MPCGPU_POST=sort MPCGPU_POST_WIDE=0: the packed records with their row and tperm sections.
C  mpcgpu_align_pairs on the forced route (tests/_align_pairs_long.py small_scenarios) under MPCGPU_POST_WIDE=1 and =0, and
   post_info() after such a call.
TEST INFRASTRUCTURE."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np

import _align_pairs as A
import _align_pairs_long as L
import _golden as G
import _oracle as O
import _parity as P
from muscle_amd._lib import MpcGpu

VARIANT = 1
THREADS = (1024, 128)  # kernels_postw.h MPC_POSTW_THREADS: the device, the emulator
KEY_SHIFT, KEY_SHIFT_LONG = 22, 16  # kernels_fb.h: MPC_KEY_ROW_SHIFT, MPC_KEY_ROW_SHIFT_LONG (mpcgpu_post_scores: the latter when LX > 1023)


def radix_passes(LX):
    """the kernel's digit rule: 8 bits per pass over the flat index's significant bits, key shift + bits(LX - 1)"""
    shift = KEY_SHIFT_LONG if LX > 1023 else KEY_SHIFT
    return (shift + (LX - 1).bit_length() + 7) // 8


assert radix_passes(1100) == 4  # 16 + 11 = 27 bits
assert radix_passes(12) == 4    # 22 + 4 = 26 bits
assert radix_passes(1) == 3     # 22 bits


# ---- A: lists ----------------------------------------------------------------------------------------------------------------
# shape -> densities (the staircase generator is added to every shape)
ALL = (0.02, 0.3, 0.9)
SHAPES = {
    (1, 1): ALL, (1, 9): ALL, (7, 1): ALL, (3, 6): ALL,  # degenerate widths
    (90, 70): ALL, (5, 200): ALL,                          # below and above one workgroup's width; counts that are no multiple of it
    (3, 2500): ALL,    # 0.9: more than 1024 cells in a row (binary search, several cells per lane, 3 columns per lane on the device)
    (1100, 40): ALL,   # LX > 1023: 16-bit column keys, 27 significant bits, 4 radix passes
    (12, 40): ALL,     # 22-bit shift, 26 significant bits: 4 passes by the digit rule (radix_passes)
    (300, 2100): ALL,  # DP rows beyond a lowered LDS row cap (MPCGPU_POSTW_LDS=0), lists beyond the LDS key buffers
}
# the emulator runs the same table with fewer trials: the large shapes at the densities that keep a run at seconds
EMU_DENS = {(3, 2500): (0.9,), (1100, 40): (0.3,), (300, 2100): (0.02,)}
SPECIAL = ["fixed", "empty", "one_cell", "all_below"]


def _staircase(LX, LY, rng):
    mask = np.zeros((LX, LY), bool)
    c = 0
    for r in range(LX):
        c += int(rng.integers(1, 5))
        if c >= LY:
            break
        mask[r, c] = True
        if rng.random() < 0.3 and c + 2 < LY:
            mask[r, c + 2] = True
    return mask


def _scores(n, rng, thr):
    # from log(0.0098) (dropped by FromPost: P < 0.01) up to slightly above 0 (P = 1)
    sc = rng.uniform(np.log(0.0098), 0.05, n).astype(np.float32)
    return np.maximum(sc, np.float32(thr))


def _reference(LX, LY, rows, cols, sc):
    orc = O.lib()
    Pd = np.zeros((LX, LY), np.float32)
    for r, c, x in zip(rows, cols, sc):
        Pd[r, c] = np.float32(1.0) if x >= 0 else np.float32(orc.orc_expf_emul(float(x), VARIANT))
    want_ea = np.float32(O.aln_score(Pd)) / np.float32(min(LX, LY))
    woff, wval = O.sparse_from_post(Pd)
    return want_ea, woff, wval


@functools.lru_cache(maxsize=None)
def lists_of(key, emu):
    """the candidate lists of a shape (or of a SPECIAL name) with their oracle results: computed once, shared by the runs"""
    thr = G.hmm_tables()[4]
    rng = np.random.default_rng(sum(ord(ch) for ch in str(key)) + 977)  # (a seed per shape that does not depend on the hash salt)
    raw = []
    if key == "fixed":  # the advisor's minimal case: the dense DP gives 1.4
        cells = [(0, 3, 0.9), (1, 5, 0.3), (2, 2, 0.3), (2, 5, 0.5)]
        raw.append((3, 6, [c[0] for c in cells], [c[1] for c in cells], np.log(np.array([c[2] for c in cells], np.float32))))
    elif key == "empty":
        raw.append((4, 7, [], [], np.zeros(0, np.float32)))
        raw.append((1, 1, [], [], np.zeros(0, np.float32)))
    elif key == "one_cell":
        raw.append((6, 5, [3], [4], np.array([np.log(0.7)], np.float32)))
        raw.append((1, 1, [0], [0], np.array([0.01], np.float32)))
    elif key == "all_below":  # kept = 0: the tperm sort runs over nothing, EA is still that of the small probabilities
        mask = rng.random((9, 33)) < 0.4
        rows, cols = np.nonzero(mask)
        raw.append((9, 33, rows, cols, np.full(len(rows), np.float32(np.log(0.00985)), np.float32).clip(np.float32(thr), None)))
    else:
        LX, LY = key
        dens = EMU_DENS.get(key, SHAPES[key]) if emu else SHAPES[key]
        masks = [rng.random((LX, LY)) < d for d in dens] + [_staircase(LX, LY, rng)]
        for mask in masks:
            rows, cols = np.nonzero(mask)
            perm = rng.permutation(len(rows))  # cells in random order
            raw.append((LX, LY, rows[perm], cols[perm], _scores(len(rows), rng, thr)))
    return [(LX, LY, np.asarray(rows, np.uint32), np.asarray(cols, np.uint32), sc, _reference(LX, LY, rows, cols, sc))
            for LX, LY, rows, cols, sc in raw]


def check_lists(key, lib_path=None):
    emu = lib_path is not None
    s, t, m, i, thr = G.hmm_tables()
    g = MpcGpu(0, lib_path)
    try:
        g.set_hmm(s, t, m, i, thr, VARIANT)
        for LX, LY, rows, cols, sc, (want_ea, woff, wval) in lists_of(key, emu):
            what = "%s: %dx%d, %d cells" % (key, LX, LY, len(rows))
            ea1, off1, val1 = g.post_scores(LX, LY, rows, cols, sc, 1)
            assert g.post_info()[:3] == (1, 64, 1), (what, g.post_info())
            for env in ({}, {"MPCGPU_POSTW_LDS": "0"}):
                ea, off, val = A.with_env(env, lambda: g.post_scores(LX, LY, rows, cols, sc, 2))
                info = g.post_info()
                assert info[0] == 2 and info[1] in THREADS and info[2] == 1, (what, env, info)
                assert info[3] == radix_passes(LX), (what, env, info)
                assert P.bits(ea) == P.bits(want_ea), "EA %s %s: %r vs %r" % (what, env, ea, want_ea)
                assert np.array_equal(off, woff) and np.array_equal(val, wval), (what, env, "against the oracle")
                assert P.bits(ea) == P.bits(ea1) and np.array_equal(off, off1) and np.array_equal(val, val1), (what, env, "against kernel 1")
            if (LX, LY) == (1100, 40):
                assert g.post_info()[3] == 4
    finally:
        g.close()


def check_kernel_argument(lib_path=None):
    """values above 2 are refused by name; 0 and 1 keep their kernels"""
    from muscle_amd._lib import MpcGpuError
    s, t, m, i, thr = G.hmm_tables()
    g = MpcGpu(0, lib_path)
    try:
        g.set_hmm(s, t, m, i, thr, VARIANT)
        assert g.post_info() == (0, 0, 0, 0)
        LX, LY, rows, cols, sc, _ = lists_of("fixed", lib_path is not None)[0]
        for bad in (3, 7, -1):
            try:
                g.post_scores(LX, LY, rows, cols, sc, bad)
                raise AssertionError("kernel %d was accepted" % bad)
            except MpcGpuError as e:
                assert "mpcgpu_post_scores" in str(e) and "post_wide_kernel" in str(e), str(e)
        g.post_scores(LX, LY, rows, cols, sc, 0)
        assert g.post_info() == (0, 64, 1, 0)
        g.post_scores(LX, LY, rows, cols, sc, 1)
        assert g.post_info() == (1, 64, 1, 0)
    finally:
        g.close()


# ---- B: a whole stage --------------------------------------------------------------------------------------------------------
def _read_device(ptr, nbytes, emu, mem):
    out = np.empty(nbytes, np.uint8)
    if emu:
        C.memmove(out.ctypes.data, ptr, nbytes)
    else:
        mem.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert mem.hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


def _stage(seqs, hmm_name, mega, lib_path, env):
    """-> ((stages, ea), post_info after stage A, the exported shard's bytes)"""
    from _pair_order import DevMem

    def run():
        s, t, m, i, thr = G.hmm_tables(hmm_name)
        g = MpcGpu(0, lib_path)
        mem = DevMem(lib_path)
        try:
            g.set_hmm(s, t, m, i, thr)
            g.set_seqs(seqs)
            if mega is not None:
                g.set_mega(mega["alpha"], mega["weight"], mega["lp"], mega["mx"], mega["profs"])
            g.calc_posteriors()
            info = g.post_info()
            nbytes = g.shard_info()[0]
            buf = mem.alloc(nbytes)
            g.shard_export(buf)
            g.synchronize()
            shard = _read_device(buf, nbytes, lib_path is not None, mem)
            ea = g.get_ea().copy()
            g.build_store()
            stages = [g.get_sparse_range()]
            for _ in range(2):
                g.cons_iter()
                g.cons_commit()
                stages.append(g.get_sparse_range())
            return (stages, ea), info, shard
        finally:
            g.close()
            mem.free()
    return A.with_env(env, run)


STAGE_SETS = ["amino", "mega"]


def check_stage(which, lib_path=None):
    if which == "amino":
        seqs, hmm_name, mega = G.mpc("n8_L60")["seqs"], "hmm_amino", None
    else:
        d = G.mega("mega_synth_6x40_s2")
        seqs, hmm_name, mega = d["seqs"], "hmm_amino", {k: d[k] for k in ("alpha", "weight", "lp", "mx", "profs")}
    npairs = len(seqs) * (len(seqs) - 1) // 2
    want = P.run_oracle(seqs, hmm_name=hmm_name, mega=mega)
    got, info, shard = _stage(seqs, hmm_name, mega, lib_path, {"MPCGPU_POST_WIDE": "1"})
    P.assert_same(got, want, "MPCGPU_POST_WIDE=1")
    LXbig = max(len(s) for s in seqs[:-1])
    assert info[0] == 2 and info[1] in THREADS and info[2] == npairs and info[3] == radix_passes(LXbig), info
    got1, info1, shard1 = _stage(seqs, hmm_name, mega, lib_path, {"MPCGPU_POST": "sort", "MPCGPU_POST_WIDE": "0"})
    assert info1 == (1, 64, npairs, 0), info1
    P.assert_same(got1, want, "MPCGPU_POST=sort")
    assert shard.tobytes() == shard1.tobytes(), "packed records (rowcnt, colcnt, ent, row, tperm) differ between post_wide_kernel and post_kernel"
    # unset and 0: a list that fits keeps the row-list kernel
    got0, info0, _ = _stage(seqs, hmm_name, mega, lib_path, {"MPCGPU_POST_WIDE": "0"})
    assert info0[:3] == (0, 64, npairs) and info0[3] == 0, info0
    P.assert_same(got0, want, "MPCGPU_POST_WIDE=0")


# ---- C: mpcgpu_align_pairs on the forced route ----------------------------------------------------------------------------------
def wide_scenario(name):
    """the scenario as MPCGPU_POST_WIDE=1 defines its routes. Forced wide, EVERY list takes the raw dense build — also one that would fit
    the row-list kernel — so the one call of small_scenarios() that asks for the row-list route ("letters": "the row-list route after
    it") carries the forcing value here, which makes the route it is checked against the one the knob prescribes. All else is the
    scenario of tests/_align_pairs_long.py."""
    sc = L.scenario(name)
    for call in sc.calls:
        if L.FORCE["MPCGPU_POST_SORT_CAP"] != call.env.get("MPCGPU_POST_SORT_CAP"):
            call.env = L.forced(call.env)
    return sc


def check_align_pairs(name, lib_path, aln_waves, wide):
    """small_scenarios() under MPCGPU_POST_WIDE. "0": L.check unchanged. "1": the same child, calls and per-call checks
    (L.run_scenario, L.check_call) on wide_scenario(name); the "other expf variant" call compares its list with a second run that drops
    the forcing value, which under the knob is a second raw build: its trace is checked for exactly those two builds. "regrowth" is
    scenario D of the issue: MPCGPU_CAND_PER_ROW=1 overflows post_wide_kernel's lists, the flag reaches the host, the regrown run matches
    the oracle."""
    if wide == "0":
        L.check(name, lib_path, aln_waves, extra_env={"MPCGPU_POST_WIDE": "0"})
        return
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MPCGPU_TRACE="1", MPCGPU_POST_WIDE="1", PYTHONPATH=os.path.dirname(here) + os.pathsep + here)
    r = subprocess.run([sys.executable, "-u", os.path.join(here, "_post_wide.py"), name, lib_path or ""], env=env, cwd=here,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500, text=True)
    out = r.stdout
    assert r.returncode == 0 and "OK scenario" in out, "exit %d\n%s" % (r.returncode, out[-4000:])
    sc = wide_scenario(name)
    parts = [p.split("\nEND\n", 1)[0] for p in out.split("CALL ")[1:]]
    assert len(parts) == len(sc.calls), (name, len(parts))
    for k, (call, part) in enumerate(zip(sc.calls, parts)):
        assert "[mpcgpu] post wide: " in part and "[mpcgpu] post: sort_cap" not in part and "[mpcgpu] post rows: " not in part, (name, k, "finishing kernel")
        if call.expf == "other":
            assert [ln for ln in part.splitlines() if ln.startswith(("PASS ", "FAIL "))] == ["PASS %d" % k], (name, k, part[-2000:])
            raws = [int(ln[len(L.RAW_LINE):].split()[0]) for ln in part.splitlines() if ln.startswith(L.RAW_LINE)]
            assert raws == [len(call.pairs)] * 2, (name, k, raws)
            continue
        L.check_call(sc, k, part, aln_waves)


def check_align_pairs_info(lib_path=None):
    """post_info()[0] after an align_pairs under FORCE: 2 with MPCGPU_POST_WIDE=1, 1 with 0"""
    seqs = A.related([20, 64, 130, 90], 201)
    s, t, m, i, thr = G.hmm_tables()
    g = MpcGpu(0, lib_path)
    try:
        g.set_hmm(s, t, m, i, thr)
        g.set_seqs_registry(seqs)
        pairs = [(0, 1), (2, 3), (3, 2)]
        res = {}
        for wide in ("1", "0"):
            res[wide] = A.with_env(dict(L.FORCE, MPCGPU_POST_WIDE=wide), lambda: g.align_pairs([a for a, _ in pairs], [b for _, b in pairs]))
            info = g.post_info()
            if wide == "1":
                assert info[0] == 2 and info[1] in THREADS and info[2] == len(pairs) and info[3] == radix_passes(130), info
            else:
                assert info == (1, 64, len(pairs), 0), info
        for (p1, s1, e1), (p0, s0, e0) in zip(res["1"], res["0"]):
            assert p1 == p0 and P.bits(s1) == P.bits(s0) and P.bits(e1) == P.bits(e0)
    finally:
        g.close()


if __name__ == "__main__":
    L.run_scenario(wide_scenario(sys.argv[1]), sys.argv[2] or None)
