"""Chains finished inside the sweeps (fb_chain_post_kernel, MPCGPU_FB_POST_FUSE) against the separate finishing launch and the oracle.

A case is a set of sequences and the knobs both runs share. The stage runs with MPCGPU_FB_POST_FUSE=1 and =0 on fresh contexts; the
exported shards (per pair: row counts, column counts, entries, rows, tperm, behind the header with every nnz and EA) must be the same
bytes, EA and nnz the same bits, and the store built from the fused shard and its EA must be the oracle's. The per-pair overflow flag
never leaves the library: a retry shows as a stage that still matches with a candidate room that cannot hold the lists at first.
stage_a_fuse_info() says how many pairs the sweeps finished: `fused` states what a case expects of it ("all", "some", "none", or
"rule": the pairs of the bins MPCGPU_FB_POST_FUSE=2 fuses). A case may carry the knob's value (default 1), the least number of
launches of the finishing family it must show (a finishing launch and a pack per batch, one more finishing launch per redone batch:
how a case proves its batches and its retry), and oracle=False where the comparison with the separate launch has to do."""
import numpy as np

import _align_pairs as A
import _parity as P
from muscle_amd._lib import MpcGpu
from muscle_amd.synth import make_family


def cut(seqs, lengths):
    return [s[:n] for s, n in zip(seqs, lengths)]


def family(lengths, seed):
    return cut(make_family(len(lengths), max(lengths), seed=seed), lengths)


H23 = [70, 130, 97, 128, 129, 85, 111, 64 + 9]          # 8 sequences of 70..130: two and three rows per lane, LX < LY, > LY, equal (below)
H23 = H23 + [97, 130]                                   # two lengths twice: LX == LY
H7 = [390, 410, 401, 397, 410, 385 + 8]                 # the benchmark's bin
TINY = ["M", "KV", "ACD", "WYFL", "GHIKL"]


def cases(emu):
    c = {}
    for cmax in ("2", "16"):
        for grade in ("0", "1"):
            c["chains_max%s_grade%s" % (cmax, grade)] = (family(H23, 31), {"MPCGPU_FB_CHAIN_MAX": cmax, "MPCGPU_FB_CHAIN_GRADE": grade}, "all")
    c["h7"] = (family(H7, 32), {}, "all")
    # sequences of 1..5 residues beside the family, and rows of 100 and more as row-block pairs: those take the separate launch in the same call
    c["mixed"] = (family(H23, 33) + TINY, {"MPCGPU_FB_LONG_MIN": "100", "MPCGPU_FB_LONG_H": "1"}, "some")
    c["list_beyond_lds"] = (family(H23, 34), {"MPCGPU_POST_SORT_CAP": "2"}, "all")
    c["row_beyond_ea_batch"] = (family(H23, 35), {"MPCGPU_POST_BATCH": "2"}, "all")
    # 1024 candidates per pair is the floor MPCGPU_CAND_PER_ROW=1 leaves: poly-A 60 x 100 holds 1627 (tests/_stage_a.py), the batch is redone
    over = ["A" * 60, "A" * 100] + family(H23[:3], 36)
    c["overflow_retry"] = (over, {"MPCGPU_CAND_PER_ROW": "1"}, "all", "1", 3)
    c["empty_list"] = (["AAAAAAAAA", "WWWWWWWWWWWW"], {}, "all")
    # every pair its own batch (MPCGPU_SCRATCH_GB=0): the sweeps of batch b + 1 write the second set of records, sizes and flags while batch b
    # is read back and packed, and the sets change places at every boundary; with the small room, batches are redone with the next one queued
    n23 = len(H23) * (len(H23) - 1) // 2
    c["batches_of_one"] = (family(H23, 40), {"MPCGPU_SCRATCH_GB": "0"}, "all", "1", 2 * n23)
    c["overflow_retry_batches_of_one"] = (over, {"MPCGPU_SCRATCH_GB": "0", "MPCGPU_CAND_PER_ROW": "1"}, "all", "1", 2 * 10 + 1)
    # the rule: bins whose fused workgroup is as often resident and uses no scratch memory. On the device H = 7 spills and H = 2 would lose a workgroup per CU: their chains go
    # to the finishing launch through the index list, beside the fused chains of H = 3; the emulator has no registers and fuses all
    c["mixed_bins_rule"] = (family(H23[:7] + H7[:3], 42), {}, "rule", "2")
    if not emu:
        # two batches with chains in each: 44 850 pairs of three rows per lane under 1 GB of scratch (~38 KB per pair; the forward planes
        # that 1 GB leaves still take chains of two at these lengths); against the separate launch only
        c["two_batches"] = (family([129 + (7 * k) % 31 for k in range(300)], 43), {"MPCGPU_SCRATCH_GB": "1"}, "all", "1", 4, False)
    c["chains_off"] = (family(H23, 37), {"MPCGPU_FB_CHAIN": "0"}, "none")
    c["sort_kernel"] = (family(H23, 38), {"MPCGPU_POST": "sort"}, "none")
    return c


NAMES = sorted(cases(False))
EMU_NAMES = sorted(cases(True))


def rule_pairs(seqs, bins):
    """pairs finished in the sweeps when every pair runs in the chain kernel and the bins `bins` (stage_a_fuse_bins(): which ones the
    rule takes depends on the registers the compiler gave each instantiation) are fused: those whose row sequence — the first of the
    pair — has that many rows per lane"""
    return sum(len(seqs) - 1 - i for i, q in enumerate(seqs) if (len(q) + 63) // 64 in bins)


def stage(seqs, env, lib_path):
    """-> dict(shard bytes, ea, nnz, fused pairs, store) of one stage on a fresh context"""
    from _pair_order import DevMem
    from _post_wide import _read_device

    def run():
        s, t, m, i, thr = P.G.hmm_tables("hmm_amino")
        g = MpcGpu(0, lib_path)
        mem = DevMem(lib_path)
        try:
            g.set_hmm(s, t, m, i, thr)
            g.set_seqs(seqs)
            g.timers_enable(True)
            g.timers_reset()
            g.calc_posteriors()
            out = {"fused": g.stage_a_fuse_info(), "bins": g.stage_a_fuse_bins(), "pairs": g.stage_a_info()[0], "post_launches": g.timers_get()["post"][1]}
            nbytes = g.shard_info()[0]
            buf = mem.alloc(nbytes)
            g.shard_export(buf)
            g.synchronize()
            out["shard"] = _read_device(buf, nbytes, lib_path is not None, mem).tobytes()
            out["ea"], out["nnz"] = g.get_ea().copy(), g.get_nnz().copy()
            g.build_store()
            out["store"] = g.get_sparse_range()
            return out
        finally:
            g.close()
            mem.free()
    return A.with_env(env, run)


def check(name, lib_path=None):
    cs = cases(lib_path is not None)[name]
    seqs, env, fused, knob, launches, oracle = cs + ("1", 0, True)[len(cs) - 3:]
    on = stage(seqs, dict(env, MPCGPU_FB_POST_FUSE=knob), lib_path)
    off = stage(seqs, dict(env, MPCGPU_FB_POST_FUSE="0"), lib_path)
    n = len(seqs) * (len(seqs) - 1) // 2
    assert on["pairs"] == off["pairs"] == n
    assert off["fused"] == 0 and not off["bins"], (off["fused"], off["bins"])
    assert on["post_launches"] >= launches and off["post_launches"] >= launches, (on["post_launches"], off["post_launches"], launches)
    if fused == "rule":
        # every pair here runs in the chain kernel, in the bin of its row sequence (the first of the pair)
        want_fused = rule_pairs(seqs, on["bins"])
        assert on["fused"] == want_fused, (on["fused"], want_fused, on["bins"], n)
        if lib_path is None:  # the device: seven rows per lane do not fit the sweeps' registers, some bin of the others does
            assert 0 < on["fused"] < n and 7 not in on["bins"], (on["fused"], n, on["bins"])
        else:                 # the emulator has neither registers nor scratch memory: every bin
            assert on["fused"] == n, (on["fused"], n)
    elif fused == "all":
        assert on["fused"] == n, (on["fused"], n)
    elif fused == "some":
        assert 0 < on["fused"] < n, (on["fused"], n)
    else:
        assert on["fused"] == 0, on["fused"]
    assert np.array_equal(on["nnz"], off["nnz"]), "nnz"
    assert np.array_equal(P.bits(on["ea"]), P.bits(off["ea"])), "EA bits"
    assert on["shard"] == off["shard"], "packed records (rowcnt, colcnt, ent, row, tperm) differ between the fused and the separate finishing"
    if not oracle:
        return
    (want,), want_ea = P.run_oracle(seqs, iters=0)
    assert np.array_equal(P.bits(on["ea"]), P.bits(want_ea)), "EA against the oracle"
    assert len(on["store"]) == len(want)
    for k, ((o1, v1), (o2, v2)) in enumerate(zip(on["store"], want)):
        assert np.array_equal(o1, o2) and np.array_equal(v1, v2), ("pair", k, "against the oracle")


def check_default(lib_path=None):
    """unset: nothing is fused. 2: the rule (a bin is fused where its workgroup stays as often resident and uses no scratch memory) —
    whatever it chooses, the shard is the one of the separate launch"""
    seqs = family(H23, 39)
    dflt = stage(seqs, {}, lib_path)
    rule = stage(seqs, {"MPCGPU_FB_POST_FUSE": "2"}, lib_path)
    off = stage(seqs, {"MPCGPU_FB_POST_FUSE": "0"}, lib_path)
    assert dflt["fused"] == 0 and not dflt["bins"]
    assert rule["fused"] == rule_pairs(seqs, rule["bins"]), (rule["fused"], rule["bins"])
    for got in (dflt, rule):
        assert got["shard"] == off["shard"] and np.array_equal(P.bits(got["ea"]), P.bits(off["ea"]))
    return rule["fused"]
