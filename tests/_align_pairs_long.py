"""mpcgpu_align_pairs beyond the row-list limit: pair lists that do not fit post_rows_kernel (stage A then finishes with the sort-based
post_kernel and the dense posteriors are built from the RAW candidate lists: kernels_aln.h dense_post_raw_kernel) and matrices wider
than calc_aln_kernel's LDS rows (calc_aln_tiled_kernel). Shared by tests/test_emu_align_pairs_long.py (small sequences forced onto
the route) and tests/test_gpu_align_pairs_long.py (real sizes, and the forced cases once more). Every comparison is 0 ulp against
tests/_align_pairs.py ap_oracle: path string, score bits, EA bits, get_list_sparse offsets and values.

The forcing value. mpcgpu_stage_a.inc post_rows_fits() counts 8 * MPCGPU_POST_SORT_CAP bytes for the row-list kernel's sorted list:
20 000 entries alone exceed its 150 KB, so no list fits and every general-path call takes the raw route (post_kernel's own LDS sort
buffer is min(next_pow2(candidate room), 32 768) entries: 64 KB for the 520-residue sequences here, fill_post()). MPCGPU_PAIRS_SMALL=0 keeps the short-list path (which never reads
the knob) out of the way. MPCGPU_ALN_TILE lowers the columns per tile of calc_aln_tiled_kernel so that matrices of ~100 columns
cross several tile edges.

A scenario is one context and a list of calls; a child process runs it with MPCGPU_TRACE=1 and prints, per call, the markers
"CALL k" ... "PASS k" / "FAIL k message" ... "END" around the library's trace lines. The parent (check()) asserts, per call:
  the result           PASS (oracle bits, and the launch counters below) in the child
  raw route            one "[mpcgpu] align_pairs dense posteriors from raw candidates: N pairs" line per chunk, N = the chunk's pairs;
                       launch counter buildpost_gen (the family the raw build is timed under) = chunks — resp. no line, 0
  alignment kernels    the "calc_aln LX x LY: <kernel>" lines list exactly the pairs of chunks that are not all one-wave, with the
                       kernel run_calc_aln (mpcgpu_joins.inc) must choose for that size and MPCGPU_ALN_KERNEL
  row blocks           "fb row blocks: H=" present exactly when a pair has LX >= long_min
  refusal              MpcGpuError naming mpcgpu_align_pairs and both lengths; no stage-A or alignment line
TEST INFRASTRUCTURE."""
import os
import subprocess
import sys
import traceback

import numpy as np

import _align_pairs as A
from muscle_amd._lib import MpcGpu, MpcGpuError

FORCE = {"MPCGPU_POST_SORT_CAP": "20000", "MPCGPU_PAIRS_SMALL": "0"}
RAW_LINE = "[mpcgpu] align_pairs dense posteriors from raw candidates: "
TILED = "rows in LDS, column tiles"
INT_MAX = 2 ** 31 - 1


def aln_kernel(LX, LY, env, aln_waves):
    """run_calc_aln's choice (mpcgpu_joins.inc); aln_waves: MPC_ALN_THREADS / 64 of the build (16 on the device, 2 on the emulator)"""
    pick = A.env_int(env, "MPCGPU_ALN_KERNEL", 0)
    W = LY + 1
    if A.one_wave(LX, LY) and pick in (0, 1):
        return A.WAVE
    if (W + 255) // 256 * 64 <= 1024 and pick in (0, 2):
        return A.QUAD
    if pick == 4 or (2 * W + aln_waves + 4) * 4 > A.LDS_BYTES:
        return TILED
    return A.LDSROWS


def raw_route(lens, env):
    return not A.post_rows_ok(lens, env)


class Call:
    def __init__(self, what, pairs, env=None, mega=False, refused=False, sparse=None, expf=None):
        self.what, self.pairs, self.env, self.mega, self.refused = what, list(pairs), dict(env or {}), mega, refused
        self.sparse = sparse  # None: every pair; else the pairs to read (long pairs: each read costs a stage)
        self.expf = expf      # set_hmm's expf_variant before the call: "host" (the oracle's) or "other" (then the reference is the row-list route)


class Scenario:
    def __init__(self, name, seqs, calls, mega_seed=None):
        self.name, self.seqs, self.calls = name, seqs, calls
        self.mega_seed = mega_seed

    def lens(self, call):
        return [(len(self.seqs[x]), len(self.seqs[y])) for x, y in call.pairs]


def forced(env=None):
    e = dict(FORCE)
    e.update(env or {})
    return e


def small_scenarios():
    """the forced-route cases: small related sequences, the whole table on the emulator and once more on the device"""
    out = []
    tile = {"MPCGPU_ALN_KERNEL": "4", "MPCGPU_ALN_TILE": "37"}
    # letters; the 6 x 520 pair keeps the chunk from being all one-wave, so every pair's alignment goes through run_calc_aln and
    # MPCGPU_ALN_KERNEL decides its kernel: the default choice, the tiled kernel (tiles of 37 columns), the LDS rows
    seqs = A.related([20, 64, 130, 90, 45, 6, 520, 1], 201)
    pairs = [(0, 1), (2, 3), (3, 2), (4, 0), (1, 4), (5, 6), (7, 2), (2, 7), (2, 2)]
    out.append(Scenario("letters", seqs, [Call("default alignment kernels", pairs, forced()),
                                          Call("MPCGPU_ALN_KERNEL=4, tiles of 37", pairs, forced(tile)),
                                          Call("MPCGPU_ALN_KERNEL=4, one tile", pairs, forced({"MPCGPU_ALN_KERNEL": "4"})),
                                          Call("MPCGPU_ALN_KERNEL=3", pairs, forced({"MPCGPU_ALN_KERNEL": "3"})),
                                          Call("the row-list route after it", pairs, {"MPCGPU_PAIRS_SMALL": "0"})]))
    # row blocks with one row per lane: 16-bit keys in the candidate lists
    knob = {"MPCGPU_FB_LONG_MIN": "65", "MPCGPU_FB_LONG_H": "1"}
    seqs = A.related([130, 70, 64, 25, 520], 202)
    pairs = [(0, 3), (1, 0), (2, 1), (3, 0), (0, 4), (0, 0)]
    out.append(Scenario("row_blocks", seqs, [Call("16-bit keys", pairs, forced(knob)),
                                             Call("16-bit keys, tiles of 37", pairs, forced(dict(knob, **tile)))]))
    # Mega profiles, then letters on the same context
    seqs = A.related([70, 30, 110, 1, 45, 520], 203)
    pairs = [(0, 1), (2, 0), (3, 4), (4, 2), (1, 5)]
    out.append(Scenario("mega", seqs, [Call("Mega", pairs, forced(), mega=True), Call("Mega, tiles of 37", pairs, forced(tile), mega=True),
                                       Call("letters after", pairs, forced())], mega_seed=7))
    # both expf variants: the host's (= the oracle's) must be bit-identical through the raw builder's own mpc_score_to_prob
    seqs = A.related([90, 80, 40, 520], 204)
    pairs = [(0, 1), (1, 2), (2, 3)]
    # (the other variant is within 1 ulp of the oracle, not on it: its raw route is compared with its own row-list route)
    out.append(Scenario("expf", seqs, [Call("host expf variant", pairs, forced(), expf="host"), Call("the other expf variant", pairs, forced(), expf="other")]))
    # more than 256 pairs: two chunks (256 + 44)
    seqs = A.related([14] * 14 + [30, 520], 205)
    rng = np.random.default_rng(5)
    pairs = [tuple(int(v) for v in rng.choice(15, 2, replace=False)) for _ in range(300)]
    pairs[17] = (14, 15)
    pairs[280] = (3, 14)  # (the second chunk is all one-wave: one batched alignment launch)
    out.append(Scenario("chunks", seqs, [Call("300 pairs", pairs, forced(), sparse=[299, 5, 262, 0, 17, 280])]))
    # no scratch budget: stage A serves one pair per batch, the chunk is halved down to one pair
    seqs = A.related([12] * 4 + [40, 520], 206)
    pairs = [(a, b) for a in range(6) for b in range(6) if a != b][:12]
    out.append(Scenario("halving", seqs, [Call("12 pairs", pairs, forced({"MPCGPU_SCRATCH_GB": "0"}), sparse=[11, 3])]))
    # regrowth: 1024 candidates do not hold a poly-A pair's list: the attempts that overflowed must leave nothing behind
    seqs = ["A" * 130, "A" * 100, "A" * 520]
    out.append(Scenario("regrowth", seqs, [Call("poly-A", [(0, 1), (1, 0), (1, 2)], forced({"MPCGPU_CAND_PER_ROW": "1"}))]))
    return out


SMALL_NAMES = [s.name for s in small_scenarios()]


def sched_scenario():
    """what the thread-order runs (EMU_SCHED=reverse / random) repeat: both new kernels, several tiles"""
    s = small_scenarios()
    sc = next(x for x in s if x.name == "letters")
    return Scenario("sched", sc.seqs, sc.calls[1:2])


def gpu_scenario():
    """real sizes, one context (tests/test_gpu_align_pairs_long.py lists what each call is for)"""
    lens = [12200, 12200, 300, 20000, 2, 15000, 60000, 6000, 400, 380, 410, 395, 20800, 20800]
    seqs = A.related(lens, 301)
    one = lambda what, p, **kw: Call(what, [p], {}, sparse=[0], **kw)
    calls = [one("12200 x 12200", (0, 1)), one("300 x 20000", (2, 3)), one("20000 x 300", (3, 2)), one("2 x 15000", (4, 5)),
             one("15000 x 2", (5, 4)), one("300 x 60000", (2, 6)),
             Call("a long pair among ordinary ones", [(8, 9), (2, 3), (10, 11), (9, 8)], {}, sparse=[0, 3]),
             one("20800 x 20800: outside the envelope", (12, 13), refused=True), Call("valid after the refusal", [(8, 9), (11, 10)], {})]
    return Scenario("long", seqs, calls)


def gpu_wide_scenario():
    """6000 x 60000 (row blocks, 16-bit keys, column tiles), the same registry, a context of its own: at 60 000 columns the float
    forward / backward sums of the reference carry several log units of rounding, 48 M of the pair's 360 M cells pass the threshold
    (the oracle says the same), and the one-wave sort of post_kernel over such a list takes minutes — kept apart so that the other
    calls do not wait for it"""
    sc = gpu_scenario()
    return Scenario("long_wide", sc.seqs, [Call("6000 x 60000", [(7, 6)], {}, sparse=[0])])


GPU_CALLS = [c.what for c in gpu_scenario().calls]


def scenario(name):
    if name == "long":
        return gpu_scenario()
    if name == "long_wide":
        return gpu_wide_scenario()
    if name == "sched":
        return sched_scenario()
    return next(s for s in small_scenarios() if s.name == name)


# ---- the child ----------------------------------------------------------------------------------------------------------------
def run_scenario(sc, lib_path=None):
    import _oracle as O
    h, (s, t, m, i, thr) = A.hmm()
    g = MpcGpu(0, lib_path)
    mega = None if sc.mega_seed is None else A.with_mega(sc.seqs, sc.mega_seed)
    try:
        g.set_hmm(s, t, m, i, thr)
        g.set_seqs_registry(sc.seqs)
        g.timers_enable(True)
        mega_on = False
        for k, call in enumerate(sc.calls):
            print("CALL %d" % k, flush=True)
            try:
                if call.expf is not None:
                    fma = 1 if O.lib().orc_host_expf_uses_fma() else 0
                    g.set_hmm(s, t, m, i, thr, fma if call.expf == "host" else 1 - fma)
                if call.mega != mega_on:
                    if call.mega:
                        g.set_mega(mega["alpha"], mega["weight"], mega["lp"], mega["mx"], mega["profs"])
                    else:
                        g.set_mega(None, None, None, None, None)
                    mega_on = call.mega
                _run_call(g, sc, call, mega if call.mega else None)
                print("PASS %d" % k, flush=True)
            except Exception:  # the next call still runs: one context, one process
                sys.stderr.flush()
                print("FAIL %d %s" % (k, traceback.format_exc().replace("\n", " | ")[-1500:]), flush=True)
            sys.stderr.flush()
            print("END", flush=True)
    finally:
        g.close()
    print("OK scenario", flush=True)


def _run_call(g, sc, call, mega):
    lens = sc.lens(call)
    xs, ys = [x for x, _ in call.pairs], [y for _, y in call.pairs]
    g.timers_reset()

    def run():
        try:
            return g.align_pairs(xs, ys), None
        except MpcGpuError as e:
            return None, str(e)
    res, err = A.with_env(call.env, run)
    sys.stderr.flush()
    if call.refused:
        LX, LY = lens[0]
        assert LX * LY * 5 + 100 > INT_MAX, "the pair is inside the envelope"
        assert res is None and "mpcgpu_align_pairs" in err and str(LX) in err and str(LY) in err and str(INT_MAX) in err, ("refusal", err)
        return
    assert err is None, err
    tm = g.timers_get()
    chunks = A.chunks_of(len(lens), call.env)
    raw = raw_route(lens, call.env)
    if A.env_int(call.env, "MPCGPU_SCRATCH_GB", 32) != 0:  # (the halving stages of the first chunk do not reach the dense build)
        assert tm["buildpost_gen"][1] == (len(chunks) if raw else 0), ("raw dense builds", tm["buildpost_gen"], len(chunks), raw)
    want_aln = sum(1 if all(A.one_wave(*l) for l in lens[q0:q0 + nq]) else nq for q0, nq in chunks)
    assert tm["calc_aln"][1] == want_aln, ("launches of calc_aln", tm["calc_aln"], want_aln)
    if call.expf == "other":  # the row-list route of the same variant: same matrix bits, so same paths, scores and records
        rows_env = {k: v for k, v in call.env.items() if k != "MPCGPU_POST_SORT_CAP"}
        assert not raw_route(lens, rows_env)
        recs = A.with_env(call.env, lambda: [A.list_sparse(g, q, lens[q][0]) for q in range(len(xs))])
        res2, err2 = A.with_env(rows_env, run)
        assert err2 is None, err2
        recs2 = A.with_env(rows_env, lambda: [A.list_sparse(g, q, lens[q][0]) for q in range(len(xs))])
        for q in range(len(xs)):
            assert res[q][0] == res2[q][0] and A.bits(res[q][1]) == A.bits(res2[q][1]) and A.bits(res[q][2]) == A.bits(res2[q][2]), (q, "raw against rows")
            assert np.array_equal(recs[q][0], recs2[q][0]) and np.array_equal(recs[q][1], recs2[q][1]), (q, "get_list_sparse, raw against rows")
        return
    wants = [A.oracle_pair(sc.seqs, x, y, mega) for x, y in call.pairs]
    for q, ((p, score, ea), w) in enumerate(zip(res, wants)):
        assert p == w["path"], (q, call.pairs[q], "path")
        assert A.bits(score) == A.bits(w["score"]) and A.bits(ea) == A.bits(w["ea"]), (q, call.pairs[q], "score / EA", score, w["score"], ea, w["ea"])

    def sparse():
        for q in (call.sparse if call.sparse is not None else range(len(xs))):
            off, val = A.list_sparse(g, q, len(sc.seqs[xs[q]]))
            assert np.array_equal(off, wants[q]["off"]) and np.array_equal(val, wants[q]["val"]), (q, call.pairs[q], "get_list_sparse")
    A.with_env(call.env, sparse)


# ---- the parent ---------------------------------------------------------------------------------------------------------------
def run_child(name, lib_path=None, timeout=1500, extra_env=None):
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MPCGPU_TRACE="1", PYTHONPATH=os.path.dirname(here) + os.pathsep + here)
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, "-u", os.path.join(here, "_align_pairs_long.py"), name, lib_path or ""], env=env, cwd=here,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout, text=True)
    out = r.stdout
    keep = os.environ.get("MPCGPU_TEST_KEEP_OUTPUT")  # a directory: the child's whole output (trace lines with the kernels' times) is kept there
    if keep:
        with open(os.path.join(keep, "align_pairs_long_%s.log" % name), "w") as f:
            f.write(out)
    assert r.returncode == 0 and "OK scenario" in out, "exit %d\n%s" % (r.returncode, out[-4000:])
    sc = scenario(name)
    parts = out.split("CALL ")[1:]
    assert len(parts) == len(sc.calls), (name, len(parts))
    return sc, [p.split("\nEND\n", 1)[0] for p in parts]


def check_call(sc, k, part, aln_waves):
    """call k of the scenario from its part of the child's output"""
    call = sc.calls[k]
    tag = (sc.name, k, call.what)
    verdict = [ln for ln in part.splitlines() if ln.startswith("PASS ") or ln.startswith("FAIL ")]
    assert verdict == ["PASS %d" % k], (tag, verdict or part[-2000:])
    lines = [ln for ln in part.splitlines() if ln.startswith("[mpcgpu]")]
    # (get_list_sparse stages pairs again: the lines of the align_pairs call end with its last alignment; a re-stage prints no
    # alignment and no dense-build line, so both lists below are the call's own)
    rawl = [int(ln[len(RAW_LINE):].split()[0]) for ln in lines if ln.startswith(RAW_LINE)]
    aln = [ln.split("calc_aln ", 1)[1] for ln in lines if ln.startswith("[mpcgpu] calc_aln ")]
    rb = [ln for ln in lines if ln.startswith("[mpcgpu] fb row blocks: H=")]
    if call.refused:
        assert not lines, (tag, "device work before the refusal", lines[:4])
        return
    lens = sc.lens(call)
    chunks = A.chunks_of(len(lens), call.env)
    assert rawl == ([nq for _, nq in chunks] if raw_route(lens, call.env) else []), (tag, "raw dense builds", rawl)
    want_aln = []
    for q0, nq in chunks:
        sub = lens[q0:q0 + nq]
        if not all(A.one_wave(*l) for l in sub):
            want_aln += ["%d x %d: %s" % (LX, LY, aln_kernel(LX, LY, call.env, aln_waves)) for LX, LY in sub]
    if call.expf == "other":  # the same list once more on the row-list route
        want_aln += want_aln
    assert aln == want_aln, (tag, "calc_aln kernels", aln[:8], want_aln[:8])
    lm = A.long_min_of(call.env)
    assert bool(rb) == any(LX >= lm for LX, _ in lens), (tag, "row blocks", rb[:2])


def check(name, lib_path=None, aln_waves=16, extra_env=None, timeout=1500):
    sc, parts = run_child(name, lib_path, timeout, extra_env)
    for k in range(len(sc.calls)):
        check_call(sc, k, parts[k], aln_waves)


if __name__ == "__main__":
    run_scenario(scenario(sys.argv[1]), sys.argv[2] or None)
