"""Chains of structure-profile input (fb_chain_mega_kernel, MPCGPU_FB_CHAIN_MEGA) against the oracle, the bb11001 golden and the same
stage with MPCGPU_FB_CHAIN=0 (fb_kernel<H, true> alone). Shared by tests/test_gpu_mega_chains.py and tests/test_emu_mega_chains.py.

A scenario is a set of sequences with profiles (scenario()). run() performs one all-pairs stage A and the store of it on a fresh
context and returns EA, nnz, every pair's offsets and (probability bits, column) words, stage_a_info(), stage_a_chain_bins() and the
launch count of the forward/backward family. On the device every environment setting runs in a child process of its own (child():
this file as a script, under a time limit; MPCGPU_TRACE is read once per process) that leaves its results in a file and its trace
on stderr; a (scenario, environment) is run once per test process and shared. The emulator twin runs in process under with_env.

Lengths. T = ceil(LX / H) lanes own rows (H = ceil(LX / 64)); a pair chains when LY + 1 >= T. SYNTH holds 20 sequences in the bins
H = 1, 2 and 4, among them one of 250 residues (T = 63), one of 126 (T = 63), one of 62 (LY + 1 == 63: chains behind both) and one of
61 (LY + 1 < 63: cuts their chains and runs alone in fb_kernel). TEST INFRASTRUCTURE."""
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

import _golden as G
import _parity as P
from muscle_amd._lib import MpcGpu
from muscle_amd.synth import make_family

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 120  # seconds a child may take: a few seconds of work behind the start of Python and of the device

SYNTH = [250, 126, 40, 62, 200, 61, 64, 65, 128, 129, 256, 193, 100, 57, 70, 230, 33, 90, 150, 210]
N19 = [120, 60, 70, 64, 80, 90, 75, 66, 100, 110, 61, 85, 95, 72, 68, 105, 77, 88, 99]  # T(120) = 60: every partner chains: 16 + 2
ROWBLOCK = [100, 800, 90, 128, 70, 111]

ON = {"MPCGPU_FB_CHAIN_MEGA": "1"}
OFF = {"MPCGPU_FB_CHAIN": "0"}
GRADE0 = {"MPCGPU_FB_CHAIN_GRADE": "0"}


def cut(lengths, seed):
    fam = make_family(len(lengths), max(lengths), seed=seed)
    return [s[:n] for s, n in zip(fam, lengths)]


_SCEN = {}


def scenario(name):
    """-> (seqs, mega tables and profiles)"""
    if name not in _SCEN:
        if name == "bb11001":
            m = G.mega("mega_bb11001")
            _SCEN[name] = (m["seqs"], m)
        else:
            kind, nfeat = name.split("_f")
            lengths = {"synth": SYNTH, "n19": N19, "rowblock": ROWBLOCK}[kind]
            seqs = cut(lengths, seed=300 + len(lengths))
            _SCEN[name] = (seqs, P.random_mega(seqs, seed=40 + int(nfeat), nfeat=int(nfeat)))  # alphabets ragged across the features
    return _SCEN[name]


def lanes_t(LX):
    H = (LX + 63) // 64
    return (LX + H - 1) // H


def expected_chains(lengths, cmax=16, long_min=769):
    """(chained pairs, chains) of the all-pairs list when every bin chains, whole chains (MPCGPU_FB_CHAIN_GRADE=0) and room for every
    axis: build_chains of mpcgpu_stage_a.inc restated"""
    n, pairs, chains = len(lengths), 0, 0
    for i in range(n):
        if lengths[i] >= long_min:
            continue
        T, run = lanes_t(lengths[i]), 0
        for j in list(range(i + 1, n)) + [None]:
            if j is not None and lengths[j] + 1 >= T and run < cmax:
                run += 1
                continue
            if run >= 2:
                pairs, chains = pairs + run, chains + 1
            run = 1 if j is not None and lengths[j] + 1 >= T else 0
    return pairs, chains


def run(seqs, mega, lib_path=None, letters_after=False):
    """one stage A and its store on a fresh context -> dict. letters_after: then mpcgpu_set_mega(nfeat = 0) and the byte stage on the
    same context, under "letters" """
    s, t, m, i, thr = G.hmm_tables("hmm_amino")
    g = MpcGpu(0, lib_path)
    try:
        g.set_hmm(s, t, m, i, thr)
        g.set_seqs(seqs)
        if mega is not None:
            g.set_mega(mega["alpha"], mega["weight"], mega["lp"], mega["mx"], mega["profs"])
        out = _stage(g)
        if letters_after:
            g.set_mega(None, None, None, None, None)  # nfeat = 0: back to byte sequences
            out["letters"] = _stage(g)
        return out
    finally:
        g.close()


def _stage(g):
    g.timers_enable(True)
    g.timers_reset()
    g.calc_posteriors()
    out = {"info": g.stage_a_info(), "bins": sorted(g.stage_a_chain_bins()), "fb_launches": int(g.timers_get()["fb"][1]),
           "coop": g.stage_a_coop_info(), "ea": g.get_ea().copy(), "nnz": g.get_nnz().copy()}
    g.build_store()
    out["store"] = [(np.array(o), np.array(v)) for o, v in g.get_sparse_range()]
    return out


def same(tag, got, ea, store):
    """EA bits, nnz, offsets, columns and value bits of every pair"""
    assert np.array_equal(P.bits(got["ea"]), P.bits(ea)), (tag, "EA bits")
    assert len(got["store"]) == len(store), tag
    for k, ((o1, v1), (o2, v2)) in enumerate(zip(got["store"], store)):
        assert int(got["nnz"][k]) == int(o2[-1]), (tag, "pair", k, "nnz")
        assert np.array_equal(o1, o2), (tag, "pair", k, "offsets")
        assert np.array_equal(np.asarray(v1).view(np.uint32), np.asarray(v2).view(np.uint32)), (tag, "pair", k, "columns / value bits")


_ORACLE = {}


def oracle(name):
    """(store, EA) of the scenario's stage A on the oracle, once per process"""
    if name not in _ORACLE:
        seqs, mega = scenario(name)
        (st,), ea = P.run_oracle(seqs, iters=0, mega=mega)
        _ORACLE[name] = (st, ea)
    return _ORACLE[name]


# ---- a child process per environment setting ----------------------------------------------------------------------------------
_RUNS = {}
_STOP = []  # set when a child died of a signal or ran out of time: no further child is started on the device in this process


def child(what, env, lib_path=None):
    """`what` (a scenario name, or "letters:" / "msas:" + one) in a process of its own under `env` and CHILD_TIMEOUT
    -> (result, its [mpcgpu] trace lines); once per test process"""
    key = (what, tuple(sorted(env.items())), lib_path)
    if key in _RUNS:
        return _RUNS[key]
    assert not _STOP, "not started: an earlier child did not end in order (%s)" % _STOP[0]
    fd, path = tempfile.mkstemp(suffix=".pkl")
    os.close(fd)
    e = dict(os.environ, PYTHONPATH=os.path.dirname(HERE) + os.pathsep + HERE)
    for k in ("MPCGPU_FB_CHAIN_MEGA", "MPCGPU_FB_CHAIN", "MPCGPU_FB_CHAIN_MAX", "MPCGPU_FB_CHAIN_GRADE", "MPCGPU_TRACE"):
        e.pop(k, None)
    e.update(env)
    p = subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "_mega_chains.py"), what, path, lib_path or ""], env=e, cwd=HERE,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        text = p.communicate(timeout=CHILD_TIMEOUT)[0]
    except subprocess.TimeoutExpired:
        p.kill()
        text = p.communicate()[0]
        os.unlink(path)
        _STOP.append("%s under %s: time limit" % (what, env))
        raise AssertionError("%s under %s ran longer than %d s\n%s" % (what, env, CHILD_TIMEOUT, text[-3000:]))
    if p.returncode < 0 or p.returncode in (134, 139):
        _STOP.append("%s under %s: exit %d" % (what, env, p.returncode))
    try:
        assert p.returncode == 0, "%s under %s: exit %d\n%s" % (what, env, p.returncode, text[-3000:])
        with open(path, "rb") as f:
            res = pickle.load(f)
    finally:
        os.unlink(path)
    _RUNS[key] = (res, [ln for ln in text.splitlines() if ln.startswith("[mpcgpu]")])
    return _RUNS[key]


def trace_bins(lines, prefix):
    """{H: pairs} of the trace lines that begin with `prefix` ... H=<H> ... pairs=<n>"""
    out = {}
    for ln in lines:
        if ln.startswith(prefix):
            H = int(ln.split("H=", 1)[1].split()[0])
            out[H] = out.get(H, 0) + int(ln.split("pairs=", 1)[1].split()[0])
    return out


# ---- a pair list with profiles loaded: mpcgpu_align_msas ------------------------------------------------------------------------
MSAS_CHAINED = (7, 2)


def msas_case(name="synth_f8"):
    """12 pairs: eight in a row with one seq1, four scattered -> (registry, mega, arguments of align_msas, pairs); MSAS_CHAINED: what
    stage_a_info()[1:] says of it with whole chains"""
    import _buildpost as BP
    seqs, mega = scenario(name)
    rng = np.random.default_rng(23)
    # seq1 = 12: 100 residues, T = 50. Its eight partners in list order: 62, 64 (a chain of two), 40 (too short: alone in fb_kernel),
    # 65, 57, 90, 250, 200 (a chain of five)
    grp1, grp2 = [12, 8, 14], [2, 3, 6, 7, 13, 16, 17, 0, 4]
    rows1, C1 = BP.random_msa(seqs, grp1, rng)
    rows2, C2 = BP.random_msa(seqs, grp2, rng)
    pairs = [(0, b) for b in (1, 2, 0, 3, 4, 6, 7, 8)] + [(1, 3), (2, 0), (1, 8), (2, 5)]
    seq1, seq2 = [grp1[a] for a, b in pairs], [grp2[b] for a, b in pairs]
    m1, m2 = [BP.pos_to_col(rows1[a]) for a, b in pairs], [BP.pos_to_col(rows2[b]) for a, b in pairs]
    return seqs, mega, (seq1, seq2, m1, m2, C1, C2), pairs


def msas_restatement(name="synth_f8"):
    """the oracle per pair and the numpy restatement of buildposterior3flat.cpp:19-85 (tests/test_gpu_parity.py::
    test_align_msas_vs_restatement), with the emissions of the profiles -> (path, score, EA per pair)"""
    import _oracle as O
    seqs, mega, (seq1, seq2, m1, m2, C1, C2), pairs = msas_case(name)
    s, t, m, i, thr = G.hmm_tables()
    h = O.make_hmm(s, t, m, i)
    mg = O.make_mega(mega["alpha"], mega["weight"], mega["lp"], mega["mx"])
    post = np.zeros((C1, C2), np.float32)
    ea = []
    for q, (X, Y) in enumerate(zip(seq1, seq2)):
        LX, LY = len(seqs[X]), len(seqs[Y])
        Pd = O.post(O.fwd_mega(h, mg, mega["profs"][X], mega["profs"][Y]), O.bwd_mega(h, mg, mega["profs"][X], mega["profs"][Y]), LX, LY)
        ea.append(np.float32(O.aln_score(Pd)) / np.float32(min(LX, LY)))
        off, val = O.sparse_from_post(Pd)
        p, col = val[0::2].view(np.float32), val[1::2]
        for r in range(len(off) - 1):
            for k in range(off[r], off[r + 1]):
                post[m1[q][r], m2[q][col[k]]] += p[k]  # buildposterior3flat.cpp:81
    sc, path = O.calc_aln(post)
    return path, sc, np.array(ea, np.float32)


def run_msas(name, lib_path=None):
    seqs, mega, args, pairs = msas_case(name)
    s, t, m, i, thr = G.hmm_tables()
    g = MpcGpu(0, lib_path)
    try:
        g.set_hmm(s, t, m, i, thr)
        g.set_seqs_registry(seqs)
        g.set_mega(mega["alpha"], mega["weight"], mega["lp"], mega["mx"], mega["profs"])
        path, sc, ea = g.align_msas(*args)
        return {"path": path, "score": np.float32(sc), "ea": np.array(ea, np.float32), "info": g.stage_a_info(), "bins": sorted(g.stage_a_chain_bins())}
    finally:
        g.close()


if __name__ == "__main__":
    _what, _out, _lib = sys.argv[1], sys.argv[2], sys.argv[3] or None
    if _what.startswith("msas:"):
        _res = run_msas(_what[5:], _lib)
    else:
        _letters = _what.startswith("letters:")
        _seqs, _mega = scenario(_what[8:] if _letters else _what)
        _res = run(_seqs, _mega, _lib, letters_after=_letters)
        if _letters:
            _res["fresh"] = run(_seqs, None, _lib)
    sys.stderr.flush()
    with open(_out, "wb") as _f:
        pickle.dump(_res, _f)
    print("OK", flush=True)
