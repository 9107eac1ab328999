"""sw_kernel (muscle_amd/csrc/kernels_sw.h: score-only Smith-Waterman for lists of pairs, the scores behind the guide tree of
`muscle -super7 in.fa`) — shared by tests/test_sw_table.py (the restatement against the compiled reference's bits),
tests/test_emu_sw.py (the emulator build) and tests/test_gpu_sw.py (the device). Every comparison is 0 ulp.

The reference's own SWFast_SMx (sw.cpp:142-275) dies in its trace-back when a pair's best cell lies in the last row or column
(sw.cpp:73-74), so its bits exist only for inputs where that cannot happen: the golden sequences (tests/golden/sw_scores.npz, written
by tests/golden/make_sw_golden.py from SWFast_Seqs_BLOSUM62 itself) all end in the wildcard X, which scores 0 — a cell of the last
row or column can equal but never exceed the running best. Everything else is checked against sw_ref below, a numpy float32
restatement of the recurrence that tests/test_sw_table.py pins to those bits.
TEST INFRASTRUCTURE."""
import functools
import os

import numpy as np

import _golden as G
from muscle_amd._lib import MpcGpu, MpcGpuError
from muscle_amd.synth import AMINO, make_family

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCORES = os.path.join(GOLDEN_DIR, "sw_scores.npz")
DROPIN = os.path.join(GOLDEN_DIR, "sw_dropin.json")

# kernels_sw.h: rows per lane up to MPC_SW_HMAX = 8 (a bin per 64 rows), row blocks of 512 rows beyond
LANE = 64
BLOCK_ROWS = 512
# drop-in sets: name -> (sequences, family length, seed, extra arguments of -super7)
DROPIN_SETS = {"swx_12x40": (12, 40, 21, []), "swx_20x30_b6": (20, 30, 22, ["-shrub_size", "6"])}


def dropin_seqs(name, terminated=True):
    n, L, seed, _ = DROPIN_SETS[name]
    return [s + ("X" if terminated else "") for s in make_family(n, L, seed=seed)]


def golden_input():
    """the sequences the golden scores are for: 36 related sequences cut to lengths 2 .. 300, each ending in X"""
    fam = make_family(36, 310, seed=17)
    rng = np.random.default_rng(5)
    lens = [1, 2, 3, 63, 64, 65, 127, 128, 129, 299] + [int(x) for x in rng.integers(4, 299, 26)]
    out = []
    for s, ln in zip(fam, lens):
        a = int(rng.integers(0, len(s) - ln))
        out.append(s[a:a + ln] + "X")
    return out


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(SCORES)
    return {"seqs": [str(s) for s in z["seqs"]], "scores": z["scores"], "letter_of_char": z["letter_of_char"], "sub": z["blosum62"],
            "open": float(z["open"]), "ext": float(z["ext"])}


def tables():
    g = golden()
    return g["letter_of_char"], g["sub"], g["open"], g["ext"]


def sw_ref(a, b, loc=None, sub=None, open_score=None, ext_score=None):
    """SWFast_SMx's score (sw.cpp:183-264) in numpy float32, one anti-diagonal at a time: every cell keeps its own chain of single
    adds and maxima (a row-wise vectorisation would re-associate the + Ext chain of I). Borders as the reference sets them:
    -9e9f, and 0 in M(0, 0) (sw.cpp:166-182, 260)."""
    t = tables()
    loc = t[0] if loc is None else loc
    sub = np.asarray(t[1] if sub is None else sub, np.float32)
    op = np.float32(t[2] if open_score is None else open_score)
    ex = np.float32(t[3] if ext_score is None else ext_score)
    alpha = sub.shape[0]
    la = np.asarray(loc, np.uint8)[np.frombuffer(a.encode() if isinstance(a, str) else bytes(a), np.uint8)].astype(np.int64)
    lb = np.asarray(loc, np.uint8)[np.frombuffer(b.encode() if isinstance(b, str) else bytes(b), np.uint8)].astype(np.int64)
    LA, LB = len(la), len(lb)
    subx = np.zeros((alpha + 1, alpha + 1), np.float32)  # a letter >= alpha scores 0 against everything (blosumsmx.cpp:46-49)
    subx[:alpha, :alpha] = sub
    la, lb = np.minimum(la, alpha), np.minimum(lb, alpha)
    NEG = np.float32(-9e9)
    zero = np.float32(0)
    # diagonal d holds the cells i + j = d, indexed by i + 1 (index 0 = the row above the matrix)
    M2 = np.full(LA + 1, NEG, np.float32)  # M outputs of diagonal d - 2
    M1 = np.full(LA + 1, NEG, np.float32)  # ... d - 1
    D1 = np.full(LA + 1, NEG, np.float32)
    I1 = np.full(LA + 1, NEG, np.float32)
    best = zero
    for d in range(LA + LB - 1):
        lo, hi = max(0, d - LB + 1), min(LA - 1, d)
        i = np.arange(lo, hi + 1)
        j = d - i
        mdiag = M2[i].copy()      # M output of cell (i - 1, j - 1); NEG outside the matrix
        if d == 0:
            mdiag[0] = zero       # float M0 = 0 (sw.cpp:182)
        din = D1[i]               # D output of cell (i - 1, j)
        iin = I1[i + 1]           # I output of cell (i, j - 1)
        x = np.maximum(np.maximum(mdiag, din), iin)
        x = np.where(zero >= x, zero, x) + subx[la[i], lb[j]]
        mo = mdiag + op
        dn = np.maximum(din + ex, mo)
        inn = np.maximum(iin + ex, mo)
        if len(x):
            best = max(best, np.float32(x.max()))
        M0 = np.full(LA + 1, NEG, np.float32)
        D0 = np.full(LA + 1, NEG, np.float32)
        I0 = np.full(LA + 1, NEG, np.float32)
        M0[i + 1], D0[i + 1], I0[i + 1] = x, dn, inn
        M2, M1, D1, I1 = M1, M0, D0, I0
    return np.float32(best)


# ---- the case table -----------------------------------------------------------------------------------------------------------
def _rand(L, seed, alphabet=AMINO):
    rng = np.random.default_rng(seed)
    return "".join(alphabet[int(k)] for k in rng.integers(0, len(alphabet), L))


def _mutate(s, seed, p=0.25):
    rng = np.random.default_rng(seed)
    return "".join(AMINO[int(rng.integers(0, 20))] if rng.random() < p else ch for ch in s)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (sequences, seq1, seq2 or None for all pairs, environment of the call)"""
    if name == "len_1_2":
        seqs = ["A", "W", "AW", "WA", "C", "WW"]
        return seqs, None, None, {}
    if name == "no_positive_cell":  # every letter pair scores below 0: exactly 0.0f
        return ["WWWW", "DDDDD", "W", "D"], [0, 2, 0], [1, 3, 3], {}
    if name == "wildcards":
        return ["XXXX", "XXXXXXX", "X", "AXA", "BZJUO*-"], None, None, {}
    if name == "lower_and_other_bytes":
        base = _rand(40, 3)
        return [base.lower(), _mutate(base, 4), base[:10] + " .-*1~" + base[10:].lower(), "\x01\x7f" + base[5:30]], None, None, {}
    if name == "identical":  # the best cell lies in the last row and column
        s = _rand(90, 8)
        return [s, s, s[:50], s[40:]], None, None, {}
    if name == "lane_bins":  # rows per lane x 64: lengths at and one either side of every bin boundary, as row and as column sequence
        base = _rand(BLOCK_ROWS + 2, 11)
        lens = sorted({h * LANE + d for h in range(1, 9) for d in (-1, 0, 1)} - {BLOCK_ROWS + 1})  # (513 rows: "row_blocks")
        seqs = [_mutate(base[:L], 100 + L) for L in lens]
        partner = len(seqs)
        seqs += [_mutate(base[:70], 7), _mutate(base[:200], 9)]
        s1 = list(range(partner)) + [partner] * partner
        s2 = [partner + 1] * partner + list(range(partner))
        return seqs, s1, s2, {}
    if name == "row_blocks":  # the row-block kernel: one block + 1 row, two blocks - 1, two, two + 1, and a third block of one lane
        base = _rand(2 * BLOCK_ROWS + 70, 12)
        lens = [BLOCK_ROWS + 1, 2 * BLOCK_ROWS - 1, 2 * BLOCK_ROWS, 2 * BLOCK_ROWS + 1, 2 * BLOCK_ROWS + 65]
        seqs = [_mutate(base[:L], 200 + L) for L in lens] + [_mutate(base[300:420], 5), _mutate(base[:BLOCK_ROWS], 6)]
        n = len(lens)
        return seqs, list(range(n)) + [n + 1, 0], [n] * n + [0, n + 1], {}
    if name == "ragged_all_pairs":  # 40 sequences of lengths 1 .. 300
        fam = make_family(40, 300, seed=31)
        rng = np.random.default_rng(32)
        lens = [1, 2, 300] + [int(x) for x in rng.integers(1, 300, 37)]
        return [s[:L] for s, L in zip(fam, lens)], None, None, {}
    if name == "batch_cut":  # batches of 7 pairs cut the chains of 12 sequences (66 pairs); chains of at most 100 columns
        return make_family(12, 45, seed=33), None, None, {"MPCGPU_SW_BATCH": "7", "MPCGPU_SW_CHAIN_COLS": "100"}
    if name == "chain_cut":  # the chain limit at exactly the columns of two pairs (46 + 1 each): two pairs chain, a third does not
        seqs = [_rand(46, 40 + k) for k in range(6)]
        return seqs, None, None, {"MPCGPU_SW_CHAIN_COLS": "94"}
    if name == "explicit_list":  # repeated pairs, i > j, i == j, runs that chain and runs that do not
        seqs = make_family(9, 60, seed=34)
        s1 = [3, 3, 3, 0, 8, 8, 2, 2, 2, 2, 5, 1, 1]
        s2 = [4, 5, 6, 0, 1, 1, 7, 8, 3, 4, 2, 0, 1]
        return seqs, s1, s2, {}
    if name == "long_5000":  # device only
        base = _rand(5000, 51)
        return [base, _mutate(base, 52, 0.4)], [0], [1], {}
    if name == "long_30x20000":  # device only
        base = _rand(20000, 53)
        return [_mutate(base[9000:9030], 54), base], [0, 1], [1, 0], {}
    raise KeyError(name)


CASES = ["len_1_2", "no_positive_cell", "wildcards", "lower_and_other_bytes", "identical", "lane_bins", "row_blocks", "ragged_all_pairs",
         "batch_cut", "chain_cut", "explicit_list"]
GPU_ONLY = ["long_5000", "long_30x20000"]


@functools.lru_cache(maxsize=None)
def expected(name):
    seqs, s1, s2, _ = case(name)
    if s1 is None:
        pairs = [(i, j) for i in range(len(seqs)) for j in range(i + 1, len(seqs))]
    else:
        pairs = list(zip(s1, s2))
    memo = {}
    out = np.zeros(len(pairs), np.float32)
    for q, (i, j) in enumerate(pairs):
        if (i, j) not in memo:
            memo[(i, j)] = sw_ref(seqs[i], seqs[j])
        out[q] = memo[(i, j)]
    out.setflags(write=False)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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


def context(seqs, lib_path=None, scores=True):
    s, t, m, i, thr = G.hmm_tables()
    g = MpcGpu(0, lib_path)
    g.set_hmm(s, t, m, i, thr)
    g.set_seqs_registry(seqs)
    if scores:
        g.sw_set_scores(*tables())
    return g


def check_golden(lib_path=None):
    gd = golden()
    g = context(gd["seqs"], lib_path)
    try:
        got = g.sw_scores()
        assert np.array_equal(bits(got), bits(gd["scores"])), np.nonzero(bits(got) != bits(gd["scores"]))[0][:10]
        n = len(gd["seqs"])
        info = g.sw_info()
        assert info[0] == n * (n - 1) // 2 and info[2] == 1 and info[4] == 0, info
        # symmetric in (A, B): the transposed list gives the same bits
        s1 = [j for i in range(n) for j in range(i + 1, n)]
        s2 = [i for i in range(n) for j in range(i + 1, n)]
        assert np.array_equal(bits(g.sw_scores(s1, s2)), bits(gd["scores"]))
    finally:
        g.close()


def check_case(name, lib_path=None):
    seqs, s1, s2, env = case(name)
    want = expected(name)
    g = context(seqs, lib_path)
    try:
        got = _with_env(env, lambda: g.sw_scores(s1, s2))
        bad = np.nonzero(bits(got) != bits(want))[0]
        assert len(bad) == 0, (name, bad[:10], got[bad[:10]], want[bad[:10]])
        info = g.sw_info()
        assert info[0] == len(want), info
        if name == "no_positive_cell":
            assert np.array_equal(bits(got), np.zeros(len(got), np.uint32))
        if name == "batch_cut":
            assert info[2] == (66 + 6) // 7, info
        if name == "chain_cut":  # 15 pairs; a chain holds two pairs of 47 columns each and not three
            assert info[3] == 3 + 2 + 2 + 1 + 1, info
        if name == "row_blocks":
            assert info[4] == 6, info
        if name in ("lane_bins", "ragged_all_pairs"):
            assert info[4] == 0, info
    finally:
        g.close()


def check_refusals(lib_path=None):
    seqs = ["ACDEFGHIKL", "ACDEFGHIKLMNPQRSTVWY" * 3277][:2]  # 10 and 65 540 residues
    assert len(seqs[1]) > 65535
    g = context(seqs + ["ACD" * 21845 + "A"], lib_path, scores=False)  # ... and 65 536
    try:
        def refused(fn, *words):
            try:
                fn()
            except MpcGpuError as e:
                assert all(w in str(e) for w in words), str(e)
                return
            raise AssertionError("accepted: %s" % (words,))
        refused(lambda: g.sw_scores([0], [0]), "mpcgpu_sw_scores", "mpcgpu_sw_set_scores")
        loc, sub, op, ex = tables()
        refused(lambda: g.sw_set_scores(loc, sub, 1.0, ex), "mpcgpu_sw_set_scores", "positive")
        refused(lambda: g.sw_set_scores(loc, np.zeros((40, 40), np.float32), op, ex), "mpcgpu_sw_set_scores", "alphabet")
        g.sw_set_scores(loc, sub, op, ex)
        refused(lambda: g.sw_scores([0], [2]), "mpcgpu_sw_scores", "65536", "65535")
        refused(lambda: g.sw_scores([1], [0]), "mpcgpu_sw_scores", "65540", "65535")
        refused(lambda: g.sw_scores(), "mpcgpu_sw_scores", "65535")
        refused(lambda: g.sw_scores([0], [3]), "mpcgpu_sw_scores", "out of range")
        # the context stays usable, and its store epoch where it was
        ep = g.store_epoch() if hasattr(g, "store_epoch") else None
        got = g.sw_scores([0], [0])
        assert bits(got)[0] == bits(sw_ref(seqs[0], seqs[0]))
        if ep is not None:
            assert g.store_epoch() == ep
    finally:
        g.close()
