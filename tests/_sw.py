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
NBINS = 10  # mpcgpu_sw_bins: bins 1 .. 8 = rows per lane, bin 9 = the row-block kernel (index 0 unused)
LONG_BIN = 9
# drop-in sets: name -> (sequences, family length, seed, extra arguments of -super7)
DROPIN_SETS = {"swx_12x40": (12, 40, 21, []), "swx_20x30_b6": (20, 30, 22, ["-shrub_size", "6"]),
               "swx_8x560_b4": (8, 560, 23, ["-shrub_size", "4"])}
# ... cut to these lengths (before the X): as row sequences the row-block kernel twice and the bins 2, 3, 5, 6 and 8; the last sequence
# is a column only
DROPIN_CUTS = {"swx_8x560_b4": [550, 110, 530, 180, 300, 360, 450, 480]}


def dropin_seqs(name, terminated=True):
    n, L, seed, _ = DROPIN_SETS[name]
    fam = make_family(n, L, seed=seed)
    if name in DROPIN_CUTS:
        assert all(len(s) >= c for s, c in zip(fam, DROPIN_CUTS[name])), [len(s) for s in fam]
        fam = [s[:c] for s, c in zip(fam, DROPIN_CUTS[name])]
    return [s + ("X" if terminated else "") for s in fam]


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
LONG_CHAIN_LENS = [600, 40, 513, 70, 1025, 33, 520]
# column sequences of "long_chain_separators": the run the rows are swept against first, and a second run whose separators fall on
# columns 63, 128 and 193 of the item (63, 64 and 65 modulo 64: the last column of a 64-column chunk and the first two of the next)
SEPARATOR_RUNS = ([1, 1, 2, 63, 64, 65, 1, 130], [63, 64, 64, 1, 1, 62])


def separator_columns(run):
    """columns of the separators on the column axis of an item that holds the sequences of these lengths"""
    out, at = [], 0
    for L in run:
        at += L
        out.append(at)
        at += 1
    return out


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
    if name in ("long_chains", "long_chains_cols1", "long_chains_batch4"):
        # all pairs of long and short rows in turn: the row-block items hold 6, 4 and 2 pairs (one each with one column sequence per item;
        # batches of 4 pairs cut the chains)
        base = _rand(1025, 61)
        seqs = [_mutate(base[:L], 300 + L) for L in LONG_CHAIN_LENS]
        env = {"long_chains": {}, "long_chains_cols1": {"MPCGPU_SW_CHAIN_COLS": "1"}, "long_chains_batch4": {"MPCGPU_SW_BATCH": "4"}}[name]
        return seqs, None, None, env
    if name.startswith("long_chain_separators"):
        # a row sequence of several row blocks against two runs of consecutive column sequences: the separator columns of the first run
        # lie back to back and behind sequences of 63, 64 and 65 columns, those of the second at columns 63, 64 and 65 of a 64-column
        # chunk of the item's column axis. The row sequence once below and once above its columns in the set.
        LA = {"": 1025, "_513": 513, "_1024": 1024, "_1536": 1536}[name[len("long_chain_separators"):]]
        base = _rand(1536, 62)
        row = _mutate(base[:LA], 63)
        cols = [_mutate(base[40 * k:40 * k + L], 400 + k) for k, L in enumerate(SEPARATOR_RUNS[0] + SEPARATOR_RUNS[1])]
        n0, n1 = len(SEPARATOR_RUNS[0]), len(SEPARATOR_RUNS[1])
        hi = 1 + n0 + n1
        run0, run1 = list(range(1, 1 + n0)), list(range(1 + n0, hi))
        return [row] + cols + [row], [0] * n0 + [hi] * n0 + [0] * n1 + [hi] * n1, run0 + run0 + run1 + run1, {}
    if name == "long_5000":  # device only
        base = _rand(5000, 51)
        return [base, _mutate(base, 52, 0.4)], [0], [1], {}
    if name == "long_30x20000":  # device only
        base = _rand(20000, 53)
        return [_mutate(base[9000:9030], 54), base], [0, 1], [1, 0], {}
    raise KeyError(name)


CASES = ["len_1_2", "no_positive_cell", "wildcards", "lower_and_other_bytes", "identical", "lane_bins", "row_blocks", "ragged_all_pairs",
         "batch_cut", "chain_cut", "explicit_list", "long_chains", "long_chains_cols1", "long_chains_batch4", "long_chain_separators",
         "long_chain_separators_513", "long_chain_separators_1024", "long_chain_separators_1536"]
GPU_ONLY = ["long_5000", "long_30x20000"]


def pair_list(n, s1=None, s2=None):
    """the pairs of a call: the lists, or all pairs i < j in InitPairs order"""
    if s1 is None:
        return [(i, j) for i in range(n) for j in range(i + 1, n)]
    return [(int(a), int(b)) for a, b in zip(s1, s2)]


_REF_MEMO = {}


def want_scores(seqs, s1=None, s2=None, tab=None):
    """sw_ref of every pair of the call, computed once per distinct (row sequence, column sequence, tables): big lists are built from
    few distinct sequences. tab = (key, letter_of_char, sub, open, ext) or None for the reference's tables."""
    key, args = (None, ()) if tab is None else (tab[0], tab[1:])
    pairs = pair_list(len(seqs), s1, s2)
    out = np.zeros(len(pairs), np.float32)
    for q, (i, j) in enumerate(pairs):
        k = (seqs[i], seqs[j], key)
        if k not in _REF_MEMO:
            _REF_MEMO[k] = sw_ref(seqs[i], seqs[j], *args)
        out[q] = _REF_MEMO[k]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    seqs, s1, s2, _ = case(name)
    return want_scores(seqs, s1, s2)


def predict(lens, s1=None, s2=None, env=None):
    """The plan of mpcgpu_sw_scores (mpcgpu_sw.inc) restated from its rule. The list is cut into batches of MPCGPU_SW_BATCH pairs
    (2^24). Inside a batch a pair joins the item before it when it has the same row sequence, its column sequence is the next one of
    the set (y == previous y + 1) and the item's columns (every column sequence and its separator) stay within MPCGPU_SW_CHAIN_COLS
    (8192); otherwise it opens an item, and an item never crosses a batch. An item's bin is the rows per lane of its row sequence,
    ceil(L / 64) for L <= 512, and bin 9 (the row-block kernel) beyond.
    -> items: per bin, summed over the batches; batches; long_items; chains: (batch, bin, row sequence, pairs, columns) per item in
    list order; batch_items: per batch the items of every bin."""
    env = env or {}
    batch_cap = max(1, int(env.get("MPCGPU_SW_BATCH", 1 << 24)))
    chain_cols = max(1, int(env.get("MPCGPU_SW_CHAIN_COLS", 8192)))
    pairs = pair_list(len(lens), s1, s2)
    chains, batch_items = [], []
    for nb, q0 in enumerate(range(0, len(pairs), batch_cap)):
        cur, prev_y = None, None
        count = [0] * NBINS
        for x, y in pairs[q0:q0 + batch_cap]:
            cols = int(lens[y]) + 1
            if cur is not None and cur[2] == x and y == prev_y + 1 and cur[4] + cols <= chain_cols:
                cur[3] += 1
                cur[4] += cols
            else:
                lx = int(lens[x])
                cur = [nb, (lx + LANE - 1) // LANE if lx <= BLOCK_ROWS else LONG_BIN, x, 1, cols]
                chains.append(cur)
                count[cur[1]] += 1
            prev_y = y
        batch_items.append(count)
    items = [sum(b[k] for b in batch_items) for k in range(NBINS)]
    return {"items": items, "batches": len(batch_items), "long_items": items[LONG_BIN], "chains": [tuple(c) for c in chains],
            "batch_items": batch_items}


def check_plan(g, pr, tag=""):
    """sw_info() and sw_bins() of the last call against the restated plan: the items of every bin exactly; the workgroups of a bin
    between one per batch that has items of the bin and one per four items (the library takes the smaller of that and a multiple of
    the device's CUs, which the plan does not know)"""
    info = g.sw_info()
    items, groups = g.sw_bins()
    assert list(items) == pr["items"], (tag, items, pr["items"])
    assert info[2] == pr["batches"] and info[3] == sum(pr["items"]) and info[4] == pr["long_items"], (tag, info, pr["items"], pr["batches"])
    for b in range(NBINS):
        lo = sum(1 for c in pr["batch_items"] if c[b])
        hi = sum((c[b] + 3) // 4 for c in pr["batch_items"])
        assert lo <= groups[b] <= hi, (tag, b, groups, lo, hi)
    return items, groups


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
        check_plan(g, predict([len(x) for x in gd["seqs"]]), "golden")
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
        # the routes: every bin's items as the restated plan has them
        pr = predict([len(x) for x in seqs], s1, s2, env)
        items, groups = check_plan(g, pr, name)
        if name == "lane_bins":  # every sw_kernel<H, false> was launched, the row-block kernel was not
            assert all(items[h] >= 1 and groups[h] >= 1 for h in range(1, 9)) and items[LONG_BIN] == 0 and groups[LONG_BIN] == 0, (items, groups)
        if name == "row_blocks":
            assert items[LONG_BIN] == 6 and groups[LONG_BIN] >= 1, (items, groups)
        if name == "long_chains":
            assert sorted(c[3] for c in pr["chains"] if c[1] == LONG_BIN) == [2, 4, 6] and items[LONG_BIN] == 3, pr["chains"]
        if name == "long_chains_cols1":
            assert items[LONG_BIN] == 12 and sum(items) == len(want), items
        if name.startswith("long_chain_separators"):
            assert items[LONG_BIN] == 4 and sum(items) == 4, items
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


# ---- a wave that takes a second item ------------------------------------------------------------------------------------------
QUEUE_CUS = 304  # the lists of size "gpu" give every wave of a device of up to this many CUs a second item


def queue_reuse_bin1(n):
    """all pairs of n sequences of 3 .. 8 residues (twelve distinct ones in turn), one pair per item: n (n - 1) / 2 items of bin 1"""
    distinct = [_rand(3 + k % 6, 80 + k) for k in range(12)]
    return [distinct[k % 12] for k in range(n)], None, None, {"MPCGPU_SW_CHAIN_COLS": "1"}


def queue_reuse_long(count):
    """count items of the row-block bin, none a chain: item q pairs row sequence q mod 6 (513 .. 530 residues) with column sequence q mod 8
    (4 and 90 residues in turn), so the row sequence changes from every item to the next and neighbouring items differ in their columns"""
    base = _rand(530, 90)
    rows = [_mutate(base[:L], 500 + L) for L in (513, 516, 520, 523, 527, 530)]
    cols = [_mutate(base[100 + k:100 + k + (4, 90)[k % 2]], 600 + k) for k in range(8)]
    return rows + cols, [q % 6 for q in range(count)], [6 + q % 8 for q in range(count)], {}


def queue_reuse_sizes(size, lib_path=None):
    """-> (sequences of the bin-1 list, items of the row-block list). "gpu": for up to QUEUE_CUS CUs — more than 8 x 4 x 304 = 9 728
    items of bin 1 and more than 2 x 4 x 304 = 2 432 of the row-block bin. "emu": the smallest lists for the CUs the emulator reports,
    read from the workgroups of a first call whose (items + 3) / 4 lies above the grid's limit of 8 per CU."""
    if size == "gpu":
        return 150, 2600
    seqs, s1, s2, env = queue_reuse_bin1(24)
    g = context(seqs, lib_path)
    try:
        got = _with_env(env, lambda: g.sw_scores(s1, s2))
        assert np.array_equal(bits(got), bits(want_scores(seqs, s1, s2)))
        items, groups = g.sw_bins()
    finally:
        g.close()
    assert items[1] == 276 and groups[1] < 69 and groups[1] % 8 == 0, ("the first call did not reach the grid's limit", items, groups)
    cus = groups[1] // 8
    n = 2
    while n * (n - 1) // 2 <= 4 * 8 * cus:
        n += 1
    return n, 4 * 2 * cus + 1


def check_queue_reuse(size, lib_path=None):
    n, count = queue_reuse_sizes(size, lib_path)
    for what, b, (seqs, s1, s2, env) in (("bin 1", 1, queue_reuse_bin1(n)), ("row blocks", LONG_BIN, queue_reuse_long(count))):
        want = want_scores(seqs, s1, s2)
        g = context(seqs, lib_path)
        try:
            got = _with_env(env, lambda: g.sw_scores(s1, s2))
            bad = np.nonzero(bits(got) != bits(want))[0]
            assert len(bad) == 0, (what, bad[:10], got[bad[:10]], want[bad[:10]])
            items, groups = check_plan(g, predict([len(x) for x in seqs], s1, s2, env), what)
            assert items[b] == len(want) and sum(items) == len(want), (what, items)
            # four waves per workgroup: more items than waves, so at least one wave went back to the queue and took a second item
            assert items[b] > 4 * groups[b], "%s: %d items for %d workgroups of 4 waves — no wave is certain to have taken a second item " \
                "(a device of more than %d CUs needs longer lists)" % (what, items[b], groups[b], QUEUE_CUS)
        finally:
            g.close()


# ---- tables other than BLOSUM62 / -11 / -1 -----------------------------------------------------------------------------------
TABLES = [(1, 0.0, 0.0, True), (32, -0.3, -0.7, True), (4, -2.5, 0.0, False), (20, 0.0, -1.0, True), (20, -1.0, -11.0, True)]  # alpha, open, ext, symmetric


@functools.lru_cache(maxsize=None)
def table_case(k):
    """-> (tab = (key, letter_of_char, sub, open, ext), sequences) for TABLES[k]: a seeded random substitution table with a positive
    diagonal, byte 'A' + l for letter l and the wildcard for every other byte, sequences of 5, 70, 130, 600 and 31 letters 0 .. alpha
    (the wildcard included)"""
    alpha, op, ex, symmetric = TABLES[k]
    rng = np.random.default_rng(700 + k)
    sub = rng.uniform(-5.0, 3.0, (alpha, alpha)).astype(np.float32)
    if symmetric:
        sub = np.triu(sub) + np.triu(sub, 1).T
    sub[np.diag_indices(alpha)] = np.abs(sub[np.diag_indices(alpha)]) + np.float32(0.5)
    loc = np.full(256, alpha, np.uint8)
    loc[ord("A"):ord("A") + alpha] = np.arange(alpha)
    chars = [chr(ord("A") + l) for l in range(alpha)] + ["~"]
    seqs = ["".join(chars[int(l)] for l in rng.integers(0, alpha + 1, L)) for L in (5, 70, 130, 600, 31)]
    sub.setflags(write=False)
    return ("table%d" % k, loc, sub, op, ex), seqs


def check_tables(lib_path=None):
    """one context, one table after the other: every call scores with the tables set last"""
    g = None
    try:
        for k, (alpha, op, ex, symmetric) in enumerate(TABLES):
            tab, seqs = table_case(k)
            if g is None:
                g = context(seqs, lib_path, scores=False)
            else:
                g.set_seqs_registry(seqs)
            g.sw_set_scores(*tab[1:])
            n = len(seqs)
            lists = [(None, None)]
            if not symmetric:  # score(A, B) != score(B, A): the transposed list too
                pairs = pair_list(n)
                lists.append(([j for i, j in pairs], [i for i, j in pairs]))
            for s1, s2 in lists:
                got = g.sw_scores(s1, s2)
                want = want_scores(seqs, s1, s2, tab)
                bad = np.nonzero(bits(got) != bits(want))[0]
                assert len(bad) == 0, (TABLES[k], s1 is None, bad[:10], got[bad[:10]], want[bad[:10]])
                check_plan(g, predict([len(x) for x in seqs], s1, s2), TABLES[k])
        # back to the first table on the same context and the same sequences
        tab = table_case(0)[0]
        g.sw_set_scores(*tab[1:])
        assert np.array_equal(bits(g.sw_scores()), bits(want_scores(seqs, None, None, tab)))
    finally:
        if g is not None:
            g.close()


# ---- reuse of a context -------------------------------------------------------------------------------------------------------
def check_context_reuse(lib_path=None):
    """sets of fewer, more and longer sequences in turn on one context, through mpcgpu_set_seqs_registry and through mpcgpu_set_seqs:
    a call with a row-block bin after one without and the reverse; the buffers of the larger call stay"""
    fam = make_family(12, 64, seed=71)
    A = [s[:L] for s, L in zip(fam, [60, 7, 33, 58, 1, 45, 60, 12, 29, 51, 3, 40])]
    base = _rand(700, 72)
    B = [_mutate(base[:80], 73), base, _mutate(base[300:330], 74), _mutate(base[100:300], 75)]
    s, t, m, i, thr = G.hmm_tables()
    g = MpcGpu(0, lib_path)
    try:
        g.set_hmm(s, t, m, i, thr)
        g.sw_set_scores(*tables())
        first = None
        for setter in (g.set_seqs_registry, g.set_seqs):
            for seqs in (A, B, A):
                setter(seqs)
                got = g.sw_scores()
                want = want_scores(seqs)
                bad = np.nonzero(bits(got) != bits(want))[0]
                assert len(bad) == 0, (setter.__name__, len(seqs), bad[:10], got[bad[:10]], want[bad[:10]])
                items, _ = check_plan(g, predict([len(x) for x in seqs]), (setter.__name__, len(seqs)))
                assert (items[LONG_BIN] > 0) == (seqs is B), items
                if seqs is A:  # the bits of the first call, whatever ran in between
                    first = got.copy() if first is None else first
                    assert np.array_equal(bits(got), bits(first))
    finally:
        g.close()


# ---- beside the posterior stage -----------------------------------------------------------------------------------------------
def check_beside_the_stage(lib_path=None):
    """mpcgpu_sw_scores between mpcgpu_build_store and the relax iterations: shard, store and values are what the oracle has, the store
    epoch moves as on a context without the call, and the scores are the restatement's"""
    import _parity as P
    seqs = make_family(8, 50, seed=77)
    want = P.run_oracle(seqs, iters=2)
    s, t, m, i, thr = G.hmm_tables()

    def run(with_sw):
        g = MpcGpu(0, lib_path)
        try:
            g.set_hmm(s, t, m, i, thr)
            g.set_seqs(seqs)
            g.calc_posteriors()
            g.build_store()
            epochs = [g.store_epoch()]
            scores = None
            if with_sw:
                g.sw_set_scores(*tables())
                scores = g.sw_scores()
                assert g.store_epoch() == epochs[0]
                check_plan(g, predict([len(x) for x in seqs]), "beside the stage")
            ea = g.get_ea().copy()
            stages, nnz = [g.get_sparse_range()], [g.get_nnz().copy()]
            for _ in range(2):
                g.cons_iter()
                epochs.append(g.store_epoch())
                g.cons_commit()
                epochs.append(g.store_epoch())
                stages.append(g.get_sparse_range())
                nnz.append(g.get_nnz().copy())
            return stages, ea, nnz, epochs, scores
        finally:
            g.close()
    stages, ea, nnz, epochs, scores = run(True)
    P.assert_same((stages, ea), want, "store and values around mpcgpu_sw_scores")
    for st, z in zip(want[0], nnz):
        assert [len(v) // 2 for _, v in st] == z.tolist()
    assert np.array_equal(bits(scores), bits(want_scores(seqs)))
    stages0, ea0, nnz0, epochs0, _ = run(False)
    assert epochs == epochs0 and epochs[-1] > epochs[0], (epochs, epochs0)
    P.assert_same((stages0, ea0), want, "the same context without the call")
