"""The LONG form of the record store and of relax_band_kernel (kernels_store.h: 32-bit block distances and entry positions;
MpcRbLongCxx, kernels_relaxb.h) against the oracle, bit for bit. Shared by tests/test_gpu_relax_long.py (MI355X) and
tests/test_emu_relax_long.py (the same source on the emulator). Runs go through tests/_relax.py's run_store: EA, the store after
the build and after each of two iterations (mpcgpu_get_sparse_range) equal P.run_oracle's, 0 ulp; relax_info names the path.

What the inputs are claimed to be is asserted from the oracle's matrices (check_forced_claims, record_blocks), and for the field-width
cases (FIELD: dist_hi, col_high, col_8000, maxlen) from record_layout, a numpy restatement of where var_build_long_kernel puts every block and
entry: tests/test_relax_long_table.py holds those claims, no device. The further paths of the long form (grid-stride trips, split
ranges, batched and wide joins, partial stores, form changes on one context) are the check_* functions below, shared by
tests/test_gpu_relax_long_paths.py and tests/test_emu_relax_long_paths.py.
TEST INFRASTRUCTURE."""
import functools

import numpy as np

import _joins as J
import _relax as R
from muscle_amd._lib import MpcGpu
from muscle_amd.synth import make_family
import _golden as G

LONG = ("band-long", "relax_band_kernel", "MpcRbLongCxx")
FORCE = {"MPCGPU_RELAX_LONG": "1"}


@functools.lru_cache(None)
def forced_seqs(n):
    """n sequences of ragged lengths 5 .. 120: a family (rows store cells), one sequence of ONE residue, and one unrelated
    sequence (pairs with rows that store no cell)"""
    fam = make_family(n, 120, seed=20 + n)
    lens = [120, 5, 47, 88, 13, 101, 64, 29, 117][:n]
    seqs = [s[:ln] for s, ln in zip(fam, lens)]
    seqs[1] = seqs[0][40:41]                              # 1 residue
    if n >= 5:
        seqs[3] = make_family(1, 88, seed=77)[0][:88]      # unrelated to the family
    else:
        seqs[2] = make_family(1, 47, seed=77)[0][:47]
    return tuple(seqs)


def check_forced_claims(seqs):
    st = R.oracle(seqs)[0][0]
    assert min(len(s) for s in seqs) == 1 and max(len(s) for s in seqs) <= 120 and min(len(s) for s in seqs[2:]) >= 5
    assert any(len(v) > 0 and any(o[i + 1] == o[i] for i in range(len(o) - 1)) for o, v in st), "no pair with a row that stores no cell"
    assert any(any(o[i + 1] - o[i] > 2 for i in range(len(o) - 1)) for o, v in st), "no row with an overflow block"


def record_blocks(seqs):
    """largest record of the store in 16-byte blocks: len(A) + sum over rows of max(ceil(count / 2) - 1, 0), both orientations"""
    st = R.oracle(seqs)[0][0]
    n = len(seqs)
    best, k = 0, 0
    for x in range(n):
        for y in range(x + 1, n):
            o, v = st[k]
            k += 1
            rows = np.diff(np.asarray(o, np.int64))
            cols = np.bincount(np.asarray(v[1::2], np.int64), minlength=len(seqs[y]))
            for ln, cnt in ((len(seqs[x]), rows), (len(seqs[y]), cols)):
                best = max(best, ln + int(np.maximum((cnt + 1) // 2 - 1, 0).sum()))
    return best


def run(seqs, env, has=(), lacks=(), fallback=False, lib_path=None, store=(), store_not=()):
    """one store under env: build, two iterations, everything against the oracle; relax_info after each iteration"""
    r = R.Run("long form", seqs, env, store=store, store_not=store_not, it=R.both(has=has, lacks=lacks, fallback=fallback))
    cs = R.Case("long", [r])
    g = MpcGpu(0, lib_path)
    try:
        g.set_hmm(*G.hmm_tables())
        g.timers_enable(True)
        return R.run_store(g, cs, 0, r, marks=False)
    finally:
        g.close()


def check_join(seqs, env, lib_path=None):
    """mpcgpu_build_post / mpcgpu_align_alns(_w) on a fixed bipartition (odd against even sequences: both stored orientations) after
    two iterations on a store built under env: the row form of BuildPost reads the block records (launch counters 1/0/0), matrix,
    path and score equal the restatement + the oracle's CalcAlnFlat"""
    def body():
        ctx = J.Ctx(list(seqs), lib_path)
        try:
            info, fb = ctx.g.relax_info()
            j = ctx.join(list(range(1, len(seqs), 2)), list(range(0, len(seqs), 2)), np.random.default_rng(5))
            ctx.check(j, "row", what="join over the long form")
            return info, fb
        finally:
            ctx.close()
    return J.with_env(dict(env), body)


# ---- where the long form puts things (kernels_store.h: var_build_long_kernel, the two scans and the entry loop) -----------------
def record_layout(o, v, LA, fwd):
    """the record (A, Z) of one stored pair (X, Y), X < Y, from its sparse matrix (o: row offsets, v: value / column words): fwd = A is
    X (the record's rows are the matrix's rows), else A is Y (its rows are the matrix's columns). var_build_long_kernel statement by
    statement. Per row of A: cnt, nb (blocks), ovf0 (block at which its overflow blocks start: LA + ovf_before[r]; its first block is
    block r) and dist (bytes from its first block to its second, 0 where it has one block). Per entry, in the matrix's stored order:
    col (the stored column), unit and slot, db (the distance its block carries, bytes), pos = unit * 2 + slot (pos_f / pos_t)"""
    o = np.asarray(o, np.int64)
    col = np.asarray(v[1::2], np.int64)
    row = np.repeat(np.arange(len(o) - 1), np.diff(o))
    nnz = len(col)
    if fwd:
        r, c, rank = row, col, np.arange(nnz)
    else:  # tperm: the entry's rank in the row-major order of the transpose
        order = np.lexsort((row, col))
        rank = np.empty(nnz, np.int64)
        rank[order] = np.arange(nnz)
        r, c = col, row
    cnt = np.bincount(r, minlength=LA)
    nb = (cnt + 1) // 2
    vo = np.maximum(nb - 1, 0)
    s_start, s_ovf = np.cumsum(cnt) - cnt, np.cumsum(vo) - vo  # the two exclusive scans
    within = rank - s_start[r]
    j, slot = within // 2, within % 2
    ovf0 = LA + s_ovf
    unit = np.where(j == 0, r, ovf0[r] + j - 1)
    delta = np.where(j + 1 < nb[r], np.where(j == 0, ovf0[r] - r, 1), 0)
    return dict(cnt=cnt, nb=nb, ovf0=ovf0, dist=np.where(nb > 1, (ovf0 - np.arange(LA)) * 16, 0), col=c, unit=unit, slot=slot,
                db=delta * 16, pos=unit * 2 + slot, blocks=LA + int(vo.sum()))


def record_words(lay, LA):
    """the third and fourth word of every block of the record, as var_build_long_kernel writes them"""
    w = np.full((lay["blocks"], 2), 0xffff, np.int64)  # MPC_PADL_SENTINEL
    u, s, c, db = lay["unit"], lay["slot"], lay["col"], lay["db"]
    w[u[s == 0], 0] = c[s == 0] | ((db[s == 0] << 16) & 0xffffffff)
    w[u[s == 1], 1] = c[s == 1] | (db[s == 1] & 0xffff0000)
    odd = np.ones(lay["blocks"], bool)  # blocks that hold one entry repeat its column, distance 0
    odd[u[s == 1]] = False
    one = (s == 0) & odd[u]
    w[u[one], 1] = c[one]
    return w


def layouts(seqs):
    """record_layout of every ordered pair (A, Z), A != Z, of the store: {(A, Z): layout}"""
    st = R.oracle(seqs)[0][0]
    n, k, out = len(seqs), 0, {}
    for x in range(n):
        for y in range(x + 1, n):
            o, v = st[k]
            k += 1
            out[(x, y)] = record_layout(o, v, len(seqs[x]), True)
            out[(y, x)] = record_layout(o, v, len(seqs[y]), False)
    return out


def field_counts(seqs):
    """what a store of these sequences holds, by field: rows by the upper half of their first block's distance (hi0 / hi1 / hi2: rows
    of two and more blocks with dist.hi 0, 1, >= 2; *_lo: those of them with dist.lo != 0), stored columns by range, entry positions
    from 65 536 on, rows of three and more blocks, rows without a cell"""
    c = dict.fromkeys(("hi0", "hi0_lo", "hi1", "hi1_lo", "hi2", "hi2_lo", "col_lt_1fff", "col_1fff", "col_1fff_7fff", "col_7fff", "col_8000",
                       "col_gt_8000", "pos_ge_65536", "rows_3_blocks", "rows_empty", "max_blocks"), 0)
    for (A, Z), lay in layouts(seqs).items():
        many = lay["nb"] > 1
        hi, lo = lay["dist"] >> 16, lay["dist"] & 0xffff
        for name, sel in (("hi0", hi == 0), ("hi1", hi == 1), ("hi2", hi >= 2)):
            c[name] += int((many & sel).sum())
            c[name + "_lo"] += int((many & sel & (lo != 0)).sum())
        col = lay["col"]
        c["col_lt_1fff"] += int((col < 0x1fff).sum())
        c["col_1fff"] += int((col == 0x1fff).sum())
        c["col_1fff_7fff"] += int(((col > 0x1fff) & (col <= 0x7fff)).sum())
        c["col_7fff"] += int((col == 0x7fff).sum())
        c["col_8000"] += int((col == 0x8000).sum())
        c["col_gt_8000"] += int((col > 0x8000).sum())
        c["pos_ge_65536"] += int((lay["pos"] >= 65536).sum())
        c["rows_3_blocks"] += int((lay["nb"] >= 3).sum())
        c["rows_empty"] += int((lay["cnt"] == 0).sum())
        c["max_blocks"] = max(c["max_blocks"], lay["blocks"])
    return c


# ---- the field-width cases: no knob, the library's own trigger decides ------------------------------------------------------------
POLY = "A"


def _with_stretches(length, seed, stretches):
    """a random sequence of `length` residues with low-complexity stretches [(at, residues[, letter])] written over it"""
    base = make_family(1, 4500, seed=seed)[0]
    s = (base * (length // len(base) + 1))[:length]
    for at, ln, *letter in stretches:
        s = s[:at] + (letter[0] if letter else POLY) * ln + s[at + ln:]
    assert len(s) == length
    return s


UNRELATED = 9  # make_family(1, 70, seed=9): the unrelated sequence of tests/_relax.py's base()


@functools.lru_cache(None)
def field_seqs(name):
    """dist_hi: 9000 positions with low-complexity stretches of 60 at rows 100, 2500 and 8165 (the last across column 8191), three
    partners of 60, 80 and 100 of the same letter, one unrelated sequence of 70.
    col_high: 40 000 positions, a stretch of 60 at 32 740 (across column 32 767 / 32 768) and one of 90 of ANOTHER letter at 39 900 (a
    partner of the same letter would put all its weight on the longer stretch), a partner of each, one unrelated.
    (The reference's float32 posteriors keep no cell of a stretch further than some 700 positions from the end of a sequence this long,
    so 40 000 positions cannot hold cells at column 32 768.)
    col_8000: 33 000 positions, a stretch of 60 at 32 740: columns 0x7fff and 0x8000 and both sides of them; a partner of 60, one unrelated
    sequence and a fragment of three residues.
    maxlen / over: 65 534 / 65 535 positions of ONE residue (G) with low-complexity stretches of 60 at row 100 and of 40 at 65 480,
    partners of 40, 55 and 30 residues. The background is chosen from the reference's arithmetic, not from the library's: with a
    sequence of mixed composition the float32 forward / backward sums of the reference keep nearly every cell of a pair from about
    50 000 positions on (`dense`), a row of a record (short, long) then holds some 60 000 entries = 480 KB, and no band tile can hold
    it in 160 KB of LDS whatever the cutter does; against a glycine background the posteriors stay sparse (rows of at most 32 entries).
    dense: 65 534 positions of mixed composition, a stretch of 40 at 65 480, a partner of 40 and a fragment of three residues (two
    short partners keep the case at a third of the cells): what such a store does instead."""
    other = make_family(1, 70, seed=UNRELATED)[0]
    if name == "dist_hi":
        return (_with_stretches(9000, 101, ((100, 60), (2500, 60), (8165, 60))), POLY * 60, POLY * 80, POLY * 100, other)
    if name == "col_high":
        return (_with_stretches(40000, 103, ((32740, 60), (39900, 90, "Q"))), POLY * 60, "Q" * 90, other)
    if name == "dist_hi_small":  # (the emulator's size: stretches at rows 40 and 4100 of 4200, dist.hi 1 and 0)
        return (_with_stretches(4200, 101, ((40, 60), (4100, 60))), POLY * 60, other[:30])
    if name == "col_8000":
        return (_with_stretches(33000, 103, ((32740, 60),)), POLY * 60, other[:30], "MKV")
    if name in ("maxlen", "over"):
        ln = 65534 if name == "maxlen" else 65535
        long = "G" * ln
        for at, k in ((100, 60), (65480, 40)):
            long = long[:at] + POLY * k + long[at + k:]
        return (long, POLY * 40, POLY * 55, other[:30])
    if name == "dense":
        return (_with_stretches(65534, 105, ((65480, 40),)), POLY * 40, "MKV")
    raise KeyError(name)


# what each case must hold (tests/test_relax_long_table.py): counts that must be > 0
# (col_high keeps its stretch at 32 740 and the partner of that stretch although the oracle stores no cell of them, field_seqs says
# why: the input is the one the case was specified with, and col_8000 carries the claims on 0x7fff and 0x8000 in its place)
FIELD = {
    "dist_hi": ("hi0", "hi0_lo", "hi1", "hi1_lo", "hi2", "hi2_lo", "col_1fff", "col_1fff_7fff", "rows_3_blocks", "rows_empty"),
    "col_high": ("hi0_lo", "col_gt_8000", "pos_ge_65536", "rows_3_blocks", "rows_empty"),
    "col_8000": ("hi0_lo", "col_1fff_7fff", "col_7fff", "col_8000", "col_gt_8000", "pos_ge_65536", "rows_3_blocks", "rows_empty"),
    "maxlen": ("hi2_lo", "col_gt_8000", "pos_ge_65536", "rows_3_blocks", "rows_empty"),
}
GATHER = ("CSR slabs", "kernel=relax_kernel")


def check_field(name, lib_path=None, join=True):
    """one field-width case with no knob: store, two committed iterations and EA equal the oracle's on the long form by the library's
    own trigger; then joins in both group orders. The row reader of the records (build_post_rows_long_kernel) reads the record
    (S in MSA 1, T in MSA 2) by the rows of S and needs C2 <= 1024, so it reads the records (long, short): the 32-bit distances.
    With the long sequence in MSA 2 (C2 > 1024) the dispatcher takes the general path, which reads the packed matrices; that order
    is run and asserted as such. So the column decode of the row reader never meets a column above 1023: the columns at 0x1fff,
    0x7fff, 0x8000 and above are read by the relax and the commit only.
    dist_hi: the join by rows has 512 < C2 <= 1024, for which the host code launches build_post_rows_long_kernel<16> on a long store
    (mpcgpu_joins.inc). The launch counters count the row form as one family, 1/0/0, and do not tell <8> from <16>: the width and
    the long store are asserted, the template argument follows from the dispatch and is not observed."""
    seqs = field_seqs(name)
    n = len(seqs)
    run(seqs, {}, has=LONG, lacks=GATHER, fallback=False, store=("band-long",), lib_path=lib_path)
    if not join:
        return
    ctx = J.Ctx(list(seqs), lib_path)
    try:
        info, fb = ctx.g.relax_info()
        assert "band-long" in info and "MpcRbLongCxx" in info and not fb, info
        rng = np.random.default_rng(7)
        kw = {"C2": 600} if name == "dist_hi" else {}  # > 512 columns: build_post_rows_long_kernel<16>
        j = ctx.join([0, n - 1], list(range(1, n - 1)), rng, **kw)
        assert (j.C2 > 512) == (name == "dist_hi") and j.C2 <= J.ROW_C2, j.C2
        ctx.check(j, "row", what="%s: rows of the long record" % name)
        j = ctx.join(list(range(1, n - 1)), [0, n - 1], rng)
        assert j.C2 > J.ROW_C2
        ctx.check(j, "general", what="%s: the long sequence in MSA 2" % name)
    finally:
        ctx.close()


def check_over(lib_path=None):
    """65 535 positions: stage A takes the pair (mpcgpu_stage_a.inc refuses from MPC_KEY_COL_MASK_LONG + 1 = 65 536 on: `LXlong >
    65535`), build_var_store returns "does not fit" for a sequence above MPC_RL_MAXLEN = 65 534, and the store falls to the gather
    layout: CSR slabs, relax_kernel, is_fallback == 1, values equal the oracle's. Decided from the code; no refusal to assert."""
    run(field_seqs("over"), {}, has=GATHER, lacks=("band-long", "relax_band_kernel"), fallback=True, store=("CSR slabs",), store_not=("band-long",), lib_path=lib_path)


def check_dense(lib_path=None):
    """65 534 positions of mixed composition (field_seqs: dense): the store is built in the long form, no band tile holds a row of
    some 60 000 entries, so the first relax falls to the CSR slabs (relax_kernel, is_fallback == 1) and stays there; store, both
    iterations and EA equal the oracle's"""
    seqs = field_seqs("dense")
    st = R.oracle(seqs)[0][0]
    widest = max(int(np.bincount(np.asarray(v[1::2], np.int64)).max()) for _, v in st[:2])
    assert widest * 8 > 160 * 1024, widest  # one row of a record (short, long): 8 bytes an entry against the LDS of a CU
    run(seqs, {}, has=GATHER, lacks=("relax_band_kernel",), fallback=True, store=("band-long",), lib_path=lib_path)


# ---- the further paths of the long form, forced at small shapes ------------------------------------------------------------------
def stride_n(cus):
    """sequences for n * n >= 2 * min(n * n, 4 * cus): EVERY workgroup of var_build_long_kernel's grid builds a second record on the
    scratch it has used (n * n > 4 * cus alone gives only the first n * n - 4 * cus workgroups a second trip)"""
    n = 3
    while n * n < 8 * cus:
        n += 1
    return n


@functools.lru_cache(None)
def stride_seqs(n):
    """n sequences of ragged lengths 8 .. 40 of one family, one of ONE residue and one unrelated"""
    fam = make_family(n, 40, seed=61)
    seqs = [s[:8 + (7 * k) % 33] for k, s in enumerate(fam)]
    seqs[1] = seqs[0][3:4]
    seqs[n // 2] = make_family(1, 40, seed=77)[0][:31]
    return tuple(seqs)


def check_stride(cus, lib_path=None):
    n = stride_n(cus)
    seqs = stride_seqs(n)
    assert n * n > 4 * cus and n * n >= 8 * cus, (n, cus)
    lens = sorted(len(s) for s in seqs)
    assert lens[0] == 1 and lens[1] >= 8 and lens[-1] <= 40, lens
    st = R.oracle(seqs)[0][0]
    assert any(len(v) and (np.diff(o) == 0).any() for o, v in st) and any((np.diff(o) > 2).any() for o, v in st)
    run(seqs, FORCE, has=LONG, lacks=("window records",) + GATHER, fallback=False, store=("band-long",), lib_path=lib_path)
    return n


def range_scripts(npairs):
    """split ranges before one commit, an uneven explicit split, the empty range beside a full one, and a second iteration split
    differently from the first: [(script, launches per iteration)]"""
    k = 7
    assert 0 < k < npairs // 2
    return [([["lo", "hi"], [(0, k), (k, npairs)]], (2, 2)),
            ([[None, "empty"], ["empty", (0, npairs - k), (npairs - k, npairs)]], (1, 2)),
            ([[(0, 1), (1, 2), (2, npairs)], ["hi", "lo"]], (3, 2))]


def check_ranges(lib_path=None):
    """commit_pairs_long_kernel after relaxes in pieces (the e0 / e1 clipping of entries relaxed by another launch), on forced_seqs(9)"""
    seqs = forced_seqs(9)
    npairs = len(seqs) * (len(seqs) - 1) // 2
    g = MpcGpu(0, lib_path)
    try:
        g.set_hmm(*G.hmm_tables())
        g.timers_enable(True)
        for q, (script, launches) in enumerate(range_scripts(npairs)):
            r = R.Run("ranges %d" % q, seqs, FORCE, script=script, store=("band-long",), win=False,
                      it=[dict(has=LONG, fallback=False, win=False, launches=ln) for ln in launches])
            R.run_store(g, R.Case("long_ranges", [r]), q, r, marks=False)
    finally:
        g.close()


def check_joins(lib_path=None):
    """joins over a forced long store: three joins in one batch (build_post_rows_batch_long_kernel<8>), plain and weighted single joins
    under MPCGPU_BP=rows and =sort (the sort path reads the packed matrices: equal bytes whatever the form), and one join with
    C2 > 512 from gap columns (build_post_rows_long_kernel<16>)"""
    seqs = list(forced_seqs(9))

    def body():
        ctx = J.Ctx(seqs, lib_path)
        try:
            info, fb = ctx.g.relax_info()
            assert "band-long" in info and "MpcRbLongCxx" in info and not fb, info
            rng = np.random.default_rng(11)
            joins = [ctx.join([0, 3, 5], [1, 2, 6], rng), ctx.join([8, 2], [0, 7], rng), ctx.join([4, 1, 7], [6, 3], rng), ctx.join([5], [2, 8, 0], rng)]
            chunks, single = ctx.check_batch(joins, what="batch over the long form")
            assert len(chunks) == 1 and len(chunks[0]) >= 3 and not single, (chunks, single)
            for j in joins[:2]:
                ctx.check(j, "row", mode="rows", what="MPCGPU_BP=rows")
                ctx.check(j, "general", mode="sort", what="MPCGPU_BP=sort")
                for w in ((None, None), (j.w1, j.w2)):
                    posts = [J.with_env({"MPCGPU_BP": m}, lambda: ctx.g.build_post(*j.args(), *w).copy()) for m in ("rows", "sort")]
                    assert np.array_equal(J.bits(posts[0]), J.bits(posts[1])), "rows and sort differ"
            wide = ctx.join([1, 4, 0], [7, 2, 5], rng, C2=600)
            assert 512 < wide.C2 <= J.ROW_C2
            ctx.check(wide, "row", what="C2 > 512 over the long form")
        finally:
            ctx.close()
    J.with_env(dict(FORCE), body)


def form_case():
    """short (window records) -> long -> short with a smaller n -> long with a larger n -> short, on ONE context, each relaxed twice;
    relax_info of every store equals that of a fresh context (R.run_case with fresh=True): d_pos grows for the 32-bit positions,
    pad_long moves pos_t, the window records of the earlier store are released"""
    N = R.narrow()
    big = tuple(make_family(11, 90, seed=57))
    short = dict(store=("band index", "+ window records"), store_not=("band-long",), win=True)
    lng = dict(store=("band-long",), store_not=("window records",), win=False)
    return R.Case("long_forms", [
        R.Run("short", N, {}, it=R.both(has=(R.WIN,), lacks=("band-long", "MpcRbLong"), win=True, fallback=False), **short),
        R.Run("long, same sequences", N, FORCE, it=R.both(has=LONG, lacks=("window records",), win=False, fallback=False), **lng),
        R.Run("short, smaller n", N[:5], {}, it=R.both(has=(R.WIN,), lacks=("band-long", "MpcRbLong"), win=True, fallback=False), **short),
        R.Run("long, larger n", big, FORCE, it=R.both(has=LONG, lacks=("window records",), win=False, fallback=False), **lng),
        R.Run("short again", N, {}, it=R.both(has=(R.WIN,), lacks=("band-long", "MpcRbLong"), win=True, fallback=False), **short),
    ], fresh=True)


def check_forms(size, lib_path=None):
    R.run_case(form_case(), size, lib_path)
