"""Custom pair orders (mpcgpu_set_pair_order) against the oracle: plain functions that take lib_path (None: the HIP library;
tests/emu/libmpcgpu_emu.so: the emulator build of the same sources), called by tests/test_emu_parity.py and, under
@pytest.mark.gpu, by tests/test_gpu_parity.py. The reference of every stage is _parity.run_oracle (bit for bit: EA, then offsets
and values of all three stages); the reference of positions is muscle_amd.mpcflat.position_pairs.

Run as a script (`python _pair_order.py reject CASE LIB`), it is the child process of the rejection tests: one invalid call on a
context that holds a finished run, which must be refused by name and change nothing (emulator only: on a GPU such calls reach
device memory out of bounds)."""
import ctypes as C
import os
import sys

import numpy as np

import _buildpost as BP
import _golden as G
import _oracle as O
import _parity as P
from muscle_amd._lib import MpcGpu, MpcGpuError, plan_partition
from muscle_amd.mpcflat import position_pairs
from muscle_amd.synth import make_family

# the relax kernels: the default band tiles, relax_var_kernel's two geometries (tests/test_emu_parity.py: VAR_PRIMARY / VAR_FALLBACK),
# the CSR slabs + gather kernel
RELAX_ENVS = [{}, {"MPCGPU_RELAX_TILES": "pairs"},
              {"MPCGPU_RELAX_TILES": "pairs", "MPCGPU_RELAX_LDS_KB": "1", "MPCGPU_RELAX_LDS_KB_1024": "160"},
              {"MPCGPU_RELAX": "gather"}]


class Env:
    """environment variables for the duration of a with block"""

    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class DevMem:
    """caller-owned device buffers: numpy arrays on the emulator (its "device" pointers are host pointers), hipMalloc on a GPU"""

    def __init__(self, lib_path):
        self.emu = lib_path is not None
        self.keep, self.ptrs = [], []
        if not self.emu:
            self.hip = None
            for name in ("libamdhip64.so.7", "libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
                try:
                    self.hip = C.CDLL(name)
                    break
                except OSError:
                    continue
            assert self.hip is not None
            self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            self.hip.hipFree.argtypes = [C.c_void_p]

    def alloc(self, nbytes):
        nbytes = max(int(nbytes), 16)
        if self.emu:
            a = np.zeros(nbytes, np.uint8)
            self.keep.append(a)
            return a.ctypes.data
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        self.ptrs.append(p.value)
        return p.value

    def free(self):
        """after every context that adopted one of the buffers is closed"""
        for p in self.ptrs:
            self.hip.hipFree(C.c_void_p(p))
        self.ptrs, self.keep = [], []


# ---- orders -------------------------------------------------------------------------------------------------------------
def random_order(n, rng, max_groups=4):
    """[0,n) cut into groups: a triangle per group, the rectangles between groups (some split by rows or by columns), shuffled"""
    k = int(rng.integers(1, min(n, max_groups) + 1))
    cuts = [0] + sorted(int(x) for x in rng.choice(np.arange(1, n), k - 1, replace=False)) + [n]
    groups = list(zip(cuts[:-1], cuts[1:]))
    rects = [[a, b, a, b] for a, b in groups]
    for i, (xa, xb) in enumerate(groups):
        for ya, yb in groups[i + 1:]:
            how = int(rng.integers(3))
            if how == 1 and xb - xa > 1:
                m = int(rng.integers(xa + 1, xb))
                rects += [[xa, m, ya, yb], [m, xb, ya, yb]]
            elif how == 2 and yb - ya > 1:
                m = int(rng.integers(ya + 1, yb))
                rects += [[xa, xb, ya, m], [xa, xb, m, yb]]
            else:
                rects.append([xa, xb, ya, yb])
    rng.shuffle(rects)
    return np.array(rects, np.uint32)


def fixed_orders(lens, lib_path, worlds=(2, 3, 8)):
    """name -> rectangles: the shapes a generator rarely makes, and mpcgpu_plan_partition's own (where it cuts blocks)"""
    n = len(lens)
    g1, g2 = n // 3, 2 * n // 3
    out = {
        "one triangle": [[0, n, 0, n]],
        "reverse rows": [[x, x + 1, x + 1, n] for x in range(n - 1, -1, -1)],  # (the last one, x = n - 1, is empty)
        # one-sequence triangles and empty rectangles (0 pairs) between the ones that hold the pairs
        "empty and one-sequence": [[0, 0, 0, n], [n, n, n, n]] + [r for x in range(n) for r in ([x, x + 1, x, x + 1], [x, x + 1, x + 1, n])]
        + [[n // 3, n // 3, n // 2, n], [1, n // 2, n, n]],
        "off-diagonal first": [[g1, g2, g2, n], [0, g1, g2, n], [0, g1, g1, g2], [g2, n, g2, n], [g1, g2, g1, g2], [0, g1, 0, g1]],
    }
    for world in worlds:
        rects, _ = plan_partition(lens, world, lib_path)
        if len(rects):
            out["plan_partition world %d" % world] = rects
    return {k: np.array(v, np.uint32).reshape(-1, 4) for k, v in out.items()}


def new_ctx(lib_path, seqs, rects=None, mega=None):
    g = MpcGpu(0, lib_path)
    g.set_hmm(*G.hmm_tables())
    g.set_seqs(seqs)
    if rects is not None:
        g.set_pair_order(rects)
    if mega is not None:
        g.set_mega(mega["alpha"], mega["weight"], mega["lp"], mega["mx"], mega["profs"])
    return g


def run_on(g, iters=2):
    """the whole stage on an existing context, in one piece: (stages, ea) as _parity.run_lib returns them"""
    g.calc_posteriors()
    ea = g.get_ea().copy()
    g.build_store()
    stages = [g.get_sparse_range()]
    if g.n >= 3:
        for _ in range(iters):
            g.cons_iter()
            g.cons_commit()
            stages.append(g.get_sparse_range())
    return stages, ea


def positions(g):
    n = g.n
    return {(x, y): g.pair_position(x, y) for x in range(n) for y in range(x + 1, n)}


def check_positions(g, rects):
    """pair_position == the inverse of position_pairs, for every pair"""
    n = g.n
    px, py = position_pairs(n, np.zeros((0, 4)) if rects is None else rects)
    assert len(px) == n * (n - 1) // 2 and len(set(zip(px.tolist(), py.tolist()))) == len(px), "not an order of all pairs"
    got = positions(g)
    for q, (x, y) in enumerate(zip(px.tolist(), py.tolist())):
        assert got[(x, y)] == q, ("pair", x, y, got[(x, y)], q)


def check_positions_many(lib_path, seed=1):
    """positions only (host tables, no stage): the fixed orders at 3..16 sequences (plan_partition cuts blocks at 8 ranks from 16 on),
    40 generated ones, then back to InitPairs order"""
    rng = np.random.default_rng(seed)
    g = MpcGpu(0, lib_path)
    g.set_hmm(*G.hmm_tables())
    for n in (3, 4, 7, 12, 16):
        seqs = make_family(n, 12, seed=n)
        g.set_seqs(seqs)
        for name, rects in fixed_orders([len(s) for s in seqs], lib_path).items():
            g.set_pair_order(rects)
            check_positions(g, rects)
        for _ in range(8):
            rects = random_order(n, rng)
            g.set_pair_order(rects)
            check_positions(g, rects)
        g.set_pair_order(None)
        check_positions(g, None)
    g.close()


# ---- the stage under one order ------------------------------------------------------------------------------------------
def cut_points(N, parts, rng):
    return [0] + sorted(int(x) for x in rng.choice(np.arange(1, N), min(parts - 1, N - 1), replace=False)) + [N]


def run_sharded(lib_path, seqs, rects, rng, mem, iters=2, mega=None):
    """stage A as 2-3 position ranges (cut anywhere, inside rectangles too), each on a context of its own; the shards exported into
    one buffer in shuffled order at explicit offsets (gaps between them); store_import_part(own = all) on the first context; every
    relax in two position halves, then cons_commit -> (stages, ea)"""
    n = len(seqs)
    N = n * (n - 1) // 2
    cuts = cut_points(N, int(rng.integers(2, 4)), rng)
    ctxs = [new_ctx(lib_path, seqs, rects, mega) for _ in cuts[:-1]]
    sizes = []
    for g, a, b in zip(ctxs, cuts[:-1], cuts[1:]):
        g.calc_posteriors(a, b)
        sizes.append(g.shard_info()[0])
    perm = [int(s) for s in rng.permutation(len(sizes))]
    offs, at = [0] * len(sizes), 0
    for s in perm:
        at += 4 * int(rng.integers(0, 9))
        offs[s] = at
        at += sizes[s]
    buf = mem.alloc(at)
    for s in perm:
        ctxs[s].shard_export(buf + offs[s])
    for g in ctxs[1:]:
        g.close()
    g = ctxs[0]
    g.store_import_part([cuts[s] for s in perm], [cuts[s + 1] for s in perm], [sizes[s] for s in perm], [offs[s] for s in perm], buf, 0, N)
    ea = g.get_ea().copy()
    stages = [g.get_sparse_range()]
    if n >= 3:
        for _ in range(iters):
            h = int(rng.integers(0, N + 1))
            g.cons_iter(0, h)
            g.cons_iter(h, N)
            g.cons_commit()
            stages.append(g.get_sparse_range())
    g.close()
    return stages, ea


def check_sharded_orders(lib_path, seqs, orders, seed=0, envs=(None,), want=None):
    """every order (name -> rects): positions, then the sharded stage under every relax environment == the oracle"""
    rng = np.random.default_rng(seed)
    want = want or P.run_oracle(seqs)
    mem = DevMem(lib_path)
    for name, rects in orders.items():
        g = new_ctx(lib_path, seqs, rects)
        check_positions(g, rects)
        g.close()
        for env in envs:
            with Env(env):
                P.assert_same(run_sharded(lib_path, seqs, rects, rng, mem), want, "order %s, %s" % (name, env))
    mem.free()


def check_partial_exchange(lib_path, seqs, rects, seed=0, want=None, joins=3):
    """two contexts own the positions [0,m) and [m,N) of a custom order: stage A in those two pieces, the shards gathered into a
    buffer of each, PARTIAL stores (store_import_part). Every iteration: each relaxes and commits its own slice, the slices cross by
    values_export -> values_import, and each commits the foreign one (cons_commit_range). Between the import and that commit a foreign
    pair still reads as its last committed matrix. After two iterations both equal the oracle, and again after store_complete;
    then BuildPost / AlignAlns on each (MPCGPU_BP rows and sort) equal the restatement over the oracle's final store."""
    rng = np.random.default_rng(seed)
    want = want or P.run_oracle(seqs)
    n = len(seqs)
    N = n * (n - 1) // 2
    m = int(rng.integers(1, N))
    own = [(0, m), (m, N)]
    mem = DevMem(lib_path)
    ranks = [new_ctx(lib_path, seqs, rects) for _ in own]
    for g, (a, b) in zip(ranks, own):
        g.calc_posteriors(a, b)
    sizes = [g.shard_info()[0] for g in ranks]
    bufs = [mem.alloc(sizes[0] + sizes[1]) for _ in ranks]  # one per rank: its store adopts it and commits write into it
    for buf in bufs:
        ranks[0].shard_export(buf)
        ranks[1].shard_export(buf + sizes[0])
    for g, buf, (a, b) in zip(ranks, bufs, own):
        g.store_import_part([m, 0], [N, m], [sizes[1], sizes[0]], [sizes[0], 0], buf, a, b)
    pos = positions(ranks[0])
    pairs = [(x, y) for x in range(n) for y in range(x + 1, n)]
    for g in ranks:
        assert np.array_equal(P.bits(g.get_ea()), P.bits(want[1]))
    sl = [g.values_slice(a, b) for g, (a, b) in zip(ranks, own)]
    vb = [mem.alloc(4 * cnt) for _, cnt in sl]
    for it in range(2):
        for g, (a, b) in zip(ranks, own):
            g.cons_iter(a, b)
        for g, s in zip(ranks, sl):
            g.cons_commit_range(*s)
        for g, s, v in zip(ranks, sl, vb):
            g.values_export(s[0], s[1], v)
        for r, g in enumerate(ranks):
            g.values_import(sl[1 - r][0], sl[1 - r][1], vb[1 - r])
        for r, g in enumerate(ranks):  # imported, not committed: the foreign pairs are still the last committed ones
            got = g.get_sparse_range()
            for k, p in enumerate(pairs):
                mine = own[r][0] <= pos[p] < own[r][1]
                wo, wv = want[0][it + 1 if mine else it][k]
                assert np.array_equal(got[k][0], wo) and np.array_equal(got[k][1], wv), ("rank", r, "iteration", it, "pair", p, mine)
        for r, g in enumerate(ranks):
            g.cons_commit_range(*sl[1 - r])
        for r, g in enumerate(ranks):
            P.assert_same(([g.get_sparse_range()], want[1]), ([want[0][it + 1]], want[1]), "rank %d iteration %d" % (r, it))
    for r, g in enumerate(ranks):
        g.store_complete()
        P.assert_same(([g.get_sparse_range()], g.get_ea()), ([want[0][-1]], want[1]), "rank %d after store_complete" % r)
    final = want[0][-1]
    pidx = {p: k for k, p in enumerate(pairs)}
    for _ in range(joins):
        idx = [int(x) for x in rng.permutation(n)]
        c = int(rng.integers(1, n))
        grp1, grp2 = idx[:c], idx[c:]
        rows1, C1 = BP.random_msa(seqs, grp1, rng)
        rows2, C2 = BP.random_msa(seqs, grp2, rng)
        m1, m2 = [BP.pos_to_col(x) for x in rows1], [BP.pos_to_col(x) for x in rows2]
        post = BP.build_post(final, pidx, grp1, grp2, m1, m2, C1, C2)
        sc0, path0 = O.calc_aln(post)
        for mode in ("rows", "sort"):
            with Env({"MPCGPU_BP": mode}):
                for r, g in enumerate(ranks):
                    got = g.build_post(grp1, grp2, m1, m2, C1, C2)
                    assert np.array_equal(P.bits(got.ravel()), P.bits(post.ravel())), ("build_post", mode, r, grp1, grp2)
                    path, sc = g.align_alns(grp1, grp2, m1, m2, C1, C2)
                    assert path == path0 and P.bits(sc) == P.bits(sc0), ("align_alns", mode, r, grp1, grp2)
    for g in ranks:
        g.close()
    mem.free()


def check_reorder(lib_path, seqs, rects_a, rects_b, want=None):
    """order A, then [] (InitPairs), then order B on ONE context: every run == the oracle; set_seqs with another n: InitPairs again"""
    want = want or P.run_oracle(seqs)
    g = new_ctx(lib_path, seqs)
    for name, rects in (("A", rects_a), ("InitPairs", None), ("B", rects_b)):
        g.set_pair_order(rects)
        check_positions(g, rects)
        P.assert_same(run_on(g), want, "order %s on a reused context" % name)
    g.set_seqs(seqs[:-2])
    check_positions(g, None)
    g.close()


def check_mega(lib_path, seqs, rects, seed=0):
    """structure-profile emissions under a custom order, whole and sharded"""
    mega = P.random_mega(seqs, seed=seed)
    want = P.run_oracle(seqs, mega=mega)
    g = new_ctx(lib_path, seqs, rects, mega)
    P.assert_same(run_on(g), want, "mega, custom order")
    g.close()
    mem = DevMem(lib_path)
    P.assert_same(run_sharded(lib_path, seqs, rects, np.random.default_rng(seed), mem, mega=mega), want, "mega, custom order, sharded")
    mem.free()


# ---- rejected calls (child process side; emulator only) -------------------------------------------------------------------
REJECT_SEQS = dict(n=7, length=40, seed=3)
ORDER_A = [[0, 3, 3, 7], [3, 7, 3, 7], [0, 3, 0, 3]]
REJECT_ORDERS = {
    "order_pair_twice": [[0, 3, 3, 7], [0, 7, 0, 7]],
    "order_pairs_missing": [[0, 3, 3, 7], [3, 7, 3, 7]],
    "order_past_n": [[0, 3, 3, 8], [3, 7, 3, 7], [0, 3, 0, 3]],
    "order_crosses_diagonal": [[0, 4, 3, 7], [4, 7, 4, 7], [0, 3, 0, 3]],
    "order_xa_after_xb": [[3, 0, 3, 7], [3, 7, 3, 7], [0, 3, 0, 3]],
    "order_null": None,
}
MAP_ENTRIES = ["align_alns_rows", "align_alns_general", "align_alns_batch", "build_post", "align_msas"]
REJECT_CASES = (list(REJECT_ORDERS) + ["map_%s_msa%d" % (e, s) for e in MAP_ENTRIES for s in (1, 2)]
                + ["overlap_tail", "overlap_reversed", "wrap_values_export", "wrap_values_import", "wrap_commit_first", "wrap_commit_count"])


def _bad_map(maps, kind, rng):
    """a row whose position -> column map is not strictly increasing: two positions on one column, or a decreasing step"""
    maps = [np.array(x, np.uint32) for x in maps]
    r = int(rng.integers(len(maps)))
    j = int(rng.integers(len(maps[r]) - 1))
    if kind == "dup":
        maps[r][j + 1] = maps[r][j]
    else:
        maps[r][j], maps[r][j + 1] = maps[r][j + 1], maps[r][j]
    return maps


def _map_case(g, seqs, entry, side, rng):
    """-> (entry point name, valid call, invalid call): the same join, the invalid one with one row's map broken on `side`"""
    kind = ("dup", "dec")[(MAP_ENTRIES.index(entry) + side) % 2]  # both kinds on both sides over the entry points
    grp1, grp2 = [5, 0, 3], [6, 1, 2, 4]
    rows1, C1 = BP.random_msa(seqs, grp1, rng)
    rows2, C2 = BP.random_msa(seqs, grp2, rng)
    m1, m2 = [BP.pos_to_col(x) for x in rows1], [BP.pos_to_col(x) for x in rows2]
    b1, b2 = (_bad_map(m1, kind, rng), m2) if side == 1 else (m1, _bad_map(m2, kind, rng))
    if entry in ("align_alns_rows", "align_alns_general"):
        env = {"MPCGPU_BP": "rows" if entry == "align_alns_rows" else "sort"}

        def call(a, b):
            with Env(env):
                return g.align_alns(grp1, grp2, a, b, C1, C2)
        return "mpcgpu_align_alns", lambda: call(m1, m2), lambda: call(b1, b2)
    if entry == "build_post":
        return "mpcgpu_build_post", lambda: g.build_post(grp1, grp2, m1, m2, C1, C2), lambda: g.build_post(grp1, grp2, b1, b2, C1, C2)
    if entry == "align_alns_batch":
        rows3, C3 = BP.random_msa(seqs, [2], rng)
        rows4, C4 = BP.random_msa(seqs, [4, 6], rng)
        other = ([2], [4, 6], [BP.pos_to_col(x) for x in rows3], [BP.pos_to_col(x) for x in rows4], C3, C4)
        return ("mpcgpu_align_alns_batch", lambda: g.align_alns_batch([other, (grp1, grp2, m1, m2, C1, C2)]),
                lambda: g.align_alns_batch([other, (grp1, grp2, b1, b2, C1, C2)]))
    # align_msas: pairs of rows of the two alignments, each with its row's map, on a context of its own (a registry of sequences, as
    # the drop-in keeps one: stage A on a pair list replaces the shard a store was built from)
    pr = [(0, 0), (1, 2), (2, 3), (0, 1)]
    reg = MpcGpu(0, g.L._name)
    reg.set_hmm(*G.hmm_tables())
    reg.set_seqs_registry(seqs)

    def msas(a, b):
        return reg.align_msas([grp1[i] for i, _ in pr], [grp2[j] for _, j in pr], [a[i] for i, _ in pr], [b[j] for _, j in pr], C1, C2)
    b1, b2 = (_bad_map([m1[i] for i, _ in pr], kind, rng), None) if side == 1 else (None, _bad_map([m2[j] for _, j in pr], kind, rng))
    bad1 = b1 if b1 is not None else [m1[i] for i, _ in pr]
    bad2 = b2 if b2 is not None else [m2[j] for _, j in pr]
    return ("mpcgpu_align_msas", lambda: msas(m1, m2),
            lambda: reg.align_msas([grp1[i] for i, _ in pr], [grp2[j] for _, j in pr], bad1, bad2, C1, C2))


def _same(a, b):
    """results of two valid calls (path / score / matrix / per-pair EA tuples) bit for bit"""
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    elif isinstance(a, str):
        assert a == b
    else:
        assert np.array_equal(P.bits(np.asarray(a)).ravel(), P.bits(np.asarray(b)).ravel())


def reject_case(case, lib_path):
    """one invalid call on a context that holds a finished run under ORDER_A: MpcGpuError naming the entry point, positions and
    matrices as before, and a full valid run (or, for the joins, the same valid call) afterwards still equals the oracle"""
    seqs = make_family(REJECT_SEQS["n"], REJECT_SEQS["length"], seed=REJECT_SEQS["seed"])
    n = len(seqs)
    N = n * (n - 1) // 2
    rng = np.random.default_rng(7)
    want = P.run_oracle(seqs)
    g = new_ctx(lib_path, seqs, np.array(ORDER_A, np.uint32))
    is_map = case.startswith("map_")
    if is_map:
        P.assert_same(run_on(g, iters=0), (want[0][:1], want[1]), "before")
    else:
        P.assert_same(run_on(g), want, "before")
    pos0, sp0, ea0 = positions(g), g.get_sparse_range(), g.get_ea().copy()
    mem = DevMem(lib_path)
    valid = None
    if case in REJECT_ORDERS:
        entry = "mpcgpu_set_pair_order"
        if case == "order_null":
            def bad():
                g._ck(g.L.mpcgpu_set_pair_order(g.h, 3, None))
        else:
            def bad():
                g.set_pair_order(np.array(REJECT_ORDERS[case], np.uint32))
    elif is_map:
        e, s = case[4:].rsplit("_msa", 1)
        entry, valid, bad = _map_case(g, seqs, e, int(s), rng)
        before = valid()
    elif case.startswith("overlap_"):
        entry = "mpcgpu_store_import_part"
        m = 9
        sh = [new_ctx(lib_path, seqs, np.array(ORDER_A, np.uint32)) for _ in range(2)]
        sh[0].calc_posteriors(0, m)
        sh[1].calc_posteriors(m, N)
        sizes = [x.shard_info()[0] for x in sh]
        buf = mem.alloc(sum(sizes) + 64)
        if case == "overlap_tail":  # the second shard starts one word before the end of the first
            k0s, k1s, by, offs = [0, m], [m, N], sizes, [0, sizes[0] - 4]
        else:  # listed second-first; the first lies at the start of the buffer, the second overlaps its last 8 bytes
            k0s, k1s, by, offs = [m, 0], [N, m], [sizes[1], sizes[0]], [sizes[0] - 8, 0]
        for k0, off in zip(k0s, offs):
            sh[0 if k0 == 0 else 1].shard_export(buf + off)

        def bad():
            g.store_import_part(k0s, k1s, by, offs, buf, 0, N)
    else:
        first, count = g.values_slice(0, N)
        big = 2 ** 64 - 4
        vbuf = mem.alloc(4 * (count + 16))
        entry, bad = {
            "wrap_values_export": ("mpcgpu_values_export", lambda: g.values_export(big, 8, vbuf)),
            "wrap_values_import": ("mpcgpu_values_import", lambda: g.values_import(8, big, vbuf)),
            "wrap_commit_first": ("mpcgpu_cons_commit_range", lambda: g.cons_commit_range(big, 8)),
            "wrap_commit_count": ("mpcgpu_cons_commit_range", lambda: g.cons_commit_range(8, big)),
        }[case]
    try:
        bad()
    except MpcGpuError as e:
        assert entry in str(e), (entry, str(e))
        print("refused: %s" % e, flush=True)
    else:
        raise AssertionError("%s: the invalid call was accepted" % case)
    assert positions(g) == pos0, "pair positions changed"
    P.assert_same(([g.get_sparse_range()], g.get_ea()), ([sp0], ea0), "state after the refused call")
    if is_map:
        _same(valid(), before)
        P.assert_same(run_on(g, iters=0), (want[0][:1], want[1]), "after")
    else:
        P.assert_same(run_on(g), want, "after")
    g.close()
    mem.free()
    print("OK %s" % case, flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "reject":
        reject_case(sys.argv[2], sys.argv[3])
    else:
        sys.exit("usage: _pair_order.py reject CASE LIB")
