"""UPGMA5 restated in numpy float32 (test infrastructure): UPGMA5::ScaleDistMx and FixEADistMx (upgma5.cpp:504-563), UPGMA5::Run
(upgma5.cpp:87-305) and Tree::ToFile for a rooted tree (treetofile.cpp:22-29, 68-95), plus the readers of cmd_upgma5's two input formats.

The reference's procedure is kept statement by statement where the order of statements decides a value: the clamp of negative distances, the
per-row minimum with the LOWEST partner among equal minima (ascending scan, strict '<' against FLT_MAX; UINT_MAX when nothing is below
FLT_MAX), the argmin of the cached minima over the live rows (lowest row among equals), the linkage formulas with every operation rounded to
float32 on its own, the neighbour redirect of upgma5.cpp:249-259, and — the point of UPGMA5 — m_MinDist / m_NearestNeighbor of the OTHER rows
left exactly as stale as the reference leaves them. The loop over j inside one join is written with array operations: every j of it reads
values no other j of the same join writes (row Lmin and row Rmin at column j), so the order inside the loop decides nothing but the new
row's minimum, which np.argmin over the values below FLT_MAX finds as the scan does (first = lowest j).

The matrix is a full symmetric n x n float32 array here (the reference's m_DistMx); the library works on the triangle in InitPairs order:
tri_of() / mx_of() convert."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
NONE = 0xFFFFFFFF
TRANSFORMS = ("none", "scale", "scale_dist", "ea")
LINKAGES = ("avg", "min", "max", "biased")


class UpgmaDies(Exception):
    """the reference asserts or dies on this input (upgma5.cpp:197-199, 512). kind: "ea_range" (FixEADistMx, before any join) or "no_min"
    (the join loop finds no minimum below FLT_MAX); join: the join at which the loop dies, None for "ea_range" """

    def __init__(self, msg, kind, join=None):
        Exception.__init__(self, msg)
        self.kind, self.join = kind, join


def tri_of(mx):
    """upper triangle, row-major: InitPairs order (by rows: no index arrays of the triangle's size)"""
    n = mx.shape[0]
    return np.ascontiguousarray(np.concatenate([mx[i, i + 1:] for i in range(n - 1)]), np.float32)


def mx_of(n, tri, diag=0.0):
    """the full symmetric matrix of a triangle, filled by rows: the one n x n array upgma() then works on in place"""
    mx = np.empty((n, n), np.float32)
    o = 0
    for i in range(n - 1):
        c = n - i - 1
        mx[i, i + 1:] = tri[o:o + c]
        o += c
    B = 256  # the lower triangle block by block (a column at a time would be a strided write per row)
    for b in range(0, n, B):
        e = min(n, b + B)
        blk = mx[b:e, b:e]
        blk[...] = np.where(np.triu(np.ones((e - b, e - b), bool), 1), blk, blk.T.copy())
        mx[e:, b:e] = mx[b:e, e:].T
    mx[np.arange(n), np.arange(n)] = diag
    return mx


def fold_min_max(mx):
    """MinDist / MaxDist of ScaleDistMx as the reference folds them (upgma5.cpp:524-535): both start at entry (0, 1) and meet the entries
    (i, j), j < i, row by row; std::min(Min, d) is d < Min ? d : Min and std::max(Max, d) is Max < d ? d : Max. A NaN is therefore skipped
    unless it is entry (0, 1) (then both stay NaN), and of a zero of both signs the one met FIRST is kept."""
    n = mx.shape[0]
    mn = ma = F(mx[0, 1])
    for i in range(1, n):
        row = mx[i, :i]
        lo = row[row < mn]  # nothing compares below / above a NaN
        if lo.size:
            mn = lo[np.argmin(lo)]  # first among equals, as the scan
        hi = row[ma < row]
        if hi.size:
            ma = hi[np.argmax(hi)]
    return F(mn), F(ma)


def device_min_max(tri):
    """what mpcgpu_upgma_scale returns (kernels_upgma.h: mpc_min_z / mpc_max_z): the reference's fold, except that of a zero of both
    signs -0 is the Min and +0 is the Max wherever they stand — the one answer a parallel fold can give. (Entry 0 of the triangle is
    entry (0, 1); which entry is met first decides nothing else.)"""
    t = np.asarray(tri, np.float32)
    mn = ma = F(t[0])
    if not np.isnan(mn):
        v = t[~np.isnan(t)]
        mn, ma = F(v.min()), F(v.max())
        bits = t.view(np.uint32)
        if mn == 0:
            mn = F(-0.0) if (bits == 0x80000000).any() else F(0.0)
        if ma == 0:
            ma = F(0.0) if (bits == 0).any() else F(-0.0)
    return mn, ma


def scale_dist_mx(mx, input_is_similarity=True, extremes=None, inplace=False):
    """upgma5.cpp:521-563 -> (new matrix, Min, Max); extremes: Min and Max found elsewhere (device_min_max). The diagonal stays."""
    mn, ma = fold_min_max(mx) if extremes is None else extremes
    SCALE = F(10.0)
    diag = mx.diagonal().copy()
    out = mx if inplace else mx.copy()
    with np.errstate(all="ignore"):
        if input_is_similarity:
            np.subtract(ma, out, out=out)
        else:
            np.subtract(out, mn, out=out)
        np.multiply(SCALE, out, out=out)
        np.divide(out, ma - mn, out=out)
    assert out.dtype == np.float32 and (ma - mn).dtype == np.float32
    out[np.arange(len(diag)), np.arange(len(diag))] = diag
    return out, mn, ma


def fix_ea_dist_mx(mx, inplace=False):
    """upgma5.cpp:504-519"""
    n = mx.shape[0]
    for i in range(1, n):
        d = mx[i, :i]
        if not np.all((d >= 0) & (d <= 1)):
            raise UpgmaDies("asserta(d >= 0 && d <= 1), upgma5.cpp:512", "ea_range")
    out = mx if inplace else mx.copy()
    np.subtract(F(1), out, out=out)
    np.fill_diagonal(out, 0)
    return out


def transform_mx(mx, transform, extremes=None, inplace=False):
    if transform == "scale":
        return scale_dist_mx(mx, True, extremes, inplace)[0]
    if transform == "scale_dist":
        return scale_dist_mx(mx, False, extremes, inplace)[0]
    if transform == "ea":
        return fix_ea_dist_mx(mx, inplace)
    assert transform == "none"
    return mx if inplace else mx.copy()


def _first_min_below_flt_max(vals, idx):
    """ascending scan with 'd < best', best starting at FLT_MAX, over vals (at the ascending indices idx) -> (best, index or NONE)"""
    ok = vals < FLT_MAX  # NaN: false, as in the scan
    if not ok.any():
        return F(FLT_MAX), NONE
    v = vals[ok]
    k = int(np.argmin(v))  # first occurrence of the minimum
    return F(v[k]), int(idx[ok][k])


STAT_KEYS = ("joins", "L_ge_T", "R_ge_T", "L_gt_R", "argmin_tied", "argmin_tied_waves", "argmin_tied_strides", "newmin_tied",
             "newmin_tied_waves", "newmin_tied_strides", "redirect_joins", "redirects", "stale_picks")


def new_stats(T):
    """the counters run() fills: per tree, the joins that took each path of upgma_join_kernel with a workgroup of T lanes (lane j mod T owns
    row j; wave (j mod T) // 64; stride j // T). dies_at: the join at which the reference asserts, or None"""
    st = dict.fromkeys(STAT_KEYS, 0)
    st["T"], st["dies_at"] = T, None
    return st


def _count_ties(st, name, vals, idx, best):
    """the rows that hold the minimum `best` (< FLT_MAX) among vals at idx: more than one = a tie the index decides; in different waves /
    strides = a tie the fold across waves / a lane's own scan over its strides decides"""
    T = st["T"]
    tied = idx[vals == best]
    if tied.size > 1:
        st[name + "_tied"] += 1
        st[name + "_tied_waves"] += int(np.unique((tied % T) // 64).size > 1)
        st[name + "_tied_strides"] += int(np.unique(tied // T).size > 1)


def run(mx, linkage="avg", stats=None, copy=True):
    """UPGMA5::Run on the (already transformed) matrix -> (left, right, left_len, right_len, height), n - 1 entries each. stats: a dict of
    new_stats(T), filled as a side effect (also when the run dies); what is returned does not depend on it. copy = False: mx is float32
    and may be overwritten."""
    n = mx.shape[0]
    assert n >= 2 and linkage in LINKAGES
    D = mx.astype(np.float32) if copy else mx  # astype copies
    assert D.dtype == np.float32
    D[D < 0] = 0  # upgma5.cpp:140-145 (-0.0 and NaN are not below 0)
    D[np.arange(n), np.arange(n)] = FLT_MAX  # never read by the reference (j != i everywhere): not below FLT_MAX, so no scan takes it
    allj = np.arange(n)
    min_dist = np.full(n, FLT_MAX, np.float32)
    nearest = np.full(n, NONE, np.int64)
    node = np.arange(n, dtype=np.int64)
    for i in range(n):  # upgma5.cpp:133-157: row i meets its partners in ascending order
        min_dist[i], nearest[i] = _first_min_below_flt_max(D[i], allj)
    left = np.full(n - 1, NONE, np.uint32)
    right = np.full(n - 1, NONE, np.uint32)
    llen = np.full(n - 1, FLT_MAX, np.float32)
    rlen = np.full(n - 1, FLT_MAX, np.float32)
    height = np.full(n - 1, FLT_MAX, np.float32)
    c01, c09 = F(0.1), F(1) - F(0.1)
    for k in range(n - 1):
        live = allj[node != NONE]
        md = min_dist[live]
        best, L = _first_min_below_flt_max(md, live)  # upgma5.cpp:178-195
        if L == NONE:
            if stats is not None:
                stats["dies_at"] = k
            raise UpgmaDies("assert(Lmin != UINT_MAX) at join %d, upgma5.cpp:197" % k, "no_min", k)
        R = int(nearest[L])
        if R == NONE or node[R] == NONE or R == L:
            if stats is not None:
                stats["dies_at"] = k
            raise UpgmaDies("assert(UINT_MAX != Rmin) at join %d, upgma5.cpp:192-193" % k, "no_min", k)
        js = live[(live != L) & (live != R)]  # upgma5.cpp:214-219
        dL, dR = D[L, js], D[R, js]
        with np.errstate(all="ignore"):
            avg = (dL + dR) / F(2)
            mi = np.where(dR < dL, dR, dL)  # std::min(dL, dR)
            ma = np.where(dL < dR, dR, dL)  # std::max(dL, dR)
            if linkage == "avg":
                nd = avg
            elif linkage == "min":
                nd = mi
            elif linkage == "max":
                nd = ma
            else:
                nd = c01 * avg + c09 * mi
        nd = nd.astype(np.float32)
        redirected = js[nearest[js] == R]
        nearest[redirected] = L  # upgma5.cpp:249-259
        new_min, new_nn = _first_min_below_flt_max(nd, js)
        if stats is not None:
            T = stats["T"]
            stats["joins"] += 1
            stats["L_ge_T"] += int(L >= T)
            stats["R_ge_T"] += int(R >= T)
            stats["L_gt_R"] += int(L > R)
            _count_ties(stats, "argmin", md, live, best)
            if new_nn != NONE:
                _count_ties(stats, "newmin", nd, js, new_min)
            stats["redirect_joins"] += int(redirected.size > 0)
            stats["redirects"] += int(redirected.size)
            stats["stale_picks"] += int(not (min_dist[L] == D[L, R]))
        D[L, js] = nd
        D[js, L] = nd
        h = F(D[L, R]) / F(2)  # upgma5.cpp:276-290
        uL, uR = int(node[L]), int(node[R])
        hL = F(0) if uL < n else height[uL - n]
        hR = F(0) if uR < n else height[uR - n]
        left[k], right[k] = uL, uR
        with np.errstate(all="ignore"):
            llen[k], rlen[k], height[k] = h - hL, h - hR, h
        node[L] = n + k
        nearest[L] = new_nn
        min_dist[L] = new_min
        node[R] = NONE
    return left, right, llen, rlen, height


def upgma(n, tri, transform="none", linkage="avg"):
    """what mpcgpu_upgma computes: the triangle in InitPairs order -> (left, right, left_len, right_len)"""
    return upgma_full(n, tri, transform, linkage)[:4]


def upgma_full(n, tri, transform="none", linkage="avg", stats=None):
    """-> run()'s five arrays, on ONE n x n float32 array (built by rows, transformed and clustered in place). Min and Max of a scaling
    transform are the device's (device_min_max): they are the reference's fold except for the sign of an extreme that is a zero of both
    signs, which the reference leaves to its scan order and the device decides by rule"""
    diag = FLT_MAX if transform == "none" else 0.0
    tri = np.asarray(tri, np.float32)
    ext = device_min_max(tri) if transform in ("scale", "scale_dist") else None
    return run(transform_mx(mx_of(n, tri, diag), transform, ext, inplace=True), linkage, stats, copy=False)


# ---- the launcher of mpcgpu_upgma.inc restated (upgma_run, mpcgpu_sw_tree) ------------------------------------------------------
JOIN_THREADS = {"gpu": 1024, "emu": 128}  # MPC_UPGMA_THREADS
CUS = {"gpu": 256, "emu": 2}              # MI355X; tests/emu/hip_emu.h (hipGetDeviceProperties: what the launcher reads)
FOLD_THREADS = 256                        # workgroup of the four helper kernels
LDS_ROWS_MAX = 12288                      # MPC_UPGMA_LDS_ROWS_MAX
SCRATCH_BYTES = 256                       # MPC_UPGMA_SCRATCH_BYTES


def n_tri(n):
    return n * (n - 1) // 2


def grid(m, cus):
    """workgroups of upgma_minmax_kernel / upgma_transform_kernel over m distances"""
    return max(1, min((m + 255) // 256, cus * 8))


def n_partials(m, cus):
    """(Min, Max) pairs upgma_transform_kernel folds: one per workgroup of upgma_minmax_kernel"""
    return grid(m, cus)


def passes(m, cus):
    """iterations of the grid-stride loop over the triangle in the workgroup that makes the most"""
    per = grid(m, cus) * FOLD_THREADS
    return (m + per - 1) // per


def fold_rounds(m, cus):
    """iterations of `q += blockDim.x` over the partials"""
    return (n_partials(m, cus) + FOLD_THREADS - 1) // FOLD_THREADS


def init_grid(n, cus):
    return min((n + 3) // 4, cus * 8)


def init_row_passes(n, cus):
    """rows a wavefront of upgma_init_kernel takes (4 wavefronts per workgroup)"""
    nwv = init_grid(n, cus) * (FOLD_THREADS // 64)
    return (n + nwv - 1) // nwv


def sw_norm_grid(n, cus):
    return min(n - 1, cus * 8)


def lds_cut(env_rows=None):
    """MPCGPU_UPGMA_LDS_ROWS clipped to 0 .. MPC_UPGMA_LDS_ROWS_MAX; unset: the maximum"""
    return min(LDS_ROWS_MAX, max(0, LDS_ROWS_MAX if env_rows is None else int(env_rows)))


def join_lds(n, env_rows=None):
    """-> (row state in LDS, dynamic LDS bytes of upgma_join_kernel)"""
    lds = n <= lds_cut(env_rows)
    return lds, SCRATCH_BYTES + (12 * n if lds else 0)


def extremes_positions(n, cus):
    """triangle positions (Min, Max) for make_tri's "extremes_at": [0] Min in the last entry, Max in the first entry of the second pass of
    the grid-stride loop; [1] both in workgroups b >= 256 — partials only the later rounds of the fold over the partials reach — in
    their first pass: the last lane of workgroup 256 and the first lane of the last workgroup. (A grid of at most 256 workgroups, the
    emulator's, has no such partial: workgroup grid // 2 stands in, and the fold over the partials has one round.)"""
    m, g = n_tri(n), grid(n_tri(n), cus)
    assert passes(m, cus) >= 2 and g >= 4, (n, cus, "the triangle is too small for these placements")
    b = FOLD_THREADS if g > FOLD_THREADS else g // 2
    return [(m - 1, g * FOLD_THREADS), (b * FOLD_THREADS + FOLD_THREADS - 1, (g - 1) * FOLD_THREADS)]


def newick(labels, left, right, llen, rlen):
    """Tree::Create (tree.cpp:1454-1500) + Tree::ToFile of the rooted tree (treetofile.cpp:22-29, 68-95); the root is node 2n - 2"""
    n = len(labels)
    root = 2 * n - 2
    out = []

    def node(u, length):
        group = u >= n
        if group:
            out.append("(\n")
        if u < n:
            out.append(labels[u])
        else:
            node(int(left[u - n]), llen[u - n])
            out.append(",\n")
            node(int(right[u - n]), rlen[u - n])
        if group:
            out.append(")")
        if u != root:
            out.append(":%g" % float(length))  # the edge length is kept as a double (tree.h)
        out.append("\n")

    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * n + 100))
    try:
        node(root, None)
    finally:
        sys.setrecursionlimit(old)
    out.append(";\n")
    return "".join(out)


# ---- cmd_upgma5's readers (upgma5.cpp:386-502) ---------------------------------------------------------------------------
def read_dist_mx(text):
    """label1 TAB label2 TAB dist; labels in order of first appearance; a pair the file does not name is FLT_MAX"""
    labels, index = [], {}
    rows = [ln.split("\t") for ln in text.splitlines() if ln]
    for a, b, _ in rows:
        for lab in (a, b):
            if lab not in index:
                index[lab] = len(labels)
                labels.append(lab)
    n = len(labels)
    mx = np.full((n, n), FLT_MAX, np.float32)
    for a, b, d in rows:
        mx[index[a], index[b]] = mx[index[b], index[a]] = F(float(d))
    return labels, mx


def read_dist_mx2(text):
    """reseek format: distmx TAB N, N lines index TAB label, then index1 TAB index2 TAB score; a pair the file does not name is 0"""
    lines = [ln for ln in text.splitlines() if ln]
    hdr = lines[0].split("\t")
    assert hdr[0] == "distmx"
    n = int(hdr[1])
    labels = [lines[1 + i].split("\t")[1] for i in range(n)]
    mx = np.zeros((n, n), np.float32)
    for ln in lines[1 + n:]:
        a, b, d = ln.split("\t")
        if int(a) != int(b):
            mx[int(a), int(b)] = mx[int(b), int(a)] = F(float(d))
    return labels, mx


def cmd_upgma5(text, mode, linkage):
    """cmd_upgma5 (upgma5.cpp:565-610): mode "plain", "scaledist", "eadist" or "reseek" -> the Newick text it writes"""
    if mode == "reseek":
        labels, mx = read_dist_mx2(text)
        mx = scale_dist_mx(mx)[0]
    else:
        labels, mx = read_dist_mx(text)
        if mode == "scaledist":
            mx = scale_dist_mx(mx)[0]
        elif mode == "eadist":
            mx = fix_ea_dist_mx(mx)
    left, right, llen, rlen, _ = run(mx, linkage)
    return newick(labels, left, right, llen, rlen)


# ---- test matrices --------------------------------------------------------------------------------------------------------
SUB_MIN = np.uint32(1).view(np.float32)  # the smallest subnormal: its half rounds to 0
EA_BAD = {"above_1": np.nextafter(F(1), F(2)), "neg_subnormal": -SUB_MIN, "nan": F(np.nan)}


def make_tri(n, kind, seed):
    """seeded triangle of n leaves. kind, a name or a tuple (name, parameters):
    "random" in (0, 1); "quant": 4 distinct values (ties, the redirect, stale minima); "negative": some entries below 0; "fltmax": two
    entries FLT_MAX;
    "subnormal": every entry below FLT_MIN — half of them 1 .. 15 units of the smallest subnormal (ties; 1 unit halves to 0), half anywhere
    below 2^23 units; "zeros_both": positive entries, +0 early (entries 0, m // 3) and -0 late (m // 2, m - 2): the Min is a zero of both
    signs; "zeros_both_max": its mirror, negative entries, -0 early and +0 late: the Max is;
    "nan_mid": three NaNs, none at entry 0; "nan_first": a NaN at entry 0; "nan_all": nothing else (under "ea" the value check AND the
    join loop have something to refuse: the reference dies in the check); "inf": two +inf entries;
    "ea_edge_ok": only +0, -0, 1, the float below 1, the smallest subnormal, 0.25 and 0.5;
    ("ea_one_bad", name): random in (0, 1) but the LAST entry EA_BAD[name];
    ("extremes_at", at_min, at_max): random in [0.25, 0.75) with a unique Min 0.125 and a unique Max 0.875 at these positions"""
    rng = np.random.default_rng(seed)
    m = n * (n - 1) // 2
    name = kind if isinstance(kind, str) else kind[0]
    if name == "subnormal":
        assert m >= 4
        u = np.where(rng.random(m) < 0.5, rng.integers(1, 16, m), rng.integers(1, 1 << 23, m)).astype(np.uint32)
        u[0], u[m // 2], u[m - 1] = 1, 1, (1 << 23) - 1
        return u.view(np.float32).copy()
    if name == "ea_edge_ok":
        vals = np.array([0.0, -0.0, 1.0, np.nextafter(F(1), F(0)), SUB_MIN, 0.25, 0.5], np.float32)
        return vals[rng.integers(0, len(vals), m)]
    t = rng.random(m).astype(np.float32)
    if name == "quant":
        t = (np.floor(t * 4) / 4 + 0.125).astype(np.float32)
        if m >= 2:
            t[0], t[-1] = F(0.125), F(0.875)  # two distinct values also at the smallest sizes
    elif name == "negative":
        t = (t - F(0.3)).astype(np.float32)
    elif name == "fltmax":
        # two entries: an average of two FLT_MAX is infinite and is never a minimum again, so a matrix with many of them ends in the
        # reference's assert under every linkage but "min" (as this one does under "max": the last join is the largest entry)
        t[rng.choice(m, size=min(2, m), replace=False)] = FLT_MAX
        if m >= 2:
            t[0], t[-1] = F(0.25), F(0.75)
    elif name in ("zeros_both", "zeros_both_max"):
        assert m >= 12
        t = (F(0.1) + F(0.9) * t).astype(np.float32)
        early, late = F(0.0), F(-0.0)
        if name == "zeros_both_max":
            t, early, late = -t, F(-0.0), F(0.0)
        t[0] = t[m // 3] = early  # entry 0 is where every lane of the device's fold starts: only the sign rule makes the late zero win
        t[m // 2] = t[m - 2] = late
    elif name == "nan_mid":
        assert m >= 8
        t[[m // 3, m // 2, m - 1]] = np.nan
    elif name == "nan_first":
        t[0] = np.nan
    elif name == "nan_all":
        t[:] = np.nan
    elif name == "inf":
        assert m >= 4
        t[[m // 3, m - 2]] = np.inf
    elif name == "ea_one_bad":
        t[-1] = EA_BAD[kind[1]]
    elif name == "extremes_at":
        at_min, at_max = kind[1], kind[2]
        assert 0 <= at_min < m and 0 <= at_max < m and at_min != at_max
        t = (F(0.25) + F(0.5) * t).astype(np.float32)
        t[at_min], t[at_max] = F(0.125), F(0.875)
    else:
        assert name == "random", kind
    return t


# ---- named cases: tests/test_upgma_table.py shows from run()'s counters and the restated launcher which path each one reaches; the
# device and the emulator tests run them ----
STRIDE_N = {"gpu": 2100, "emu": 300}   # rows beyond the first stride of the join workgroup: more than 2 T and no multiple of T
SMALL_N = {"gpu": 65, "emu": 129}      # one past a wavefront / one past the emulator's workgroup
EA_BAD_N = {"gpu": 1025, "emu": 140}
STRIDE_KINDS = ("quant", "random")
# the refusals these inputs are there for, from the reference's text: a NaN or an infinite Min / Max makes every scaled distance NaN
# (inf - d over inf - Min; anything with NaN), no NaN is below FLT_MAX, so join 0 finds no minimum; FixEADistMx dies on its first value
# outside 0 .. 1 (NaN fails both comparisons) before any join, whatever the join loop would have met
REFUSED = {("nan_first", "scale"): ("no_min", 0), ("nan_first", "scale_dist"): ("no_min", 0), ("inf", "scale"): ("no_min", 0),
           ("nan_all", "none"): ("no_min", 0), ("nan_all", "ea"): ("ea_range", None), ("ea_one_bad", "ea"): ("ea_range", None)}


def edge_cases(where):
    """(n, kind, transform, linkage) of the value-edge cases for "gpu" or "emu" """
    n, out = SMALL_N[where], []
    for kind in ("zeros_both", "zeros_both_max"):
        out += [(n, kind, tr, lk) for tr in ("scale_dist", "scale") for lk in LINKAGES]
    for m in (n, 300):
        out += [(m, "subnormal", "none", lk) for lk in LINKAGES] + [(m, "subnormal", "scale", "avg")]
    for kind in ("nan_mid", "inf"):
        out += [(n, kind, tr, lk) for tr in ("none", "scale") for lk in LINKAGES]
    out += [(n, "nan_first", "scale", "avg"), (n, "nan_first", "scale_dist", "max"), (n, "nan_all", "none", "avg"), (n, "nan_all", "ea", "avg")]
    out += [(n, "ea_edge_ok", "ea", lk) for lk in LINKAGES]
    out += [(EA_BAD_N[where], ("ea_one_bad", b), "ea", "avg") for b in EA_BAD]
    return out


def outcome(exp):
    """a want() in REFUSED's terms"""
    return (exp.kind, exp.join) if isinstance(exp, UpgmaDies) else "tree"


# ---- the library against the restatement ------------------------------------------------------------------------------------
_CTX = {}


def ctx(lib_path=None):
    """one context per library for all tests of a process"""
    from muscle_amd import _lib
    if lib_path not in _CTX:
        _CTX[lib_path] = _lib.MpcGpu(0, lib_path=lib_path)
    return _CTX[lib_path]


_WANT = {}


def want(n, kind, transform, linkage):
    """the restatement's answer (or the UpgmaDies it raised), computed once per case"""
    key = (n, kind, transform, linkage)
    if key not in _WANT:
        try:
            _WANT[key] = upgma(n, make_tri(n, kind, 1000 + n), transform, linkage)
        except UpgmaDies as e:
            _WANT[key] = e
    return _WANT[key]


# matrices whose trees may hold NaN branch lengths. IEEE 754 leaves sign and payload of a NaN result open, and the units differ: the x86
# unit the reference runs on hands on the NaN operand's sign from h - NaN (7fc00000 stays 7fc00000) and makes ffc00000 from inf - inf;
# gfx950 returns ffc00000 for the former (seen at 65 leaves, "nan_mid": 1 to 3 lengths per tree). A NaN length is compared as "a NaN in
# the same place"; every other length of these trees, and every length of every other matrix, bit for bit.
NAN_KINDS = ("nan_mid", "nan_first", "nan_all", "inf")


def assert_same_tree(got, exp, what, nan_any=False):
    for name, g, w in zip(("left", "right", "left_len", "right_len"), got, exp):
        if name in ("left", "right"):
            assert np.array_equal(np.asarray(g, np.uint32), np.asarray(w, np.uint32)), "%s: %s differs" % (what, name)
        else:
            gb, wb = np.asarray(g, np.float32).view(np.uint32).copy(), np.asarray(w, np.float32).view(np.uint32).copy()
            if nan_any:
                both = np.isnan(np.asarray(g, np.float32)) & np.isnan(np.asarray(w, np.float32))
                if (gb[both] != wb[both]).any():
                    at = np.nonzero(both & (gb != wb))[0]
                    print("%s: %d NaNs of %s with other bits than the restatement's, e.g. [%d] %08x, there %08x" % (what, len(at), name, at[0], gb[at[0]], wb[at[0]]))
                gb[both] = wb[both] = 0x7FC00000
            at = np.nonzero(gb != wb)[0][:8]
            assert at.size == 0, "%s: the bits of %s differ at %s: %s, expected %s" % (what, name, at, ["%08x" % x for x in gb[at]], ["%08x" % x for x in wb[at]])


def refusal_of(msg):
    """(kind, join) of a refusal of mpcgpu_upgma / mpcgpu_sw_tree after the run, in UpgmaDies' terms"""
    import re
    if "an EA value outside 0 .. 1" in msg:
        return "ea_range", None
    r = re.search(r"no distance below FLT_MAX is left at join (\d+) of (\d+)", msg)
    assert r, "neither kind of refusal: %s" % msg
    return "no_min", int(r.group(1))


def float_bits(x):
    return int(np.asarray(x, np.float32).reshape(1).view(np.uint32)[0])


def check_call(g, n, tri, transform, linkage, exp, what, lds=None, nan_any=False):
    """one mpcgpu_upgma call on context g against exp, the restatement's tree or the UpgmaDies it raised: node indices equal, float bits of
    the lengths equal, after a scaling transform mpcgpu_upgma_scale's bits equal device_min_max's; where the reference dies, a refusal by
    name, of the same kind (EA range / no minimum) and naming the same join. lds: what mpcgpu_upgma_info must say of the row state;
    nan_any: NAN_KINDS"""
    from muscle_amd import _lib
    if isinstance(exp, UpgmaDies):
        try:
            g.upgma(n, tri, transform, linkage)
        except _lib.MpcGpuError as e:
            assert "mpcgpu_upgma:" in str(e), str(e)
            assert refusal_of(str(e)) == (exp.kind, exp.join), "%s: the reference dies with %s, the library says %s" % (what, exp, e)
            if exp.kind == "no_min":
                assert str(e).count("of %d " % (n - 1)) == 1, str(e)
            return None
        raise AssertionError("%s: the reference dies here (%s), the library returned a tree" % (what, exp))
    got = g.upgma(n, tri, transform, linkage)
    info = g.upgma_info()
    assert info[0] == n, (what, info)
    if lds is not None:
        assert info[1] == (1 if lds else 0), (what, info)
    assert_same_tree(got, exp, what, nan_any=nan_any)
    if transform in ("scale", "scale_dist"):
        mn, ma = g.upgma_scale()
        emn, ema = device_min_max(tri)
        assert (float_bits(mn), float_bits(ma)) == (float_bits(emn), float_bits(ema)), "%s: Min, Max %r %r, expected %r %r" % (what, mn, ma, emn, ema)
    else:
        try:
            g.upgma_scale()
        except _lib.MpcGpuError as e:
            assert "mpcgpu_upgma_scale" in str(e), str(e)
        else:
            raise AssertionError("%s: mpcgpu_upgma_scale answered after a run without a scaling transform" % what)
    return got


def check_case(lib_path, n, kind, transform, linkage, lds):
    """mpcgpu_upgma on the process's context against the restatement (check_call); mpcgpu_upgma_info must name the path (lds: the row
    state in LDS or in global memory)"""
    exp = want(n, kind, transform, linkage)
    tri = make_tri(n, kind, 1000 + n)
    name = kind if isinstance(kind, str) else kind[0]
    return check_call(ctx(lib_path), n, tri, transform, linkage, exp, "n=%d %s %s %s" % (n, kind, transform, linkage), lds, name in NAN_KINDS)


def prefilled_outputs(n):
    """four output arrays of n - 1 entries holding a pattern no tree has"""
    return [np.full(n - 1, 0xA5A5A5A5, np.uint32), np.full(n - 1, 0x5A5A5A5A, np.uint32),
            np.full(n - 1, 0xC3C3C3C3, np.uint32).view(np.float32), np.full(n - 1, 0x3C3C3C3C, np.uint32).view(np.float32)]


def check_refusal_leaves_outputs(lib_path, n, kind, transform, linkage, exp_kind):
    """the C entry with pre-filled outputs: refused as exp_kind, and not one byte of the four arrays written"""
    from muscle_amd import _lib
    g = ctx(lib_path)
    exp = want(n, kind, transform, linkage)
    assert isinstance(exp, UpgmaDies) and exp.kind == exp_kind, (kind, transform, linkage, exp)
    tri = make_tri(n, kind, 1000 + n)
    out, keep = prefilled_outputs(n), prefilled_outputs(n)
    rc = g.L.mpcgpu_upgma(g.h, n, tri.ctypes.data, g.UPGMA_TRANSFORMS[transform], g.UPGMA_LINKAGES[linkage], *[a.ctypes.data for a in out])
    assert rc != 0
    try:
        g._ck(rc)
    except _lib.MpcGpuError as e:
        assert refusal_of(str(e)) == (exp.kind, exp.join), (str(e), exp)
    for a, b in zip(out, keep):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "an output array was written before the refusal"


def check_reuse(lib_path, big, small, env=None):
    """one context through: big, small (d_tri is kept), big with another matrix, a "no minimum" refusal, an EA refusal, small again, big
    again (after runs that ended by status). Every accepted call equals the restatement — which is what a fresh context returns, as the
    other cases show — and is also compared with a fresh context directly."""
    from muscle_amd import _lib
    calls = [(big, "quant", "scale", "avg"), (small, "quant", "none", "max"), (big, "random", "scale_dist", "biased"),
             (small, "nan_first", "scale", "avg"), (small, ("ea_one_bad", "above_1"), "ea", "avg"), (small, "quant", "scale", "min"),
             (big, "random", "none", "avg")]
    g = _lib.MpcGpu(0, lib_path=lib_path)
    try:
        kinds = []
        for n, kind, transform, linkage in calls:
            exp = want(n, kind, transform, linkage)
            tri = make_tri(n, kind, 1000 + n)
            what = "reuse: n=%d %s %s %s" % (n, kind, transform, linkage)
            got = check_call(g, n, tri, transform, linkage, exp, what)
            kinds.append(exp.kind if isinstance(exp, UpgmaDies) else "tree")
            if got is not None:
                f = _lib.MpcGpu(0, lib_path=lib_path)
                try:
                    assert_same_tree(got, f.upgma(n, tri, transform, linkage), what + " against a fresh context")
                finally:
                    f.close()
        assert kinds == ["tree", "tree", "tree", "no_min", "ea_range", "tree", "tree"], kinds
    finally:
        g.close()


def check_extremes(lib_path, n, cus):
    """Min and Max where only a later pass of the grid-stride loops, or a later round of the fold over the partials, finds them
    (extremes_positions for the CU count the launcher sees): the tree and mpcgpu_upgma_scale's bits"""
    m = n_tri(n)
    print("extremes: n", n, "CUs", cus, "grid", grid(m, cus), "passes", passes(m, cus), "rounds over the partials", fold_rounds(m, cus))
    for pos in extremes_positions(n, cus):
        for transform, linkage in (("scale", "avg"), ("scale_dist", "biased")):
            check_case(lib_path, n, ("extremes_at",) + pos, transform, linkage, lds=True)


def check_long_sequence_refused(lib_path):
    """a sequence of 65 536 positions: mpcgpu_set_seqs_registry takes it, mpcgpu_sw_tree refuses it by name before any device work"""
    import _golden as G
    import _sw
    from muscle_amd import _lib
    g = _lib.MpcGpu(0, lib_path=lib_path)
    try:
        g.set_hmm(*G.hmm_tables())
        g.set_seqs_registry(["A" * 65536, "MKVLA", "MKVLAA"])
        g.sw_set_scores(*_sw.tables())
        epoch = g.store_epoch()
        try:
            g.sw_tree()
        except _lib.MpcGpuError as e:
            assert "mpcgpu_sw_tree" in str(e) and "sequence 0" in str(e) and "65536 positions" in str(e), str(e)
        else:
            raise AssertionError("mpcgpu_sw_tree took a sequence of 65536 positions")
        assert g.store_epoch() == epoch
    finally:
        g.close()
