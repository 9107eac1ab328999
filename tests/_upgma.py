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
    """the reference asserts or dies on this input (upgma5.cpp:197-199, 512)"""


def tri_of(mx):
    """upper triangle, row-major: InitPairs order"""
    n = mx.shape[0]
    iu = np.triu_indices(n, 1)
    return np.ascontiguousarray(mx[iu], np.float32)


def mx_of(n, tri, diag=0.0):
    mx = np.full((n, n), diag, np.float32)
    iu = np.triu_indices(n, 1)
    mx[iu] = tri
    mx.T[iu] = tri
    return mx


def scale_dist_mx(mx, input_is_similarity=True):
    """upgma5.cpp:521-563 -> (new matrix, Min, Max)"""
    n = mx.shape[0]
    il = np.tril_indices(n, -1)
    d = mx[il].astype(np.float32)
    mn = min(F(mx[0, 1]), d.min())
    ma = max(F(mx[0, 1]), d.max())
    SCALE = F(10.0)
    with np.errstate(all="ignore"):
        if input_is_similarity:
            nd = (SCALE * (ma - d)) / (ma - mn)
        else:
            nd = (SCALE * (d - mn)) / (ma - mn)
    assert nd.dtype == np.float32
    out = mx.copy()
    out[il] = nd
    out.T[il] = nd
    return out, mn, ma


def fix_ea_dist_mx(mx):
    """upgma5.cpp:504-519"""
    n = mx.shape[0]
    il = np.tril_indices(n, -1)
    d = mx[il].astype(np.float32)
    if not np.all((d >= 0) & (d <= 1)):
        raise UpgmaDies("asserta(d >= 0 && d <= 1), upgma5.cpp:512")
    nd = F(1) - d
    out = mx.copy()
    out[il] = nd
    out.T[il] = nd
    np.fill_diagonal(out, 0)
    return out


def transform_mx(mx, transform):
    if transform == "scale":
        return scale_dist_mx(mx, True)[0]
    if transform == "scale_dist":
        return scale_dist_mx(mx, False)[0]
    if transform == "ea":
        return fix_ea_dist_mx(mx)
    assert transform == "none"
    return mx.copy()


def _first_min_below_flt_max(vals, idx):
    """ascending scan with 'd < best', best starting at FLT_MAX, over vals (at the ascending indices idx) -> (best, index or NONE)"""
    ok = vals < FLT_MAX  # NaN: false, as in the scan
    if not ok.any():
        return F(FLT_MAX), NONE
    v = vals[ok]
    k = int(np.argmin(v))  # first occurrence of the minimum
    return F(v[k]), int(idx[ok][k])


def run(mx, linkage="avg"):
    """UPGMA5::Run on the (already transformed) matrix -> (left, right, left_len, right_len, height), n - 1 entries each"""
    n = mx.shape[0]
    assert n >= 2 and linkage in LINKAGES
    D = mx.astype(np.float32).copy()
    D[D < 0] = 0  # upgma5.cpp:140-145 (-0.0 and NaN are not below 0)
    allj = np.arange(n)
    min_dist = np.full(n, FLT_MAX, np.float32)
    nearest = np.full(n, NONE, np.int64)
    node = np.arange(n, dtype=np.int64)
    for i in range(n):  # upgma5.cpp:133-157: row i meets its partners in ascending order
        others = allj[allj != i]
        min_dist[i], nearest[i] = _first_min_below_flt_max(D[i, others], others)
    left = np.full(n - 1, NONE, np.uint32)
    right = np.full(n - 1, NONE, np.uint32)
    llen = np.full(n - 1, FLT_MAX, np.float32)
    rlen = np.full(n - 1, FLT_MAX, np.float32)
    height = np.full(n - 1, FLT_MAX, np.float32)
    c01, c09 = F(0.1), F(1) - F(0.1)
    for k in range(n - 1):
        live = allj[node != NONE]
        _, L = _first_min_below_flt_max(min_dist[live], live)  # upgma5.cpp:178-195
        if L == NONE:
            raise UpgmaDies("assert(Lmin != UINT_MAX) at join %d, upgma5.cpp:197" % k)
        R = int(nearest[L])
        if R == NONE or node[R] == NONE or R == L:
            raise UpgmaDies("assert(UINT_MAX != Rmin) at join %d, upgma5.cpp:192-193" % k)
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
        nearest[js[nearest[js] == R]] = L  # upgma5.cpp:249-259
        D[L, js] = nd
        D[js, L] = nd
        new_min, new_nn = _first_min_below_flt_max(nd, js)
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
    diag = FLT_MAX if transform == "none" else 0.0
    return run(transform_mx(mx_of(n, tri, diag), transform), linkage)[:4]


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
def make_tri(n, kind, seed):
    """seeded triangle of n leaves: "random" in (0, 1); "quant": 4 distinct values (ties, the redirect, stale minima); "negative": some
    entries below 0; "fltmax": two entries FLT_MAX"""
    rng = np.random.default_rng(seed)
    m = n * (n - 1) // 2
    t = rng.random(m).astype(np.float32)
    if kind == "quant":
        t = (np.floor(t * 4) / 4 + 0.125).astype(np.float32)
        if m >= 2:
            t[0], t[-1] = F(0.125), F(0.875)  # two distinct values also at the smallest sizes
    elif kind == "negative":
        t = (t - F(0.3)).astype(np.float32)
    elif kind == "fltmax":
        # two entries: an average of two FLT_MAX is infinite and is never a minimum again, so a matrix with many of them ends in the
        # reference's assert under every linkage but "min" (as this one does under "max": the last join is the largest entry)
        t[rng.choice(m, size=min(2, m), replace=False)] = FLT_MAX
        if m >= 2:
            t[0], t[-1] = F(0.25), F(0.75)
    else:
        assert kind == "random"
    return t


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


def assert_same_tree(got, exp, what):
    for name, g, w in zip(("left", "right", "left_len", "right_len"), got, exp):
        if name in ("left", "right"):
            assert np.array_equal(np.asarray(g, np.uint32), np.asarray(w, np.uint32)), "%s: %s differs" % (what, name)
        else:
            gb, wb = np.asarray(g, np.float32).view(np.uint32), np.asarray(w, np.float32).view(np.uint32)
            assert np.array_equal(gb, wb), "%s: the bits of %s differ at %s" % (what, name, np.nonzero(gb != wb)[0][:8])


def check_case(lib_path, n, kind, transform, linkage, lds):
    """mpcgpu_upgma against the restatement: node indices equal, float bits of the lengths equal; where the reference dies, a refusal by
    name; mpcgpu_upgma_info must name the path (lds: the row state in LDS or in global memory)"""
    from muscle_amd import _lib
    g = ctx(lib_path)
    exp = want(n, kind, transform, linkage)
    tri = make_tri(n, kind, 1000 + n)
    what = "n=%d %s %s %s" % (n, kind, transform, linkage)
    if isinstance(exp, UpgmaDies):
        try:
            g.upgma(n, tri, transform, linkage)
        except _lib.MpcGpuError as e:
            assert "mpcgpu_upgma:" in str(e), str(e)
            return
        raise AssertionError("%s: the reference dies here (%s), the library returned a tree" % (what, exp))
    got = g.upgma(n, tri, transform, linkage)
    info = g.upgma_info()
    assert info[0] == n and info[1] == (1 if lds else 0), (what, info)
    assert_same_tree(got, exp, what)
