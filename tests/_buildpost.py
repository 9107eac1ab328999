"""Test-side restatement of MPCFlat::BuildPost (buildpostflat.cpp:18-106) in numpy float32, in the
reference's loop order (s in MSA1 outer, t in MSA2 inner, rows ascending, entries ascending; weights
1.0f as at mpcflat.cpp:324), and of CalcPosteriorFlat3 (buildposterior3flat.cpp:19-85, pair-list order):
a loop form for small cases and a vectorised form (one float32 add per pair) for production shapes;
helpers to make aligned rows. TEST INFRASTRUCTURE."""
import numpy as np


def pos_to_col(aligned_row):
    """Sequence::GetPosToCol (sequence.cpp:144-154): column of every residue of a gapped row."""
    return np.array([c for c, ch in enumerate(aligned_row) if ch != "-"], np.uint32)


def build_post(store_stage, pairs_index, seq1, seq2, p2c1, p2c2, C1, C2, w1=None, w2=None):
    """store_stage: list over pair index of (offsets, values u32 interleaved {P bits, col});
    pairs_index: dict (i,j)->k for i<j; w1/w2: sequence weights per row (default 1.0f)."""
    post = np.zeros((C1, C2), np.float32)
    for a, S in enumerate(seq1):
        for b, T in enumerate(seq2):
            w = np.float32(1.0 if w1 is None else w1[a]) * np.float32(1.0 if w2 is None else w2[b])  # w1*w2, rounded first
            if S < T:  # buildpostflat.cpp:56-77
                off, val = store_stage[pairs_index[(S, T)]]
                p, col = val[0::2].view(np.float32), val[1::2]
                for i in range(len(off) - 1):
                    for k in range(off[i], off[i + 1]):
                        post[p2c1[a][i], p2c2[b][col[k]]] += w * p[k]
            else:      # buildpostflat.cpp:78-100
                off, val = store_stage[pairs_index[(T, S)]]
                p, col = val[0::2].view(np.float32), val[1::2]
                for i in range(len(off) - 1):
                    for k in range(off[i], off[i + 1]):
                        post[p2c1[a][col[k]], p2c2[b][i]] += w * p[k]
    return post


def _entries(off, val):
    """(row, col, P) of every stored entry of one MySparseMx-layout matrix, rows ascending, entries ascending"""
    off = np.asarray(off, np.int64)
    rows = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    return rows, np.asarray(val[1::2], np.int64), np.ascontiguousarray(val[0::2]).view(np.float32)


class _PairEntries:
    """_entries of the stored pairs, each computed once"""

    def __init__(self, store_stage, pairs_index):
        self.stage, self.pidx, self.memo = store_stage, pairs_index, {}

    def __call__(self, S, T):
        k = self.pidx[(min(S, T), max(S, T))]
        if k not in self.memo:
            self.memo[k] = _entries(*self.stage[k])
        return self.memo[k]


def build_post_fast(store_stage, pairs_index, seq1, seq2, p2c1, p2c2, C1, C2, w1=None, w2=None):
    """build_post, one fancy-indexed float32 add per (s, t) pair in the same pair order. Within one pair every stored entry lands
    in a distinct cell (both position -> column maps rise strictly), so post[cells] += w * p adds the same terms to every cell
    in the same order as the loop."""
    post = np.zeros(C1 * C2, np.float32)
    ent = _PairEntries(store_stage, pairs_index)
    m1 = [np.asarray(x, np.int64) for x in p2c1]
    m2 = [np.asarray(x, np.int64) for x in p2c2]
    for a, S in enumerate(seq1):
        for b, T in enumerate(seq2):
            w = np.float32(1.0 if w1 is None else w1[a]) * np.float32(1.0 if w2 is None else w2[b])  # w1*w2, rounded first
            rows, cols, p = ent(S, T)
            if S < T:
                cell = m1[a][rows] * C2 + m2[b][cols]
            else:  # stored (T, S): rows are positions of T
                cell = m1[a][cols] * C2 + m2[b][rows]
            post[cell] += w * p
    return post.reshape(C1, C2)


def build_post_list(sparse, p2c1, p2c2, C1, C2):
    """CalcPosteriorFlat3 (buildposterior3flat.cpp:19-85) of a pair list: sparse[q] = (offsets, values) of pair q with the MSA1
    sequence on the rows; p2c1[q] / p2c2[q] its two rows' maps. Flat[col1 * C2 + col2] += P, pair after pair in list order."""
    post = np.zeros((C1, C2), np.float32)
    for q, (off, val) in enumerate(sparse):
        p, col = val[0::2].view(np.float32), val[1::2]
        for r in range(len(off) - 1):
            for k in range(off[r], off[r + 1]):
                post[p2c1[q][r], p2c2[q][col[k]]] += p[k]  # buildposterior3flat.cpp:81
    return post


def build_post_list_fast(sparse, p2c1, p2c2, C1, C2):
    """build_post_list, one fancy-indexed float32 add per pair of the list, in list order"""
    post = np.zeros(C1 * C2, np.float32)
    for q, (off, val) in enumerate(sparse):
        rows, cols, p = _entries(off, val)
        post[np.asarray(p2c1[q], np.int64)[rows] * C2 + np.asarray(p2c2[q], np.int64)[cols]] += p
    return post.reshape(C1, C2)


def term_counts(store_stage, pairs_index, seq1, seq2, p2c1, p2c2, C1, C2):
    """-> (terms per cell (C1, C2) int64, total contributions) of build_post: every stored entry of every cross pair lands in
    exactly one cell"""
    cells = []
    ent = _PairEntries(store_stage, pairs_index)
    for a, S in enumerate(seq1):
        m1 = np.asarray(p2c1[a], np.int64)
        for b, T in enumerate(seq2):
            m2 = np.asarray(p2c2[b], np.int64)
            rows, cols, _ = ent(S, T)
            cells.append((m1[rows] * C2 + m2[cols] if S < T else m1[cols] * C2 + m2[rows]).astype(np.uint32))
    cells = np.concatenate(cells) if cells else np.zeros(0, np.uint32)
    return np.bincount(cells, minlength=C1 * C2).reshape(C1, C2), len(cells)


def row_chunk_max(store_stage, pairs_index, seq1, seq2, p2c1, C1, chunk=64):
    """The largest list the row form of the device BuildPost (kernels_prog.h: build_post_one_row) fills: for every output row
    col1 and every chunk of `chunk` consecutive (a, b) pairs (a-major), the entries of row pos_a(col1) of the ordered matrix
    M(seq1[a], seq2[b]), summed over the chunk."""
    n1, n2 = len(seq1), len(seq2)
    ent = _PairEntries(store_stage, pairs_index)
    per = np.zeros((n1 * n2, C1), np.int64)  # entries each pair adds to each output row
    for a, S in enumerate(seq1):
        m1 = np.asarray(p2c1[a], np.int64)
        for b, T in enumerate(seq2):
            rows, cols, _ = ent(S, T)
            per[a * n2 + b] = np.bincount(m1[rows if S < T else cols], minlength=C1)
    tot = np.add.reduceat(per, np.arange(0, n1 * n2, chunk), axis=0)
    return int(tot.max())


def random_msa(seqs, idxs, rng, extra=0):
    """A random gapped alignment of the given sequences (same width): rows as strings. extra: more gap columns."""
    width = max(len(seqs[i]) for i in idxs) + int(rng.integers(0, 6)) + extra
    rows = []
    for i in idxs:
        s = seqs[i]
        cols = np.sort(rng.choice(width, size=len(s), replace=False))
        row = ["-"] * width
        for ch, c in zip(s, cols):
            row[c] = ch
        rows.append("".join(row))
    return rows, width
