"""What the field-width cases of the long form of the record store are claimed to contain (tests/_relax_long.py: FIELD, field_seqs),
from the oracle's stage-0 matrices and record_layout, the numpy restatement of var_build_long_kernel's placement. No device, no
library: a case that loses a claim fails here, before any device run. Run with -s to read the counts."""
import numpy as np
import pytest

import _relax_long as L
import _store_segments as S
import _relax as R


def test_layout_restatement_small():
    """record_layout on the forced small shapes: the record sizes are those of record_blocks and of _store_segments.record_sizes,
    every entry has a position of its own inside its record, a row's blocks are chained first block -> overflow run by the distances,
    and the words of a block decode (mpc_blk_col1 / mpc_blk_dist) to the column and the distance that went in"""
    seqs = L.forced_seqs(9)
    n = len(seqs)
    lays = L.layouts(seqs)
    blocks, _ = S.record_sizes(seqs, R.oracle(seqs)[0][0])
    assert max(l["blocks"] for l in lays.values()) == L.record_blocks(seqs)
    for (A, Z), lay in lays.items():
        LA = len(seqs[A])
        assert lay["blocks"] == blocks[Z * n + A], (A, Z)
        assert len(set(lay["pos"].tolist())) == len(lay["pos"]) and (lay["pos"] < 2 * lay["blocks"]).all(), (A, Z)
        first = lay["unit"] < LA
        assert np.array_equal(lay["db"][first & (lay["db"] > 0)], lay["dist"][lay["unit"][first & (lay["db"] > 0)]]), (A, Z)
        w = L.record_words(lay, LA)
        z, ww = w[lay["unit"], 0], w[lay["unit"], 1]
        assert np.array_equal((z >> 16) | (ww & 0xffff0000), lay["db"]), (A, Z, "distance")
        assert np.array_equal(np.where(lay["slot"] == 0, z & 0xffff, ww & 0xffff), lay["col"]), (A, Z, "column")
        # the overflow runs of the rows follow each other in row order and end the record
        many = np.nonzero(lay["nb"] > 1)[0]
        if len(many):
            assert lay["ovf0"][many[0]] == LA and lay["ovf0"][many[-1]] + lay["nb"][many[-1]] - 1 == lay["blocks"], (A, Z)


@pytest.mark.parametrize("name", sorted(L.FIELD))
def test_field_case_claims(name):
    seqs = L.field_seqs(name)
    c = L.field_counts(seqs)
    print("\n%s: lengths %s" % (name, [len(s) for s in seqs]))
    print("  rows by dist.hi of the first block (with lo != 0): hi=0 %d (%d), hi=1 %d (%d), hi>=2 %d (%d)"
          % (c["hi0"], c["hi0_lo"], c["hi1"], c["hi1_lo"], c["hi2"], c["hi2_lo"]))
    print("  columns: <0x1fff %d, ==0x1fff %d, (0x1fff,0x7fff] %d, ==0x7fff %d, ==0x8000 %d, >0x8000 %d"
          % (c["col_lt_1fff"], c["col_1fff"], c["col_1fff_7fff"], c["col_7fff"], c["col_8000"], c["col_gt_8000"]))
    print("  entry positions >= 65536: %d; rows of >= 3 blocks: %d; empty rows: %d; largest record: %d blocks"
          % (c["pos_ge_65536"], c["rows_3_blocks"], c["rows_empty"], c["max_blocks"]))
    for claim in L.FIELD[name]:
        assert c[claim] > 0, (name, "the case lost its claim", claim, c)
    # the library's own trigger (build_var_store): a sequence above MPC_RV_MAXLEN = 4095 and at most MPC_RL_MAXLEN = 65 534
    assert 4095 < max(len(s) for s in seqs) <= 65534, name
    if name == "dist_hi":
        assert sum(len(a) * len(b) for i, a in enumerate(seqs) for b in seqs[i + 1:]) < 3 * 10 ** 6


def test_maxlen_is_the_limit():
    assert [len(s) for s in L.field_seqs("maxlen")] == [65534, 40, 55, 30]
    assert [len(s) for s in L.field_seqs("over")] == [65535, 40, 55, 30]
    assert L.field_seqs("over")[0][:65534] == L.field_seqs("maxlen")[0] and L.field_seqs("over")[1:] == L.field_seqs("maxlen")[1:]
