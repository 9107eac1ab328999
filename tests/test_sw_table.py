"""The numpy restatement of the Smith-Waterman recurrence (tests/_sw.py sw_ref) against the bits of the compiled reference's
SWFast_Seqs_BLOSUM62 (tests/golden/sw_scores.npz: all pairs of 36 X-terminated sequences of lengths 2 .. 300), and the properties
of the case table the emulator and GPU tests rely on. No device, no library."""
import numpy as np

import _sw


def test_restatement_equals_reference_bits():
    g = _sw.golden()
    seqs, want = g["seqs"], g["scores"]
    n = len(seqs)
    assert n == 36 and len(want) == n * (n - 1) // 2 and all(s.endswith("X") and 2 <= len(s) <= 300 for s in seqs)
    assert seqs == _sw.golden_input()
    got = np.array([_sw.sw_ref(seqs[i], seqs[j]) for i in range(n) for j in range(i + 1, n)], np.float32)
    assert np.array_equal(_sw.bits(got), _sw.bits(want))
    assert (want == 0).any() and (want > 100).any()  # both ends of the range are in the fixture


def test_restatement_is_symmetric_and_order_matters():
    g = _sw.golden()
    a, b = g["seqs"][9], g["seqs"][20]
    assert _sw.bits(_sw.sw_ref(a, b)) == _sw.bits(_sw.sw_ref(b, a))
    # BLOSUM62 is fractional here (blosum.cpp:8): scores are no integers, so integer arithmetic could not reproduce them
    assert float(_sw.sw_ref(a, b)) != round(float(_sw.sw_ref(a, b)))


def test_tables_are_the_reference_ones():
    loc, sub, op, ex = _sw.tables()
    assert loc.shape == (256,) and sub.shape == (20, 20) and (op, ex) == (-11.0, -1.0)
    assert np.array_equal(sub, sub.T)
    assert [int(loc[ord(c)]) for c in _sw.AMINO] == list(range(20)) and loc[ord("X")] >= 20
    assert np.float32(sub[0, 0]) == np.float32(1.9646)


def test_case_table_properties():
    assert _sw.expected("no_positive_cell").tolist() == [0.0, 0.0, 0.0]
    assert (_sw.expected("wildcards")[:3] == 0).all()
    seqs, _, _, _ = _sw.case("identical")
    e = _sw.expected("identical")
    # identical sequences: the score is the sum of the diagonal, its best cell the last one (where the reference's trace-back dies)
    loc, sub, _, _ = _sw.tables()
    d = np.float32(0)
    for ch in seqs[0]:
        d = np.float32(d + sub[loc[ord(ch)], loc[ord(ch)]])
    assert _sw.bits(e[0]) == _sw.bits(d)
    lens = sorted(len(s) for s in _sw.case("lane_bins")[0])
    assert all(h * 64 + k in lens for h in range(1, 8) for k in (-1, 0, 1)) and 511 in lens and 512 in lens
    assert sorted(len(s) for s in _sw.case("row_blocks")[0])[-5:] == [513, 1023, 1024, 1025, 1089]
    lens = [len(s) for s in _sw.case("ragged_all_pairs")[0]]
    assert len(lens) == 40 and min(lens) == 1 and max(lens) == 300
