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


def _plan(name):
    seqs, s1, s2, env = _sw.case(name)
    return _sw.predict([len(x) for x in seqs], s1, s2, env)


def test_plan_of_the_existing_cuts():
    pr = _plan("chain_cut")  # 15 pairs of 47 columns, 94 columns per chain: rows of 5, 4, 3, 2, 1 pairs in 3 + 2 + 2 + 1 + 1 items
    assert sum(pr["items"]) == 9 and pr["items"][1] == 9 and pr["batches"] == 1
    assert [c[3] for c in pr["chains"]] == [2, 2, 1, 2, 2, 2, 1, 2, 1]
    pr = _plan("batch_cut")  # 66 pairs in batches of 7: nine full ones and one of 3, the (66 + 6) // 7 of check_case
    assert pr["batches"] == 10 and sum(c[3] for c in pr["chains"]) == 66
    assert all(sum(c[3] for c in pr["chains"] if c[0] == b) == (7 if b < 9 else 3) for b in range(10))
    pr = _plan("explicit_list")  # 3-4, 3-5, 3-6 chain; 0-0; 8-1 twice does not; 2-7, 2-8 chain; 2-3, 2-4 chain; 5-2; 1-0, 1-1 chain
    assert [c[3] for c in pr["chains"]] == [3, 1, 1, 1, 2, 2, 1, 2]
    pr = _plan("lane_bins")
    assert all(pr["items"][h] >= 1 for h in range(1, 9)) and pr["items"][_sw.LONG_BIN] == 0
    assert _plan("row_blocks")["items"][_sw.LONG_BIN] == 6
    assert _plan("ragged_all_pairs")["long_items"] == 0


def test_plan_of_long_chains():
    assert [len(s) for s in _sw.case("long_chains")[0]] == [600, 40, 513, 70, 1025, 33, 520]
    pr = _plan("long_chains")
    # all pairs: row i against i + 1 .. 6 is one item; the rows of 600, 513 and 1025 residues take the row-block kernel
    assert [(c[1], c[2], c[3]) for c in pr["chains"]] == [(9, 0, 6), (1, 1, 5), (9, 2, 4), (2, 3, 3), (9, 4, 2), (1, 5, 1)]
    assert pr["items"] == [0, 2, 1, 0, 0, 0, 0, 0, 0, 3] and pr["batches"] == 1
    assert pr["chains"][0][4] == 40 + 513 + 70 + 1025 + 33 + 520 + 6  # columns: every column sequence and its separator
    pr = _plan("long_chains_cols1")  # one pair per item
    assert pr["items"] == [0, 6, 3, 0, 0, 0, 0, 0, 0, 12] and all(c[3] == 1 for c in pr["chains"])
    pr = _plan("long_chains_batch4")  # 21 pairs: five batches of 4 and one of 1; the row of 600 residues is cut after its fourth pair
    assert pr["batches"] == 6 and [(c[0], c[2], c[3]) for c in pr["chains"]][:3] == [(0, 0, 4), (1, 0, 2), (1, 1, 2)]
    assert sum(c[3] for c in pr["chains"]) == 21 and max(c[3] for c in pr["chains"]) == 4
    # the three runs score the same pairs
    assert all(_sw.case(n)[:3] == _sw.case("long_chains")[:3] for n in ("long_chains_cols1", "long_chains_batch4"))


def test_plan_of_long_chain_separators():
    assert _sw.SEPARATOR_RUNS[0] == [1, 1, 2, 63, 64, 65, 1, 130]
    seps = [c for run in _sw.SEPARATOR_RUNS for c in _sw.separator_columns(run)]
    assert {63, 0, 1} <= {c % 64 for c in seps}  # columns 63, 64 and 65 of a 64-column chunk
    first = _sw.separator_columns(_sw.SEPARATOR_RUNS[0])
    assert first[:3] == [1, 3, 6] and first[6] - first[5] == 2  # back to back: one column between two separators
    for name, LA in (("long_chain_separators", 1025), ("long_chain_separators_513", 513), ("long_chain_separators_1024", 1024),
                     ("long_chain_separators_1536", 1536)):
        seqs, s1, s2, env = _sw.case(name)
        assert len(seqs[0]) == LA and seqs[-1] == seqs[0] and [len(x) for x in seqs[1:-1]] == _sw.SEPARATOR_RUNS[0] + _sw.SEPARATOR_RUNS[1]
        assert min(s1) < min(s2) and max(s1) > max(s2)  # the row sequence below and above its columns
        pr = _sw.predict([len(x) for x in seqs], s1, s2, env)
        assert [(c[1], c[3]) for c in pr["chains"]] == [(9, 8), (9, 8), (9, 6), (9, 6)]
        assert [c[4] for c in pr["chains"][::2]] == [sum(r) + len(r) for r in _sw.SEPARATOR_RUNS]


def test_plan_of_queue_reuse():
    # for a device of up to 304 CUs: more items than the waves of 8 workgroups per CU (bin 1) and of 2 per CU (row blocks)
    n, count = _sw.queue_reuse_sizes("gpu")
    seqs, s1, s2, env = _sw.queue_reuse_bin1(n)
    assert all(3 <= len(x) <= 8 for x in seqs) and len(set(seqs)) <= 12
    pr = _sw.predict([len(x) for x in seqs], s1, s2, env)
    assert pr["items"][1] == n * (n - 1) // 2 == sum(pr["items"]) and pr["items"][1] > 4 * 8 * _sw.QUEUE_CUS
    seqs, s1, s2, env = _sw.queue_reuse_long(count)
    assert [len(x) for x in seqs[:6]] == [513, 516, 520, 523, 527, 530] and [len(x) for x in seqs[6:]] == [4, 90] * 4
    pr = _sw.predict([len(x) for x in seqs], s1, s2, env)
    assert pr["items"][_sw.LONG_BIN] == count == sum(pr["items"]) and count > 4 * 2 * _sw.QUEUE_CUS
    assert all(a[4] != b[4] for a, b in zip(pr["chains"], pr["chains"][1:]))  # neighbouring items differ in their columns


def test_tables_case_properties():
    assert [t[:3] for t in _sw.TABLES] == [(1, 0.0, 0.0), (32, -0.3, -0.7), (4, -2.5, 0.0), (20, 0.0, -1.0), (20, -1.0, -11.0)]
    assert [t[3] for t in _sw.TABLES].count(False) == 1
    for k, (alpha, op, ex, symmetric) in enumerate(_sw.TABLES):
        (key, loc, sub, o, e), seqs = _sw.table_case(k)
        assert sub.shape == (alpha, alpha) and sub.dtype == np.float32 and np.array_equal(sub, sub.T) == symmetric
        assert [int(loc[ord("A") + l]) for l in range(alpha)] == list(range(alpha)) and (np.delete(loc, np.arange(65, 65 + alpha)) == alpha).all()
        assert [len(x) for x in seqs] == [5, 70, 130, 600, 31]
        letters = {int(loc[ord(ch)]) for x in seqs for ch in x}
        assert letters == set(range(alpha + 1))  # every letter and the wildcard
        if not symmetric:  # the order of a pair matters there
            want = _sw.want_scores(seqs, None, None, (key, loc, sub, o, e))
            pairs = _sw.pair_list(len(seqs))
            back = _sw.want_scores(seqs, [j for i, j in pairs], [i for i, j in pairs], (key, loc, sub, o, e))
            assert (_sw.bits(want) != _sw.bits(back)).any()


def test_dropin_set_reaches_the_other_bins():
    lens = [len(x) for x in _sw.dropin_seqs("swx_8x560_b4")]
    assert len(lens) == 8 and all(100 <= L - 1 <= 560 for L in lens) and sum(L - 1 > 512 for L in lens) >= 2
    pr = _sw.predict(lens)
    assert pr["items"][_sw.LONG_BIN] == 2 and pr["items"][1] == 0 and sum(1 for h in range(2, 9) if pr["items"][h]) >= 5
    assert all(x.endswith("X") for x in _sw.dropin_seqs("swx_8x560_b4"))
