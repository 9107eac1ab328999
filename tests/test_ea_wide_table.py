"""The case table of tests/_ea_wide.py on the CPU: the inputs are what the table claims (lengths, which pairs are wide, the key forms
and radix passes, the candidate counts behind the regrowth), the default threshold follows from the post_rows_fits formula, and the
narrow remainder of any split always fits the row-list arrays — so that a green table on the device means the stated paths ran."""
import itertools

import _align_pairs as A
import _ea
import _ea_wide as W


def lens(name):
    return [len(s) for s in W.case(name)["seqs"]]


def test_table_names_every_case():
    assert set(W.CASES_FORCED) < set(W.CASES) and len(set(W.CASES)) == len(W.CASES)
    for name in W.CASES:
        c = W.case(name)
        n = len(c["seqs"])
        assert c["env"]["MPCGPU_EA_WIDE"] == "1" and 2 <= n <= 34, name
        for (x, y), (LX, LY) in zip(W.pairs_of(c), W.lens_of(c)):
            assert 0 <= x < n and 0 <= y < n and x != y, (name, x, y)
            assert not c["stage"] or x < y, (name, x, y)  # the second context's all-pairs stage holds the pair as (x, y)
            assert min(LX, LY) <= 110, (name, LX, LY)  # no pair of two long sequences: the oracle's DP stays small
            assert LX * LY * 5 + 100 <= _ea.INT_MAX
        assert any(W.is_wide(c)), name
        assert name in W.CASES_FORCED or "MPCGPU_EA_WIDE_MIN" not in c["env"], name


def test_default_threshold():
    assert W.wide_min_default() == 12115 == (A.POST_ROWS_LDS - 32 - 8 * A.POST_SORT_CAP) // 12 + 1
    assert W.post_rows_fits(12114, 12114) and not W.post_rows_fits(12115, 12115)
    assert W.wide_min_default(2) > 12115 > W.wide_min_default(4096)


def test_narrow_remainder_always_fits():
    """post_rows_fits is monotone in both arguments: pairs whose longer sequence stays below the threshold fit together, whatever mix
    of row and column lengths their list holds (the sub-list's geometry is the longest row and the longest column over all of them)"""
    for cap in (2, 1024, 4096):
        m = W.wide_min_default(cap)
        assert W.post_rows_fits(m - 1, m - 1, cap) and not W.post_rows_fits(m, m, cap)
        for a, b in itertools.product((1, 11, m // 2, m - 2, m - 1), repeat=2):
            assert W.post_rows_fits(a, b, cap), (cap, a, b)
        for a, b in ((1, 2), (100, 7), (m - 1, 1), (1, m - 1)):  # monotone: a step in either argument never turns "no" into "yes"
            assert W.post_rows_fits(a, b, cap) >= W.post_rows_fits(a + 1, b, cap) >= W.post_rows_fits(a + 1, b + 1, cap)


def test_edge():
    c = W.case("edge")
    assert lens("edge") == [12114, 12115, 11, 40] and W.wide_min_of(c) == 12115
    assert c["pairs"] == [(2, 0), (2, 1), (0, 3), (1, 3)] and W.is_wide(c) == [False, True, False, True]
    L = W.lens_of(c)
    assert L[1] == (11, 12115) and L[1][0] < A.LONG_MIN   # the long sequence as the column: the chain sweeps of bin 1
    assert L[3] == (12115, 40) and L[3][0] >= A.LONG_MIN  # ... as the row: row blocks
    assert not W.post_rows_fits(12115, 12115) and W.post_rows_fits(12114, 40)  # the narrow sub-list (11 x 12 114, 12 114 x 40) fits
    assert W.route("edge") == ((4, 2, 0, 2), (2, 1, 0, 1))


def test_long_keys():
    c = W.case("long_keys")
    assert W.lens_of(c) == [(40000, 11), (11, 40000)] and W.is_wide(c) == [True, True]
    bits = lambda v: v.bit_length()
    assert (16 + bits(40000 - 1) + 7) // 8 == 4  # MPC_KEY_ROW_SHIFT_LONG: the most passes a key of 32 bits can need
    assert (22 + bits(11 - 1) + 7) // 8 == 4     # MPC_KEY_ROW_SHIFT
    assert 40000 <= 65535 and 40000 >= A.LONG_MIN > 11
    assert W.route("long_keys") == ((2, 1, 0, 1), (2, 1, 0, 1))


def test_lds_forced():
    for name, lds in (("lds_forced", None), ("lds_forced_0", "0"), ("lds_forced_64", "64")):
        c = W.case(name)
        assert lens(name) == [100, 60, 97, 63, 40, 45] and c["env"].get("MPCGPU_POSTW_LDS") == lds and W.wide_min_of(c) == 50
        assert W.is_wide(c) == [True, True, False, True, True, True]
        assert W.route(name) == ((6, 2, 0, 2), (5, 1, 0, 1))
    cand = [w["cand"] for w in W.oracle("lds_forced")]
    assert max(cand) > 64 and min(len(s) for s in W.case("lds_forced")["seqs"][:4]) + 1 < 64 < 100 + 1  # 64: some lists and rows in LDS, some not


def test_regrowth_batches_tiny_mega():
    r = W.case("regrowth")
    cand = [w["cand"] for w in W.oracle("regrowth")]
    assert A.capc_of(W.lens_of(r), {}) == 1200 and max(cand) == cand[0] == 1627
    assert W.route("regrowth") == ((3, 1, 1, 2), (3, 1, 1, 2))
    b = W.case("batches")
    nw = sum(W.is_wide(b))
    assert 0 < nw < 66 and b["env"]["MPCGPU_SCRATCH_GB"] == "0"
    assert W.route("batches") == ((66, 66, 0, 66), (nw, nw, 0, nw)) == W.route("batches_reversed")
    assert W.case("batches_reversed")["pairs"] == _ea.all_pairs(12)[::-1]
    assert lens("tiny") == [1, 1, 2] and W.is_wide(W.case("tiny")) == [True] * 3
    assert [w["cand"] for w in W.oracle("tiny")] == [1, 2, 1]
    m = W.case("mega")
    assert m["mega"] is not None and len(m["seqs"]) == 4 and all(W.is_wide(m))


def test_persistent():
    """every workgroup of the persistent grid finishes more than one pair: 1024 threads are half the 2048 a CU holds, so at most
    2 workgroups x 256 CUs are resident, fewer than the pairs of the one batch"""
    c = W.case("persistent")
    assert len(W.pairs_of(c)) == 561 > 2 * 256 and all(W.is_wide(c)) and c["batches"] == "one"
    assert W.route("persistent") == ((561, 1, 0, 1), (561, 1, 0, 1))
