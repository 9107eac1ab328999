"""The case table of tests/_ea.py on the CPU: the inputs are what the table claims (lengths, bins, chains, the row-block pair, the
candidate counts behind the regrowth, the envelope), so that a green table on the device means the stated paths ran."""
import numpy as np
import pytest

import _align_pairs as A
import _ea


def lens(name):
    return [len(s) for s in _ea.case(name)["seqs"]]


PERSISTENT = {"persistent", "persistent_sort_mixed", "persistent_small", "persistent_overflow", "persistent_overflow_small", "persistent_sort_mixed_small"}
CUS = 256  # the device the persistent cases are sized for


def cands(name):
    return [w["cand"] for w in _ea.oracle(name)]


def test_table_names_every_case():
    assert sorted(_ea.CASES) == sorted(set(_ea.CASES)) and set(_ea.CASES_DEVICE) < PERSISTENT < set(_ea.CASES)
    for name in _ea.CASES:
        c = _ea.case(name)
        n = len(c["seqs"])
        if name in PERSISTENT:  # 34 sequences (and the poly-A pair), one long column
            assert n in (34, 36) and sorted(lens(name))[-2] <= 400 and max(lens(name)) == (600 if name.endswith("_small") else 9800), name
        else:
            assert 2 <= n <= 13 and max(lens(name)) <= 769, name
        for x, y in (c["pairs"] or _ea.all_pairs(n)):
            assert 0 <= x < y < n, (name, x, y)  # (x < y: the second context's all-pairs stage holds every pair of every list)


def test_tiny():
    assert lens("tiny_n2") == [3, 4] and lens("tiny_1_1_2") == [1, 1, 2]
    cand = [w["cand"] for w in _ea.oracle("tiny_1_1_2")]
    assert cand == [1, 2, 1], cand  # a 1 x 1 pair keeps its one cell: no list is empty under these tables; P x WP keeps one of its two
    assert all(min(len(a), len(b)) == 1 for a, b in [("W", "P"), ("W", "WP"), ("P", "WP")])
    assert float(_ea.oracle("tiny_1_1_2")[0]["ea"]) == 1.0


def test_bin_edges():
    assert lens("bin_edges") == [63, 64, 65, 128, 129, 512, 513] == lens("bin_edges_reversed")
    rows = {(L + 63) // 64 for L in lens("bin_edges")[:-1]}  # the last sequence is a column only
    assert rows == {1, 2, 3, 8} and (513 + 63) // 64 == 9
    assert _ea.case("bin_edges")["pairs"] is None
    assert _ea.case("bin_edges_reversed")["pairs"] == _ea.all_pairs(7)[::-1]
    assert _ea.fb_launches(_ea.case("bin_edges")) == 4


def test_chains():
    """a chain (mpcgpu_stage_a.inc: build_chains): consecutive pairs with the same row sequence, every column sequence with LY + 1 >= T"""
    c = _ea.case("chaining")
    L = lens("chaining")
    H = (L[0] + 63) // 64
    T = (L[0] + H - 1) // H
    assert [x for x, _ in c["pairs"]] == [0] * 5 and all(L[y] + 1 >= T for _, y in c["pairs"])
    rows = [x for x, _ in _ea.case("no_chain")["pairs"]]
    assert len(set(rows)) == len(rows) == 3


def test_row_blocks():
    c = _ea.case("row_blocks")
    L = lens("row_blocks")
    long_pairs = [(x, y) for x, y in c["pairs"] if L[x] >= _ea.LONG_MIN]
    assert long_pairs == [(0, 1)] and (L[0], L[1]) == (769, 70)
    assert _ea.fb_launches(c) == 3  # the row-block launch, bins 1 and 2


def test_batches_and_regrowth():
    c = _ea.case("batches")
    assert len(c["seqs"]) == 12 and c["env"] == {"MPCGPU_SCRATCH_GB": "0"} and c["batches"] == 66 >= 3
    r = _ea.case("regrowth")
    pairs = [(len(r["seqs"][x]), len(r["seqs"][y])) for x, y in _ea.all_pairs(3)]
    cand = [w["cand"] for w in _ea.oracle("regrowth")]
    assert A.capc_of(pairs, {}) == 1200 and max(cand) == cand[0] == 1627
    assert A.regrowths(pairs, cand, {}) == 1 == r["regrow"]


def test_mega_and_envelope():
    m = _ea.case("mega")
    assert len(m["seqs"]) == 4 and m["mega"] is not None and len(m["mega"]["profs"]) == 4  # every profile bb11001.mega holds
    assert all(len(p) == len(s) * len(m["mega"]["alpha"]) for p, s in zip(m["mega"]["profs"], m["seqs"]))
    assert 25000 * 25000 * 5 + 100 > _ea.INT_MAX >= 11 * 25000 * 5 + 100


# ---- the persistent loop ------------------------------------------------------------------------------------------------------------
def workgroups(flags, grid):
    """per workgroup of a persistent grid the flags of the pairs it finishes, in its order: pid = w, w + grid, w + 2 grid, ..."""
    return [flags[w::grid] for w in range(grid)]


def both_orders(flags, grid):
    """some workgroup finishes a flagged pair and right after it an unflagged one, and some workgroup the other way round"""
    steps = {(a, b) for wg in workgroups(flags, grid) for a, b in zip(wg, wg[1:])}
    return (True, False) in steps and (False, True) in steps


@pytest.mark.parametrize("name", ["persistent", "persistent_sort_mixed", "persistent_overflow"])
def test_persistent_for_256_cus(name):
    """B > CUs * (152 KB // smem): whatever occupancy the runtime reports, the grid is smaller than the batch"""
    c = _ea.case(name)
    L = _ea.lens_of(c)
    smem, cap = _ea.post_ea_smem(L, c["env"])
    assert c["batches"] == 1 and len(L) in (561, 562)
    assert max(a for a, _ in L) <= 400 and max(b for _, b in L) == 9800  # the long sequence is a column only: no row-block pair
    assert (34 + 2 + 2 * 9802) * 4 <= smem - 8 * cap <= (400 + 2 + 2 * 9802) * 4 and smem > _ea.POST_EA_LDS_PER_CU // 2
    G = _ea.grid_bound(c, CUS)
    assert G == CUS * (_ea.POST_EA_LDS_PER_CU // smem) == 256 and len(L) > 2 * G  # every workgroup finishes at least two pairs
    is_long = [b == 9800 for _, b in L]
    at = [k for k, f in enumerate(is_long) if f]
    assert len(at) == 33 and at[0] < G <= at[-1]
    assert both_orders(is_long, G)  # stale per-position arrays both ways: a long pair then a short one, a short one then a long one
    assert any(wg[0] != wg[1] for wg in workgroups(L, G))
    assert _ea.fb_launches(c) == 1 + (name == "persistent_overflow")  # rows below 64 positions; the poly-A pair has 300


def test_persistent_small_on_two_cus():
    """the emulator's device: 2 CUs, one workgroup each"""
    for name in ("persistent_small", "persistent_overflow_small"):
        c = _ea.case(name)
        L = _ea.lens_of(c)
        assert c["batches"] == 1 and len(L) > 2 and max(a for a, _ in L) <= 60 and max(b for _, b in L) == 600
        assert both_orders([b == 600 for _, b in L], 2)
    assert max(cands("persistent")) <= 1024 and max(cands("persistent_small")) <= 1024  # at the default cap every list is in LDS
    assert _ea.expected_regrowths("persistent") == 0 == _ea.expected_regrowths("persistent_small")


@pytest.mark.parametrize("name,grid,room", [("persistent_overflow", 256, 9800), ("persistent_overflow_small", 2, 1024)])
def test_persistent_overflow(name, grid, room):
    c = _ea.case(name)
    L, cand = _ea.lens_of(c), cands(name)
    assert c["pairs"][_ea.OVERFLOW_AT] == (34, 35) and sorted(c["pairs"][:_ea.OVERFLOW_AT] + c["pairs"][_ea.OVERFLOW_AT + 1:]) == _ea.all_pairs(34)
    assert A.capc_of(L, c["env"]) == room and min(_ea.grid_bound(c, CUS), grid) == grid
    assert [k for k, n in enumerate(cand) if n > room] == [_ea.OVERFLOW_AT]  # exactly the intended pair overflows the first room
    assert room < cand[_ea.OVERFLOW_AT] <= 2 * room and _ea.expected_regrowths(name) == 1 == c["regrow"]
    wg = workgroups(list(range(len(L))), grid)[_ea.OVERFLOW_AT % grid]
    assert wg.index(_ea.OVERFLOW_AT) + 2 < len(wg) + (grid == 256)  # its workgroup goes on with good pairs (two more on 256 CUs)
    assert wg[-1] > _ea.OVERFLOW_AT


# ---- the sorted list in LDS or in the scratch slot --------------------------------------------------------------------------------
def test_sort_cap_sides():
    c = _ea.case("sort_cap_8")
    assert c["seqs"] == _ea.case("chaining")["seqs"] and c["pairs"] == _ea.case("chaining")["pairs"]
    assert _ea.post_ea_smem(_ea.lens_of(c), c["env"])[1] == 8 < min(cands("sort_cap_8"))  # every list goes through the slot
    assert _ea.post_ea_smem(_ea.lens_of(c), {})[1] == 1024 >= max(cands("chaining"))   # ... and none does in "chaining"
    for name, base, cap, lds, slot in (("sort_cap_mixed", "bin_edges", 160, 11, 10), ("persistent_sort_mixed", "persistent", 53, 285, 276),
                                        ("persistent_sort_mixed_small", "persistent_small", 57, 287, 274)):
        c, cand = _ea.case(name), cands(name)
        assert c["seqs"] == _ea.case(base)["seqs"] and c["pairs"] == _ea.case(base)["pairs"] and c["same_as"] == base
        assert _ea.post_ea_smem(_ea.lens_of(c), c["env"])[1] == cap == int(c["env"]["MPCGPU_POST_SORT_CAP"])
        assert min(cand) < cap < max(cand) <= A.capc_of(_ea.lens_of(c), c["env"])
        assert (sum(n <= cap for n in cand), sum(n > cap for n in cand)) == (lds, slot) and min(lds, slot) >= 2
        assert cand.count(cap) >= 1  # c == sort_cap: the last list that stays in LDS
    # one workgroup alternates between the LDS list and its slot, both ways
    c = _ea.case("persistent_sort_mixed")
    assert both_orders([n > 53 for n in cands("persistent_sort_mixed")], _ea.grid_bound(c, CUS))
    assert both_orders([n > 57 for n in cands("persistent_sort_mixed_small")], 2)  # (the emulator's grid)


# ---- the multi-pass EA row -----------------------------------------------------------------------------------------------------------
def row_counts(name):
    return np.concatenate([w["rows"] for w in _ea.oracle(name)])


@pytest.mark.parametrize("name,base", [("post_batch_1", "bin_edges"), ("post_batch_3", "bin_edges"),
                                       ("post_batch_1_polya", "regrowth"), ("post_batch_3_polya", "regrowth")])
def test_rows_above_the_forced_batch(name, base):
    c = _ea.case(name)
    batch = int(c["env"]["MPCGPU_POST_BATCH"])
    assert c["seqs"] == _ea.case(base)["seqs"] and c["pairs"] == _ea.case(base)["pairs"] and c["rerun"] == {} and c["same_as"] == base
    rows = row_counts(name)
    assert rows.sum() == sum(cands(name))
    assert np.count_nonzero(rows > batch) >= 10 and rows.max() <= 64  # (no row is multi-pass at the default batch of 64)
    if batch == 3:
        assert np.any((rows > 3) & (rows % 3 != 0)) and np.any((rows > 3) & (rows % 3 == 0)) and np.any(rows == 3)
    assert c["regrow"] == _ea.case(base)["regrow"] == _ea.expected_regrowths(name)


def test_row_over_64():
    c = _ea.case("row_over_64")
    assert c["env"] == {} and c["pairs"] is None and lens("row_over_64") == [78, 141, 90]
    per_pair = [int(w["rows"].max()) for w in _ea.oracle("row_over_64")]
    assert per_pair[0] == 65 > 64 >= max(per_pair[1:])  # one row of "A" * 78 x "A" * 141 holds 65 cells: two passes at the default batch
    assert 64 < 65 <= 3 * 32 and c["rerun"] == {"MPCGPU_POST_BATCH": "32"}  # ... and three under the rerun's
    L = _ea.lens_of(c)
    assert A.capc_of(L, {}) == 12 * 141 < cands("row_over_64")[0] == 2115 <= 2 * 12 * 141 and _ea.expected_regrowths("row_over_64") == 1 == c["regrow"]
    # no base case has such a row: without this one the branch runs only where the batch is forced
    assert all(int(w["rows"].max()) <= 64 for name in ("bin_edges", "chaining", "regrowth", "row_blocks") for w in _ea.oracle(name))


# ---- an overflow between batches -----------------------------------------------------------------------------------------------------
def test_batches_regrowth():
    c = _ea.case("batches_regrowth")
    L, cand = _ea.lens_of(c), cands("batches_regrowth")
    assert c["env"] == {"MPCGPU_SCRATCH_GB": "0"} and c["batches"] == len(c["pairs"]) == 7 >= 5 and c["each"]
    assert c["pairs"][3] == (5, 6) and L[3] == (60, 100)  # three batches before the poly-A pair, three behind it
    assert A.capc_of(L, c["env"]) == 1200 and [k for k, n in enumerate(cand) if n > 1200] == [3] and cand[3] == 1627 <= 2400
    assert A.regrowths_each(L, cand, c["env"]) == 1 == c["regrow"]
    r = _ea.case("batches_regrowth_reversed")
    assert r["pairs"] == c["pairs"][::-1] and r["seqs"] == c["seqs"] and r["env"] == c["env"] and r["same_as"] == "batches_regrowth"
    assert _ea.expected_regrowths("batches_regrowth_reversed") == 1 == r["regrow"]


def test_batches_regrowth_twice():
    c = _ea.case("batches_regrowth_twice")
    L, cand = _ea.lens_of(c), cands("batches_regrowth_twice")
    assert c["env"] == {"MPCGPU_SCRATCH_GB": "0", "MPCGPU_CAND_PER_ROW": "1"} and c["batches"] == len(c["pairs"]) == 8 and c["each"]
    assert A.capc_of(L, c["env"]) == 1024 and [k for k, n in enumerate(cand) if n > 1024] == [2, 5]
    assert (L[2], L[5]) == ((60, 100), (100, 150))
    # the room doubles once for the first (1024 -> 2048) and, kept for the rest of the list, once more for the second (-> 4096) ...
    assert 1024 < cand[2] == 1627 <= 2048 < cand[5] == 3318 <= 4096
    assert A.regrowths_each(L, cand, c["env"]) == 2 == c["regrow"]
    # ... where a room that fell back to 1024 behind the redone batch would double twice for the second: 3 regrowths
    assert sum(A.regrowths(L, [n], c["env"]) for n in cand) == 3
