"""The case table of tests/_ea.py on the CPU: the inputs are what the table claims (lengths, bins, chains, the row-block pair, the
candidate counts behind the regrowth, the envelope), so that a green table on the device means the stated paths ran."""
import _align_pairs as A
import _ea


def lens(name):
    return [len(s) for s in _ea.case(name)["seqs"]]


def test_table_names_every_case():
    for name in _ea.CASES:
        c = _ea.case(name)
        n = len(c["seqs"])
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
