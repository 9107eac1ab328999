"""CPU checks of the align_pairs case table (tests/_align_pairs.py): ap_oracle reproduces the compiled reference's AlignPairFlat_SparsePost
(ap_ragged.npz) bit for bit, the path predictor puts every case of both tables on the path it claims, every overflow case's candidate
list is longer than the room the library gives it, and the GPU table stays within its oracle budget."""
import numpy as np
import pytest

import _align_pairs as A
import _golden as G


def test_ap_oracle_matches_reference_golden():
    z = G.load("ap_ragged")
    seqs = [str(x) for x in z["seqs"]]
    pairs = [(int(a), int(b)) for a, b in z["pairs"]]
    assert len(pairs) == 12
    h = A.hmm()[0]
    for q, (a, b) in enumerate(pairs):
        w = A.ap_oracle(h, seqs[a].encode(), seqs[b].encode())
        assert w["path"] == str(z["p%d_path" % q]), q
        assert A.bits(w["ea"]) == A.bits(z["p%d_ea" % q]), q
        assert np.array_equal(w["off"], z["p%d_off" % q]) and np.array_equal(w["val"], z["p%d_val" % q]), q


@pytest.mark.parametrize("size", ["gpu", "emu"])
def test_predictor_puts_every_case_on_its_path(size):
    for cs in A.cases(size):
        for call in cs.calls:
            lens = cs.lens(call)
            want = [A.oracle_pair(cs.seqs, x, y, cs.mega if call.mega else None)["cand"] for x, y in call.pairs]
            assert A.predict(lens, call.env, want) == call.path, (size, cs.name, call.what)
            if call.refused:
                assert not A.post_rows_ok(lens, call.env), (size, cs.name, call.what)


@pytest.mark.parametrize("size", ["gpu", "emu"])
def test_overflow_cases_exceed_the_room(size):
    """the short path's room and the general stage's first room: max(MPCGPU_CAND_PER_ROW * longest sequence, 1024)"""
    for name in ("overflow_short", "overflow_general"):
        cs = A.case(size, name)
        for call in cs.calls:
            lens = cs.lens(call)
            cand = [A.oracle_pair(cs.seqs, x, y)["cand"] for x, y in call.pairs]
            assert max(cand) > A.capc_of(lens, call.env), (size, name, call.what, cand, A.capc_of(lens, call.env))
            assert A.regrowths(lens, cand, call.env) >= 1
    if size == "gpu":  # the issue's measurement: "A"*638 x "A"*511 has 20 866 candidates against 7 656 places
        cs = A.case("gpu", "overflow_short")
        assert A.oracle_pair(cs.seqs, 0, 1)["cand"] == 20866 and A.capc_of(cs.lens(cs.calls[0]), {}) == 7656


def test_gpu_table_oracle_budget():
    total = sum(cs.cells() for cs in A.cases("gpu"))
    assert total <= A.MAX_GPU_CELLS, total
