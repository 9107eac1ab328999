"""fb_coop_kernel on the device: the W waves of a workgroup sweep the row blocks of one pair (muscle_amd/csrc/kernels_fbcoop.h).
Every case runs MPCGPU_FB_COOP=0 and a forced W on one context and holds both to the oracle bit for bit, to each other, to
stage_a_coop_info() and to the same family-0 launch count (tests/_fb_coop.py). Block edges come from short sequences under
MPCGPU_FB_LONG_MIN=65 MPCGPU_FB_LONG_H=1 (blocks of 64 rows); the real register shapes (7 and 4 rows per lane) from the shortest
row sequences that give them two and three blocks."""
import pytest

import _align_pairs as A
import _fb_coop as F
import _golden as G
import _parity as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("W", [2, 3, 4])
def test_coop_rows(W):
    """LX = 65: two blocks (waves idle under W = 3, 4); 64 W: one block per wave; 64 W + 1: one wave wraps to a one-row block;
    64 * 2 W + 37: two rounds and a tail. 100 columns: two macro-steps per block"""
    for k, LX in enumerate([65, 64 * W, 64 * W + 1, 64 * 2 * W + 37]):
        seqs, pairs = F.pair_of(LX, 100, 400 + k)
        F.check_list(seqs, pairs, W)


@pytest.mark.parametrize("W", [2, 3, 4])
def test_coop_columns(W):
    """each side of a macro-step edge (a block's forward sweep takes ceil((LY + 64) / 64) macro-steps, its backward sweep
    ceil((LY + 63) / 64)); LY = 1 and 63 with 6 blocks: every block is over before the two-macro-step lag has passed"""
    LX = 64 * 5 + 21
    seqs = A.related([LX, 1, 63, 64, 65, 127, 129, 200], 420)
    F.check_list(seqs, [(0, y) for y in range(1, 8)], W)


@pytest.mark.parametrize("LX,W", [(897, 2), (897, 3), (1345, 2), (1345, 3)])
def test_coop_seven_rows_per_lane(LX, W):
    """fb_coop_kernel<7, false>: 897 = 2 blocks + 1 row, 1345 = 3 blocks + 1 row; nothing forced but W"""
    seqs, pairs = F.pair_of(LX, 300, 430 + W)
    F.check_list(seqs, pairs, W, base_env={}, long_min=A.LONG_MIN)


@pytest.mark.parametrize("W", [2, 3, 4])
def test_coop_four_rows_per_lane(W):
    """fb_coop_kernel<4, false> (MPCGPU_FB_LONG_H=4): 1025 = 4 blocks + 1 row"""
    seqs, pairs = F.pair_of(1025, 260, 440)
    F.check_list(seqs, pairs, W, base_env={"MPCGPU_FB_LONG_H": "4"}, long_min=A.LONG_MIN)


def test_coop_w_is_clamped_to_the_resident_waves():
    """MPCGPU_FB_COOP=16 at 7 rows per lane: two waves per SIMD, 8 per CU — the library reports the W it used"""
    seqs, pairs = F.pair_of(897, 120, 445)
    F.check_list(seqs, pairs, 16, base_env={}, long_min=A.LONG_MIN, want_w=8)


@pytest.mark.parametrize("W", [2, 3, 4])
def test_coop_list(W):
    """three row-block pairs of 2, 3 and 5 blocks, two short pairs (single-wave kernels) and a pair given twice, as one list;
    then the short pairs alone: nothing runs cooperatively"""
    seqs = A.related([70, 150, 290, 40, 64, 90, 33], 450)
    pairs = [(0, 5), (3, 6), (2, 6), (1, 5), (4, 5), (0, 5)]
    F.check_list(seqs, pairs, W)
    assert F.check_list(seqs, [(3, 6), (4, 5)], W) == (0, 0)


@pytest.mark.parametrize("W", [2, 3, 4])
def test_coop_all_pairs_store_and_relax(W):
    """mpcgpu_calc_posteriors over 4 sequences (row-block pairs: those whose first sequence has 100 residues or more), then
    mpcgpu_build_store and one relax iteration on the store built from these candidate lists"""
    seqs = A.related([130, 70, 200, 9], 460)
    F.check_all_pairs(seqs, W, {"MPCGPU_FB_LONG_MIN": "100", "MPCGPU_FB_LONG_H": "1"}, nlong=4)


@pytest.mark.parametrize("W", [2, 3, 4])
def test_coop_mega(W):
    """structure profiles (fb_coop_kernel<1, true>): the bb11001.mega fixture against the reference's recorded stage A"""
    m = G.mega("mega_bb11001")
    (stages, ea), info, fam0 = F.all_pairs(m["seqs"], F.coop_env(F.FORCE_H1, W), mega=m, iters=0)
    off, info0, fam00 = F.all_pairs(m["seqs"], F.coop_env(F.FORCE_H1, 0), mega=m, iters=0)
    assert (P.bits(ea) == P.bits(m["ea"])).all()
    assert G.stage_digest(stages[0]) == m["digest"][0]
    P.assert_same((stages, ea), off, "cooperative against single-wave, mega")
    assert info == (6, W) and info0 == (0, 0) and fam0 == fam00, (info, info0, fam0, fam00)


def test_coop_no_memory_for_a_workgroup():
    """a forced W with MPCGPU_SCRATCH_GB=0 (1 GB for the planes) and a 20000 x 20000 pair (1.6 GB): an error message, no launch, and
    the context serves the next list"""
    F.check_no_memory()
