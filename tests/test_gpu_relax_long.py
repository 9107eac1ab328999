"""The long form of the record store and of relax_band_kernel on MI355X (kernels_store.h, MpcRbLongCxx in kernels_relaxb.h): stores
with a sequence above 4095 positions or a record above 4095 blocks stay on band tiles. Everything through the C ABI against the CPU
oracle, bit for bit: EA, the store after the build and after each of two iterations (mpcgpu_get_sparse_range). tests/_relax_long.py
holds the inputs and what they are claimed to be."""
import functools

import pytest

import _relax as R
import _relax_long as L
from muscle_amd.synth import make_family

pytestmark = pytest.mark.gpu

GATHER = ("CSR slabs", "kernel=relax_kernel")


@pytest.mark.parametrize("n", [3, 5, 9])
def test_relax_long_forced(n):
    """MPCGPU_RELAX_LONG=1 at small shapes (ragged lengths 1, 5 .. 120, a pair with a row that stores no cell): values and EA equal
    the oracle's, relax_info names the long form with is_fallback == 0 (fails without the long form), and mpcgpu_build_post /
    mpcgpu_align_alns on a fixed bipartition equal the oracle's matrix, path and score through the row reader of the records"""
    seqs = L.forced_seqs(n)
    L.check_forced_claims(seqs)
    L.run(seqs, L.FORCE, has=L.LONG, lacks=("window records",) + GATHER, fallback=False, store=("band-long",))
    info, fb = L.check_join(seqs, L.FORCE)
    assert "band-long" in info and "MpcRbLongCxx" in info and not fb, info


@functools.lru_cache(None)
def threshold_seqs():
    """lengths 4096, 4200, 60, 35 of one family: the two long ones related over their whole length, the short ones to a stretch of them"""
    fam = make_family(2, 4200, seed=91)
    a, b = (fam[0] * 2)[:4096], (fam[1] * 2)[:4200]
    return (a, b, a[2000:2060], b[3000:3035])


def test_relax_long_threshold():
    """no knob: one sequence past MPC_RV_MAXLEN takes the whole store to the long form (the parent reports the CSR slabs and
    is_fallback == 1 here), values equal the oracle's"""
    seqs = threshold_seqs()
    assert sorted(len(s) for s in seqs) == [35, 60, 4096, 4200]
    assert sum(len(v) // 2 for _, v in R.oracle(seqs)[0][0]) > 4096  # rows store cells
    L.run(seqs, {}, has=L.LONG, lacks=GATHER, fallback=False, store=("band-long",))


def test_relax_long_off_keeps_gather():
    """MPCGPU_RELAX_LONG=0 on the same input: the gather layout, as before the long form existed; values equal the oracle's"""
    L.run(threshold_seqs(), {"MPCGPU_RELAX_LONG": "0"}, has=GATHER, lacks=("band-long", "relax_band_kernel"), fallback=True, store=("CSR slabs",))


def test_relax_short_store_unchanged():
    """lengths 4095, 4095, 50 with at most two stored cells per row and column (identical sequences: the posterior is the diagonal), so
    every record has exactly len blocks <= 4095: today's band layout, named as before"""
    s = make_family(1, 4095, seed=93)[0]
    s = (s * 2)[:4095]
    seqs = (s, s, s[2000:2050])
    assert [len(x) for x in seqs] == [4095, 4095, 50] and L.record_blocks(seqs) <= 4095, L.record_blocks(seqs)
    L.run(seqs, {}, has=("relax_band_kernel",), lacks=("band-long", "MpcRbLong") + GATHER, fallback=False, store=("band index",), store_not=("band-long",))


def test_relax_long_record_trigger():
    """the record-size trigger without a long sequence: two related sequences of 4050 positions (rows of three and more cells put the
    record of the pair past 4095 blocks; asserted from the oracle's matrices) and a short one: the long form by itself"""
    fam = make_family(2, 4050, seed=95)
    seqs = ((fam[0] * 2)[:4050], (fam[1] * 2)[:4050], fam[0][100:140])
    assert max(len(s) for s in seqs) <= 4095 and L.record_blocks(seqs) > 4095, L.record_blocks(seqs)
    L.run(seqs, {}, has=L.LONG, lacks=GATHER, fallback=False, store=("band-long",))
