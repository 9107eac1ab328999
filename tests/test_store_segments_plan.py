"""The host-only planner of a record store's segments (include/mpcgpu.h: mpcgpu_plan_store_segments — the function the store build
calls) at the size the feature exists for, without a device: 3000 sequences, nine million record sizes that sum to more than 2^32
blocks, at the default limit; and the small cases by hand."""
import numpy as np
import pytest

from muscle_amd._lib import MpcGpuError, plan_store_segments

LIMIT = 2 ** 32 - 1  # blocks: a record's start and a slab's end are 32-bit block indices inside their segment


def _check(n, sizes, limit, zf, bl):
    """the segments tile all Z in order, hold what their slabs hold, and stay within the limit"""
    assert zf[0] == 0 and zf[-1] == n and all(a < b for a, b in zip(zf, zf[1:])) and len(bl) == len(zf) - 1
    slab = np.asarray(sizes, np.uint64).reshape(n, n).sum(axis=1)
    for g, (a, b) in enumerate(zip(zf, zf[1:])):
        assert bl[g] == int(slab[a:b].sum()) and bl[g] <= limit, g
    assert sum(bl) == int(slab.sum())


def test_real_size_at_the_default_limit():
    """n = 3000, mean record 8149 B (1000 x L~400) = 509 blocks: 73 GB, more than 2^32 blocks"""
    n = 3000
    rng = np.random.default_rng(1)
    sizes = rng.integers(400, 619, size=n * n, dtype=np.uint32)  # mean 509 blocks
    total = int(sizes.astype(np.uint64).sum())
    assert total > 2 ** 32 and abs(total * 16 / (n * n) - 8149) < 16
    zf, bl = plan_store_segments(n, sizes)
    _check(n, sizes, LIMIT, zf, bl)
    assert len(bl) == 2 and all(b < 2 ** 32 for b in bl)  # the fewest: the first segment takes slabs while they fit
    assert bl[0] + int(sizes.reshape(n, n)[zf[1]].astype(np.uint64).sum()) > LIMIT
    assert plan_store_segments(n, sizes, LIMIT) == (zf, bl)  # 0 means the default
    assert plan_store_segments(n, sizes, 2 ** 40) == (zf, bl)  # a limit above the layout's is clamped to it


def test_hand_cases():
    sizes = np.array([1, 2, 3,  4, 5, 6,  7, 8, 9], np.uint32)  # slabs 6, 15, 24
    assert plan_store_segments(3, sizes, 24) == ([0, 2, 3], [21, 24])
    assert plan_store_segments(3, sizes, 38) == ([0, 2, 3], [21, 24])   # 6 + 15 + 24 = 45 does not fit, 21 does
    assert plan_store_segments(3, sizes, 45) == ([0, 3], [45])
    assert plan_store_segments(3, np.array([8] * 9, np.uint32), 24) == ([0, 1, 2, 3], [24, 24, 24])  # one Z per segment
    assert plan_store_segments(3, np.array([8] * 9, np.uint32), 47) == ([0, 1, 2, 3], [24, 24, 24])
    assert plan_store_segments(3, np.array([8] * 9, np.uint32), 48) == ([0, 2, 3], [48, 24])


def test_limit_below_one_slab_is_an_error():
    sizes = np.array([1, 2, 3,  4, 5, 6,  7, 8, 9], np.uint32)
    with pytest.raises(MpcGpuError, match="slab"):
        plan_store_segments(3, sizes, 23)


def test_one_sequence_and_empty_records():
    assert plan_store_segments(1, np.array([5], np.uint32)) == ([0, 1], [5])
    assert plan_store_segments(1, np.array([5], np.uint32), 5) == ([0, 1], [5])
    assert plan_store_segments(2, np.zeros(4, np.uint32), 1) == ([0, 2], [0])  # a partial store's missing records: size 0


def test_more_segments_than_the_first_array_holds():
    n = 40
    zf, bl = plan_store_segments(n, np.ones(n * n, np.uint32), n)  # 40 segments: the binding asks again with room for them
    assert zf == list(range(n + 1)) and bl == [n] * n
