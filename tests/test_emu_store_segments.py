"""A record store in segments through the SIMT emulator, which compiles the product's kernel sources (tests/_store_segments.py): case 1
of tests/test_gpu_store_segments.py — a segment boundary after every Z slab, three to four slabs per segment, both merge forms —
against the oracle and the unsegmented run, plus the emulator's race finders on the segmented staging."""
import os
import subprocess

import pytest

import _store_segments as S

EMU_DIR = os.path.join(S.HERE, "emu")
EMU_LIB = os.path.join(EMU_DIR, "libmpcgpu_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.fixture(scope="module")
def ref():
    return S.Ref()


@pytest.fixture(scope="module")
def plain(emu, ref, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("plain")
    return {form: S.child("stages", dict(env), emu, tmp) for form, env in S.FORMS.items()}


@pytest.mark.parametrize("cut", ["every", "few"])
@pytest.mark.parametrize("form", ["windows", "walk", "long"])
def test_emu_every_boundary(emu, ref, plain, tmp_path, form, cut):
    limit = (ref.limits if form == "windows" else ref.limits_walk)[cut]
    if cut == "every":
        assert ref.expect(limit, form == "windows")[1 if form == "windows" else 0] == ref.n
    env = dict(S.FORMS[form])
    env[S.HOOK] = str(limit)
    got = S.child("stages", env, emu, tmp_path)
    S.check_stages(ref, got, plain[form], form, limit, "%s, %s" % (form, cut))


@pytest.mark.parametrize("finder", [{"EMU_SCHED": "random"}, {"EMU_DMA": "late"}])
def test_emu_segmented_staging_races(emu, ref, plain, tmp_path, finder):
    """threads in random order between synchronisation points / transfers that land at the issuing thread's wait: the per-step base
    address is read where the transfers are issued, in every wave"""
    limit = ref.limits["every"]
    env = dict(S.FORMS["windows"])
    env.update(finder)
    env[S.HOOK] = str(limit)
    got = S.child("stages", env, emu, tmp_path)
    S.check_stages(ref, got, plain["windows"], "windows", limit, str(finder))


def test_emu_whole_record_tiles_are_refused_by_name(emu, ref, tmp_path):
    got = S.child("pairs", {S.HOOK: str(ref.limits["every"]), "MPCGPU_RELAX_TILES": "pairs"}, emu, tmp_path)
    assert got["error"] and "MPCGPU_RELAX_TILES=pairs" in got["error"] and "segments" in got["error"], got["error"]


@pytest.mark.parametrize("seg", [False, True], ids=["plain", "segments"])
def test_emu_long_partial_stores(emu, ref, tmp_path, seg):
    """partial stores of the long form of the block records (MPCGPU_RELAX_LONG=1), one plain and one in segments: tests/_pair_order.py's
    exchange between two contexts; band-long on both after every import"""
    env = dict(S.FORMS["long"])
    if seg:
        env[S.HOOK] = str(ref.limits_walk["every"])
    got = S.child("partial", env, emu, tmp_path)
    assert len(got["infos"]) == 2
    for info, fallback in got["infos"]:
        assert "band-long" in info and (S.seg_counts(info)[0] > 1) == seg and fallback == 0, info


def test_emu_long_joins_and_lifetime_in_segments(emu, ref, tmp_path):
    """joins (rows and sort, plain and weighted) over a long store in segments equal those over the unsegmented one; release and regrowth"""
    env = dict(S.FORMS["long"])
    one = S.child("joins", env, emu, tmp_path)
    env[S.HOOK] = str(ref.limits_walk["every"])
    seg = S.child("joins", env, emu, tmp_path)
    assert "band-long" in one["info"] and "band-long" in seg["info"] and S.seg_counts(seg["info"])[0] == ref.n and seg["fallback"] == 0, seg["info"]
    S.same_joins(one, seg)
    S.check_lifetime(ref, S.child("lifetime", env, emu, tmp_path), "long")
