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
@pytest.mark.parametrize("form", ["windows", "walk"])
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
