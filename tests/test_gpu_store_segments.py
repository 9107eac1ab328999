"""A record store in segments on MI355X (tests/_store_segments.py): MPCGPU_STORE_SEG_BLOCKS splits the store of 13 short sequences
into as many as 13 allocations, and the library runs on it what it runs on a store beyond 2^32 blocks — build, band-tile relax in both
merge forms and on the long form of the block records, commit, joins, partial stores, release and regrowth. Every case in a fresh child process (the hook is read from the
environment); the oracle and the record sizes the expected segments are planned from are computed once."""
import pytest

import _store_segments as S

pytestmark = pytest.mark.gpu
LIB = None  # the HIP library


@pytest.fixture(scope="module")
def ref():
    return S.Ref()


@pytest.fixture(scope="module")
def plain(ref, tmp_path_factory):
    """the runs without the hook, one per merge form"""
    tmp = tmp_path_factory.mktemp("plain")
    return {form: S.child("stages", dict(env), LIB, tmp) for form, env in S.FORMS.items()}


@pytest.mark.parametrize("cut", ["every", "few"])
@pytest.mark.parametrize("form", ["windows", "walk", "long"])
def test_every_boundary(ref, plain, tmp_path, form, cut):
    """case 1: a segment boundary after every Z slab (of the window records in the windows form, of the block records in the walk
    form: the limit is the largest slab of what the form stages), and three to four slabs per segment; EA and the matrices of stage 0
    and of both iterations equal the oracle's and the unsegmented run's bit for bit, on band tiles, in the planned segments"""
    limit = (ref.limits if form == "windows" else ref.limits_walk)[cut]
    if cut == "every":  # the family is ordered so that the smallest limit cuts after every slab
        assert ref.expect(limit, form == "windows")[1 if form == "windows" else 0] == ref.n
    else:
        zf = ref.plan(ref.blocks, limit)[0]
        assert all(3 <= b - a <= 4 for a, b in zip(zf[:-1], zf[1:-1])) and 1 <= zf[-1] - zf[-2] <= 4, zf  # (the last one: what is left)
    env = dict(S.FORMS[form])
    env[S.HOOK] = str(limit)
    got = S.child("stages", env, LIB, tmp_path)
    S.check_stages(ref, got, plain[form], form, limit, "%s, %s" % (form, cut))


def every(ref, form):
    """the limit that cuts after every Z slab of what the form stages"""
    return (ref.limits if form == "windows" else ref.limits_walk)["every"]


@pytest.mark.parametrize("form", ["windows", "long"])
def test_joins_on_a_segmented_store(ref, tmp_path, form):
    """case 2: BuildPost by rows and by sort, plain and weighted, and the weighted AlignAlns after two committed iterations: the commit
    wrote segmented block and window records, the row form reads them — bit-identical to the unsegmented run. long: the row reader of
    the long records (build_post_rows_long_kernel) through the per-Z bases; bit-identical to the short store's joins as well"""
    env = dict(S.FORMS[form])
    one = S.child("joins", env, LIB, tmp_path)
    env[S.HOOK] = str(every(ref, form))
    seg = S.child("joins", env, LIB, tmp_path)
    assert S.seg_counts(one["info"]) == (1, 1)
    assert S.seg_counts(seg["info"]) == ref.expect(every(ref, form), form == "windows") and seg["fallback"] == 0, seg["info"]
    S.same_joins(one, seg)
    if form == "long":
        short = S.child("joins", dict(S.FORMS["windows"]), LIB, tmp_path)
        assert "band-long" in one["info"] and "band-long" not in short["info"], (one["info"], short["info"])
        assert "band-long" in seg["info"] and S.MERGE["long"] in seg["info"] and S.seg_counts(seg["info"])[0] == ref.n, seg["info"]
        S.same_joins(short, seg)


@pytest.mark.parametrize("form,seg", [("windows", True), ("long", False), ("long", True)], ids=["windows", "long-plain", "long"])
def test_partial_stores_in_segments(ref, tmp_path, form, seg):
    """case 3: two contexts on the one device under the block partition of two ranks, partial stores in segments: every stage of both
    ranks equals the oracle, again after mpcgpu_store_complete, then a join in both forms (tests/_pair_order.py). long, as one plain
    store and in segments: mpcgpu_store_import_part builds the long records of the needed sequences only (need[] in
    var_build_long_kernel), the commits of the own and the foreign slice (own0 / own1, lazy_packed, nx / ny in
    commit_pairs_long_kernel); band-long on both contexts after every import"""
    env = dict(S.FORMS[form])
    if seg:
        env[S.HOOK] = str(every(ref, form))
    got = S.child("partial", env, LIB, tmp_path)
    assert len(got["infos"]) == 2
    for info, fallback in got["infos"]:
        assert (S.seg_counts(info)[0] > 1) == seg and fallback == 0, info
        assert ("band-long" in info) == (form == "long"), info


def test_whole_record_tiles_are_refused_by_name(ref, tmp_path):
    """case 4: relax_var_kernel does not read a store in segments; asking for it is an error that says so"""
    got = S.child("pairs", {S.HOOK: str(ref.limits["every"]), "MPCGPU_RELAX_TILES": "pairs"}, LIB, tmp_path)
    assert got["error"] and "MPCGPU_RELAX_TILES=pairs" in got["error"] and "segments" in got["error"], got["error"]


@pytest.mark.parametrize("form", ["windows", "long"])
def test_release_and_regrowth(ref, tmp_path, form):
    """case 5: mpcgpu_set_seqs with 7 of the sequences on a context that holds a store in segments, then all 13 again"""
    env = dict(S.FORMS[form])
    env[S.HOOK] = str(every(ref, form))
    S.check_lifetime(ref, S.child("lifetime", env, LIB, tmp_path), form)
