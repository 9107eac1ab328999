"""Ensembles on the GPU box: `muscle_gpu -align ... -stratified` (align.cpp:96-167: four tree permutations per perturbation
seed, every replicate an MPCFlat::Run on the same MPCFlat and the same input) writes the reference's bytes while computing the
posterior stage ONCE per seed — the other three replicates of a seed find the stage and its relax iterations in the device store
(hostcxx/mpcflat_gpu.cpp: MPCFlat::CalcPosterior, WhyNotReusable). The cases are tests/_ensemble.py's, the MD5s the compiled
reference's (tests/golden/make_ensemble_golden.py); where the compiled reference travelled along, a live run of it is the
primary check."""
import os

import pytest

import _ensemble as E

pytestmark = pytest.mark.gpu

_runs = {}


@pytest.fixture(scope="module")
def gpu_muscle():
    if not os.path.exists(E.GPU_MUSCLE):
        pytest.fail("hostcxx/_build/muscle_gpu missing: run __graft_entry__.build() where the reference sources are, "
                    "or where oracle/_ref/muscle_gpu built there travelled along")
    return E.GPU_MUSCLE


def threads():
    from muscle_amd.hostinfo import usable_cores
    return usable_cores()


def run_once(binary, name):
    """one run per case, with the drop-in's report on: its output files and its stderr serve both tests below"""
    if name not in _runs:
        _runs[name] = E.run_case(binary, name, threads=threads(), env={"MUSCLE_GPU_TIMING": "1"})
    return _runs[name]


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_ensemble_output_identical_to_reference(gpu_muscle, name):
    """every output file, byte for byte: against the live reference where it is here (a host whose libm moves both is reported,
    as in test_final_msa_identical_to_reference), and against the committed MD5s"""
    outs, _ = run_once(gpu_muscle, name)
    got, golden = E.md5s(outs), E.golden()[name]
    if os.path.exists(E.REF_MUSCLE):
        ref, _ = E.run_case(E.REF_MUSCLE, name, threads=threads())
        print("%s gpu=%s ref(live)=%s golden=%s" % (name, got, E.md5s(ref), golden))
        assert sorted(outs) == sorted(ref)
        for fn in ref:
            assert outs[fn] == ref[fn], "%s of %s differs from the live reference's" % (fn, name)
        if E.md5s(ref) != golden:
            pytest.xfail("the unmodified reference itself writes other bytes on this host than in the build container; "
                         "muscle_gpu follows the live reference")
    assert got == golden


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_posterior_stage_computed_once_per_seed(gpu_muscle, name):
    """MUSCLE_GPU_TIMING's `posterior stage: computed c reused r`: one computed stage per distinct set of tables, every other
    replicate reused"""
    _, err = run_once(gpu_muscle, name)
    print(err[-3000:])
    assert E.stage_counts(err) is not None, "no `posterior stage:` line in the report: this muscle_gpu was not linked from this tree's hostcxx/mpcflat_gpu.cpp"
    assert E.stage_counts(err) == E.CASES[name][3]


def test_reuse_switched_off(gpu_muscle):
    """MUSCLE_GPU_ENSEMBLE_REUSE=0: every replicate computes its stage, as before; the same bytes"""
    name = "strat_n8_L60"
    outs, err = E.run_case(gpu_muscle, name, threads=threads(), env={"MUSCLE_GPU_TIMING": "1", "MUSCLE_GPU_ENSEMBLE_REUSE": "0"})
    assert E.stage_counts(err) == (16, 0)
    assert outs == run_once(gpu_muscle, name)[0]
    assert E.md5s(outs) == E.golden()[name]


@pytest.mark.parametrize("name", ["strat_n8_L60", "strat_mega"])
def test_ensemble_sharded_over_contexts(gpu_muscle, name):
    """MUSCLE_GPU_DEVICES=0,0: the slot is a group of two contexts on the one device; the reuse looks at the epoch of both"""
    outs, err = E.run_case(gpu_muscle, name, threads=threads(), env={"MUSCLE_GPU_TIMING": "1", "MUSCLE_GPU_DEVICES": "0,0"})
    assert E.stage_counts(err) == (4, 12)
    assert outs == run_once(gpu_muscle, name)[0]
    assert E.md5s(outs) == E.golden()[name]
