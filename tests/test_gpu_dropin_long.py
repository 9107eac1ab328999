"""`muscle_gpu -align` on four related sequences of about 4 200 positions: every stage of MPCFlat::Run on its long-sequence path,
the consistency relax on band tiles over the record store's long form (no gather-fallback NOTE). The final MSA equals the compiled
reference's byte for byte: its MD5 is committed in tests/golden/msa_long_md5.json (written by the reference's `muscle`, 12.5 s on 8
threads; the oracle's EA of the six pairs is 0.85 .. 0.87, not degenerate), and where the compiled reference travelled along it runs
again here."""
import json
import os

import pytest

import _msa

pytestmark = pytest.mark.gpu

NAME = "synth_4x4200_s3"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msa_long_md5.json")


def test_align_long_sequences_identical_to_reference():
    from muscle_amd.hostinfo import usable_cores
    assert os.path.exists(_msa.GPU_MUSCLE), "hostcxx/_build/muscle_gpu missing: run __graft_entry__.build()"
    seqs, _, _ = _msa.input_set(NAME)
    assert len(seqs) == 4 and min(len(s) for s in seqs) > 4095
    with open(GOLDEN) as f:
        golden = json.load(f)[NAME]
    th = usable_cores()
    md5_gpu, data_gpu = _msa.run_muscle(_msa.GPU_MUSCLE, NAME, threads=th)
    if os.path.exists(_msa.REF_MUSCLE):
        md5_ref, data_ref = _msa.run_muscle(_msa.REF_MUSCLE, NAME, threads=th)
        print("%s gpu=%s ref(live)=%s golden=%s" % (NAME, md5_gpu, md5_ref, golden))
        assert data_gpu == data_ref, "final MSA differs from the live reference's"
    assert md5_gpu == golden, "final MSA differs from the reference's committed MD5"
