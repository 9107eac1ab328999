"""`muscle_gpu -super5` on the device with consensus sequences of more than 12 115 positions: CalcEADistMx's one mpcgpu_ea_scores call
(hostcxx/mpcflat_gpu.cpp, which sets MPCGPU_EA_WIDE=1) finishes the pair in post_wide_ea_kernel where the library used to refuse the
list and the run died. The MSA is the reference's (tests/golden/ea_wide_md5.json: the MD5 of the unmodified reference's output for
the same seeded input) and the one MUSCLE_GPU_EA_DISTMX=0 gives by the old route. The input (tests/_ea_wide.py: dropin_input) cannot
form the two clusters one would like: the reference's EA of two near-identical sequences is 0.985 at 5 000 positions, 0.443 at 8 000 (the
CPU oracle) and lower still at 12 200, under UCLUST's thresholds, so all six pairs of four consensus sequences reach CalcEADistMx. Each
12 200 x 12 200 alignment takes about 2.7 s on the device and -super5 makes some 25 of them, so this one test takes minutes, not seconds:
the length is what the test is about."""
import hashlib
import json
import os
import subprocess
import tempfile
import time

import pytest

import _ea_dropin as D
import _ea_wide as W
import _msa
from muscle_amd.synth import write_fasta

pytestmark = pytest.mark.gpu


def super5(binary, seqs, env):
    with tempfile.TemporaryDirectory() as d:
        write_fasta(os.path.join(d, "in.fa"), seqs)
        t0 = time.perf_counter()
        r = subprocess.run([binary, "-super5", "in.fa", "-output", "out.afa", "-threads", "1", "-quiet"], check=True, timeout=600, cwd=d,
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=dict(os.environ, MUSCLE_GPU_TIMING="1", **env))
        wall = time.perf_counter() - t0
        with open(os.path.join(d, "out.afa"), "rb") as f:
            md5 = hashlib.md5(f.read()).hexdigest()
        print("muscle_gpu -super5 %s, %s: wall %.1f s, MD5 %s" % (W.DROPIN_NAME, env, wall, md5), flush=True)
        return md5, r.stderr.decode(errors="replace")


def test_super5_long_consensus_sequences():
    if not os.path.exists(_msa.GPU_MUSCLE):
        pytest.fail("hostcxx/_build/muscle_gpu missing: run __graft_entry__.build() where the reference sources are, "
                    "or where oracle/_ref/muscle_gpu built there travelled along")
    seqs = W.dropin_input()
    assert len(seqs) == 4 and min(len(s) for s in seqs) >= W.wide_min_default()
    with open(W.DROPIN_GOLDEN) as f:
        want = json.load(f)[W.DROPIN_NAME]
    md5, err = super5(_msa.GPU_MUSCLE, seqs, {"MPCGPU_TRACE": "1"})
    assert md5 == want and D.ea_calls(err) == 1, (md5, want, err[-2000:])
    pairs = W.DROPIN_CLUSTERS * (W.DROPIN_CLUSTERS - 1) // 2
    assert "[mpcgpu] post wide ea: %d pairs" % pairs in err and "[mpcgpu] post ea:" not in err, err[-2000:]  # every pair of consensus sequences went wide
    md5, err = super5(_msa.GPU_MUSCLE, seqs, {"MUSCLE_GPU_EA_DISTMX": "0"})
    assert md5 == want and D.ea_calls(err) == 0, (md5, want, err[-2000:])
