"""The drop-in's guide tree from bare sequences (hostcxx/mpcflat_gpu.cpp: CalcGuideTree_SW_BLOSUM62 over mpcgpu_sw_scores) — shared by
tests/test_dropin_sw_emu.py (the emulator build of the library) and tests/test_gpu_dropin_sw.py (the device). The golden Newick bytes
and MSA MD5s are the compiled reference's (tests/golden/sw_dropin.json, tests/golden/make_sw_golden.py) on X-terminated sets, where its
trace-back assert cannot fire. TEST INFRASTRUCTURE."""
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np

import _sw
from muscle_amd.synth import write_fasta


def golden():
    with open(_sw.DROPIN) as f:
        return json.load(f)


def _run(binary, args, seqs, files=None, env=None, outs=()):
    with tempfile.TemporaryDirectory() as d:
        write_fasta(os.path.join(d, "in.fa"), seqs)
        for fn, text in (files or {}).items():
            with open(os.path.join(d, fn), "w") as f:
                f.write(text)
        subprocess.run([binary] + args + ["-threads", "3", "-quiet"], check=True, timeout=600, cwd=d, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, env=dict(os.environ, **(env or {})))
        return [open(os.path.join(d, o), "rb").read() for o in outs]


def swdistmx(binary, seqs, env=None):
    return _run(binary, ["-swdistmx", "in.fa", "-guidetreeout", "t.nwk"], seqs, env=env, outs=["t.nwk"])[0].decode()


def super7(binary, seqs, extra, env=None, files=None, tree=False):
    outs = _run(binary, ["-super7", "in.fa", "-output", "out.afa"] + extra + (["-guidetreeout", "t.nwk"] if tree else []), seqs, files=files, env=env,
                outs=["out.afa"] + (["t.nwk"] if tree else []))
    return outs


def check_newick(binary, name, env=None):
    assert swdistmx(binary, _sw.dropin_seqs(name), env=env) == golden()[name]["newick"]


def check_super7(binary, name, env=None):
    data = super7(binary, _sw.dropin_seqs(name), _sw.DROPIN_SETS[name][3], env=env)[0]
    assert hashlib.md5(data).hexdigest() == golden()[name]["msa_md5"]


def reseek_distmx(seqs):
    """the matrix of swdistmx.cpp:75-80 from the restatement's scores, in the format -distmxin reads (upgma5.cpp:436-503). %.9g
    round-trips a float32 exactly, so UPGMA5 starts from the same floats either way."""
    n = len(seqs)
    out = ["distmx\t%d" % n] + ["%d\ts%d" % (i, i) for i in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            norm = np.float32(_sw.sw_ref(seqs[i], seqs[j])) / (np.float32(len(seqs[i]) + len(seqs[j])) / np.float32(2.0))
            out.append("%d\t%d\t%.9g" % (i, j, np.float32(norm)))
    return "\n".join(out) + "\n"


def check_unterminated(binary, name):
    """no X terminators: the reference may die in its trace-back here (sw.cpp:73-74); muscle_gpu completes, and the MSA is the one the
    same binary writes when the restatement's normalised scores come in through -distmxin"""
    seqs = _sw.dropin_seqs(name, terminated=False)
    extra = _sw.DROPIN_SETS[name][3]
    got = super7(binary, seqs, extra)[0]
    want = super7(binary, seqs, extra + ["-distmxin", "dm.tsv"], files={"dm.tsv": reseek_distmx(seqs)})[0]
    return got, want
