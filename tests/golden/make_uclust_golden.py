#!/usr/bin/env python3
"""Generates tests/golden/uclust_dropin.json from the COMPILED REFERENCE, on the CPU: for each set of tests/_uclust_dropin.py SETS and SETS_EMU

  super5_md5     MD5 of the MSA `oracle/_ref/muscle -super5 in.fa -output out -threads 1` writes
  uclust_exit0   whether `oracle/_ref/muscle -uclust in.fa -output c.fa -minea 0.9 -threads 1` exits 0
  uclust_md5     MD5 of the centroid file that command writes (null where it does not exit 0)
  n, min_len, max_len   the set, for the record

What it found (reference rcedgar/muscle 5.3 as built by oracle/build_ref.sh): -super5 exits 0 on all six sets, and -uclust exits 0 on
all six sets too; both are run twice and must write the same bytes both times (the fixture is only worth committing if the reference
itself is deterministic on these inputs with one thread). Run where oracle/build_ref.sh has built the reference; the output is committed."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import _uclust_dropin as U  # noqa: E402
from muscle_amd.synth import write_fasta  # noqa: E402

REF_MUSCLE = os.path.join(ROOT, "oracle", "_ref", "muscle")


def ref_run(seqs, args):
    """-> (exit status, MD5 of `out` or None)"""
    with tempfile.TemporaryDirectory() as d:
        write_fasta(os.path.join(d, "in.fa"), seqs)
        r = subprocess.run([REF_MUSCLE] + args, cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=3600)
        out = os.path.join(d, "out")
        if r.returncode != 0 or not os.path.exists(out):
            return r.returncode, None
        with open(out, "rb") as f:
            return 0, hashlib.md5(f.read()).hexdigest()


def main():
    fx = {}
    for name in U.SETS + U.SETS_EMU:
        seqs = U.input_set(name)
        s5 = [ref_run(seqs, ["-super5", "in.fa", "-output", "out", "-threads", "1", "-quiet"]) for _ in range(2)]
        assert s5[0][0] == 0 and s5[0] == s5[1], (name, s5)
        uc = [ref_run(seqs, ["-uclust", "in.fa", "-output", "out", "-minea", "0.9", "-threads", "1", "-quiet"]) for _ in range(2)]
        assert uc[0] == uc[1], (name, uc)
        fx[name] = {"n": len(seqs), "min_len": min(map(len, seqs)), "max_len": max(map(len, seqs)), "super5_md5": s5[0][1],
                    "uclust_exit0": uc[0][0] == 0, "uclust_md5": uc[0][1]}
        print(name, fx[name], flush=True)
    with open(U.FIXTURE, "w") as f:
        json.dump(fx, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
