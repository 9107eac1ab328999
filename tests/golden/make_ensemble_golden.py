#!/usr/bin/env python3
"""Generates tests/golden/ensemble_md5.json: MD5 of every output file the compiled reference (oracle/_ref/muscle, built by
oracle/build_ref.sh where the reference sources are) writes for each ensemble case of tests/_ensemble.py, on the CPU.
Every case is run at two thread counts; a case whose bytes differ between them has no one golden answer and is dropped
(said on stdout; none is today: -align sums nothing in thread-arrival order). The JSON is committed."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _ensemble as E  # noqa: E402

THREADS = (1, 4)
out = {}
for name in E.CASES:
    runs = [E.md5s(E.run_case(E.REF_MUSCLE, name, threads=t, timeout=3600)[0]) for t in THREADS]
    if runs[0] != runs[1]:
        print("%s: DROPPED, the reference's bytes differ between %d and %d threads" % (name, THREADS[0], THREADS[1]))
        continue
    out[name] = runs[0]
    print(name, json.dumps(runs[0], sort_keys=True))
with open(E.GOLDEN, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
