#!/usr/bin/env python3
"""Generates the fixtures of the Smith-Waterman guide-tree tests (tests/_sw.py) from the COMPILED REFERENCE, on the CPU:

  tests/golden/sw_scores.npz   the bits SWFast_Seqs_BLOSUM62 (sw.cpp:287-295) returns for all pairs of tests/_sw.py golden_input(),
                               with the tables the reference scores with (g_CharToLetterAmino, Blosum62_sij) and Open / Ext of
                               swdistmx.cpp:106-107. A small probe (its text below, ours) is compiled against the reference headers
                               and oracle/_ref/libmuscle_ref.so (every reference object but main.o) and calls the function itself.
  tests/golden/sw_dropin.json  per set of tests/_sw.py DROPIN_SETS: the Newick bytes `oracle/_ref/muscle -swdistmx in.fa
                               -guidetreeout t` writes and the MD5 of the MSA `oracle/_ref/muscle -super7 in.fa` writes with no tree
                               option.

Every input sequence ends in X: a wildcard scores 0, so a cell of the last row or column can equal but never exceed the running
best, and the reference's trace-back assert (sw.cpp:73-74) cannot fire. The runs below are that claim's check: the probe and both
commands must exit 0. Run where oracle/build_ref.sh has built the reference; the outputs are committed."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import _sw  # noqa: E402
from muscle_amd.synth import write_fasta  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
SRC = os.environ.get("MUSCLE_REF_SRC", "/root/reference/src")

PROBE = r"""
#include "muscle.h"
#include "xdpmem.h"
float SWFast_Seqs_BLOSUM62(XDPMem &Mem, const Sequence &A, const Sequence &B, float Open, float Ext, uint &Loi, uint &Loj,
  uint &Leni, uint &Lenj, string &Path); // sw.cpp:287
extern float Blosum62_sij[20][20]; // blosum.cpp:8
int main(int argc, char **argv)
	{
	MultiSequence Input;
	Input.FromFASTA(argv[1], true);
	const float Open = -11, Ext = -1; // swdistmx.cpp:106-107
	FILE *f = fopen(argv[2], "wb");
	fwrite(g_CharToLetterAmino, 1, 256, f);
	fwrite(Blosum62_sij, sizeof(float), 400, f);
	fwrite(&Open, sizeof(float), 1, f);
	fwrite(&Ext, sizeof(float), 1, f);
	XDPMem Mem;
	const uint N = Input.GetSeqCount();
	for (uint i = 0; i < N; ++i)
		for (uint j = i + 1; j < N; ++j)
			{
			string Path;
			uint Loi, Loj, Leni, Lenj;
			float Score = SWFast_Seqs_BLOSUM62(Mem, *Input.GetSequence(i), *Input.GetSequence(j), Open, Ext, Loi, Loj, Leni, Lenj, Path);
			fwrite(&Score, sizeof(float), 1, f);
			}
	fclose(f);
	return 0;
	}
"""


def scores():
    seqs = _sw.golden_input()
    assert all(s.endswith("X") and 2 <= len(s) <= 300 for s in seqs)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "probe.cpp"), "w") as f:
            f.write(PROBE)
        exe = os.path.join(d, "probe")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fopenmp", "-pthread", "-w", "-I" + os.path.join(REF, "inc"), "-I" + SRC,
                               os.path.join(d, "probe.cpp"), "-L" + REF, "-lmuscle_ref", "-Wl,-rpath," + REF, "-o", exe])
        write_fasta(os.path.join(d, "in.fa"), seqs)
        subprocess.check_call([exe, os.path.join(d, "in.fa"), os.path.join(d, "out.bin")], stdout=subprocess.DEVNULL)
        raw = open(os.path.join(d, "out.bin"), "rb").read()
    n = len(seqs)
    loc = np.frombuffer(raw[:256], np.uint8)
    sub = np.frombuffer(raw[256:256 + 1600], np.float32).reshape(20, 20)
    op, ex = np.frombuffer(raw[1856:1864], np.float32)
    sc = np.frombuffer(raw[1864:], np.float32)
    assert len(sc) == n * (n - 1) // 2
    np.savez_compressed(_sw.SCORES, seqs=np.array(seqs), scores=sc, letter_of_char=loc, blosum62=sub, open=op, ext=ex)
    print("sw_scores.npz: %d sequences, %d pairs, %d zero scores" % (n, len(sc), int((sc == 0).sum())))


def dropin():
    out = {}
    muscle = os.path.join(REF, "muscle")
    for name, (_, _, _, extra) in _sw.DROPIN_SETS.items():
        with tempfile.TemporaryDirectory() as d:
            write_fasta(os.path.join(d, "in.fa"), _sw.dropin_seqs(name))
            subprocess.check_call([muscle, "-swdistmx", "in.fa", "-guidetreeout", "t.nwk", "-threads", "4", "-quiet"], cwd=d,
                                  stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            subprocess.check_call([muscle, "-super7", "in.fa", "-output", "out.afa", "-threads", "4", "-quiet"] + extra, cwd=d,
                                  stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            out[name] = {"newick": open(os.path.join(d, "t.nwk")).read(),
                         "msa_md5": hashlib.md5(open(os.path.join(d, "out.afa"), "rb").read()).hexdigest()}
        print(name, out[name]["msa_md5"])
    with open(_sw.DROPIN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    scores()
    dropin()
