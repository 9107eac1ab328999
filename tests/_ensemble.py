"""Ensemble (replicate) runs of a `muscle` binary: -stratified / -diversified make several MPCFlat::Runs in one process
(align.cpp:96-167), four tree permutations per perturbation seed, which the drop-in serves from ONE posterior stage per seed
(hostcxx/mpcflat_gpu.cpp: MPCFlat::CalcPosterior). The cases, how one is run, and what its outputs hash to.
TEST INFRASTRUCTURE."""
import hashlib
import json
import os
import re
import subprocess
import tempfile

import _mega
from _msa import GPU_MUSCLE, REF_MUSCLE, ROOT, make_family  # noqa: F401
from muscle_amd.synth import write_fasta

GOLDEN = os.path.join(ROOT, "tests", "golden", "ensemble_md5.json")


def _n8():
    return make_family(8, 60, seed=5)


def _dupes():
    # 7 sequences, two of them exact duplicates of others: Derep before the stage, InsertDupes after it (mpcflat.cpp:290-336)
    s = make_family(5, 50, seed=9)
    return [s[0], s[1], s[0], s[2], s[1], s[3], s[4]]


# name -> (input: list of sequences, or the text of a .mega file; options; output pattern; (computed, reused) posterior stages)
CASES = {
    "strat_n8_L60": (_n8, ["-stratified"], "out.efa", (4, 12)),
    "strat_n3_L30": (lambda: make_family(3, 30, seed=5), ["-stratified"], "out.efa", (4, 12)),  # the smallest run that still relaxes
    "strat_n2_L40": (lambda: make_family(2, 40, seed=5), ["-stratified"], "out.efa", (4, 12)),  # Consistency is skipped: host-matrix path
    "strat_dupes": (_dupes, ["-stratified"], "out.efa", (4, 12)),
    "strat_cons0": (_n8, ["-stratified", "-consiters", "0"], "out.efa", (4, 12)),  # no relax: host-matrix path
    "strat_cons1_refine3": (_n8, ["-stratified", "-consiters", "1", "-refineiters", "3"], "out.efa", (4, 12)),
    "strat_rep2": (_n8, ["-stratified", "-replicates", "2"], "out.efa", (2, 6)),  # 8 replicates, seeds 0 and 1
    "strat_files": (_n8, ["-stratified"], "out.@.afa", (4, 12)),  # a file per replicate
    "strat_mega": (lambda: _mega.mega_text("mega_bb11001"), ["-stratified"], "out.efa", (4, 12)),
    "divers_rep3": (_n8, ["-diversified", "-replicates", "3"], "out.efa", (3, 0)),  # three seeds, three different tables: nothing to reuse
}

STAGE_LINE = re.compile(r"^\[muscle_gpu\] posterior stage: computed (\d+) reused (\d+)$", re.M)


def run_case(binary, name, threads=4, timeout=300, env=None):
    """-> ({output file name: bytes}, stderr text). MUSCLE_GPU_TIMING=1 in env makes the drop-in report on stderr."""
    make_input, options, pattern, _ = CASES[name]
    inp = make_input()
    with tempfile.TemporaryDirectory() as d:
        if isinstance(inp, str):
            fa = "in.mega"
            with open(os.path.join(d, fa), "w") as f:
                f.write(inp)
        else:
            fa = "in.fa"
            write_fasta(os.path.join(d, fa), inp, None)
        r = subprocess.run([binary, "-align", fa, "-output", pattern, "-threads", str(threads), "-quiet"] + options, check=True,
                           timeout=timeout, cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})))
        outs = {}
        for fn in sorted(os.listdir(d)):
            if fn.startswith("out."):
                with open(os.path.join(d, fn), "rb") as f:
                    outs[fn] = f.read()
    return outs, r.stderr.decode(errors="replace")


def md5s(outs):
    return {fn: hashlib.md5(data).hexdigest() for fn, data in outs.items()}


def stage_counts(stderr_text):
    """(computed, reused) of the drop-in's end-of-run report, or None when the line is not there"""
    m = STAGE_LINE.findall(stderr_text)
    assert len(m) <= 1, stderr_text
    return (int(m[0][0]), int(m[0][1])) if m else None


def golden():
    with open(GOLDEN) as f:
        return json.load(f)
