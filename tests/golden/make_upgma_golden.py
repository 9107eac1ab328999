"""Writes tests/golden/upgma_{plain,scaledist,eadist,reseek}.json from the compiled reference (oracle/_ref/muscle -upgma5): per file two
seeded matrices of 9 and 12 leaves — one of random values, one of 4 distinct values (ties, the neighbour redirect of upgma5.cpp:249-259,
stale row minima) — each as the text of the input file cmd_upgma5 reads (upgma5.cpp:386-502) and the Newick text it writes under every
-linkage. TEST INFRASTRUCTURE; run from the repository root after __graft_entry__.build():  python tests/golden/make_upgma_golden.py"""
import json
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MUSCLE = os.path.join(HERE, "..", "..", "oracle", "_ref", "muscle")
MODES = {"plain": [], "scaledist": ["-scaledist"], "eadist": ["-eadist"], "reseek": ["-reseek"]}
LINKAGES = ("avg", "min", "max", "biased")


def matrix_text(mode, n, quant, seed):
    rng = np.random.default_rng(seed)
    labels = ["s%d" % i for i in range(n)]
    lines = []
    if mode == "reseek":
        lines.append("distmx\t%d" % n)
        lines += ["%d\t%s" % (i, labels[i]) for i in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            v = float(rng.random())
            if quant:
                v = (int(v * 4) + 0.5) / 4.0
            if mode == "plain":
                v *= 7.5  # any non-negative distances
            a, b = (str(i), str(j)) if mode == "reseek" else (labels[i], labels[j])
            lines.append("%s\t%s\t%.6g" % (a, b, v))
    return "\n".join(lines) + "\n"


def main():
    for mode, flags in MODES.items():
        cases = []
        for n, quant, seed in ((9, False, 11), (12, True, 12)):
            text = matrix_text(mode, n, quant, seed)
            newick = {}
            for linkage in LINKAGES:
                with tempfile.TemporaryDirectory() as d:
                    with open(os.path.join(d, "in.tsv"), "w") as f:
                        f.write(text)
                    subprocess.run([MUSCLE, "-upgma5", "in.tsv", "-output", "out.nwk", "-linkage", linkage, "-quiet"] + flags, check=True, cwd=d,
                                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                    newick[linkage] = open(os.path.join(d, "out.nwk")).read()
            cases.append({"n": n, "quantised": quant, "input": text, "newick": newick})
        with open(os.path.join(HERE, "upgma_%s.json" % mode), "w") as f:
            json.dump({"mode": mode, "flags": flags, "cases": cases}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
