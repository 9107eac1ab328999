"""`muscle_gpu -super5` end to end with UClust::Run by windows against another build of the drop-in: the two binaries
alternately, every run a cold process, on make_family(n, 150, seed=1) — wall time, the `AlignPairFlat lists: library` and `uclust windows`
rows of MUSCLE_GPU_TIMING=1 and the MD5 of the MSA.
Run on the GPU box: python diag/super5_windows.py <other muscle_gpu> <n> <runs> [window]"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from muscle_amd.synth import make_family, write_fasta


def one(binary, fasta, d, env):
    out = os.path.join(d, "out.afa")
    t0 = time.perf_counter()
    r = subprocess.run([binary, "-super5", fasta, "-output", out, "-threads", "8", "-quiet"], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                       env=dict(os.environ, MUSCLE_GPU_TIMING="1", **env))
    wall = time.perf_counter() - t0
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-2000:]
    lib = re.search(r"AlignPairFlat lists: library\s+([0-9.]+) s\s+(\d+) calls", err)
    uc = re.search(r"uclust windows.*", err)
    with open(out, "rb") as f:
        md5 = hashlib.md5(f.read()).hexdigest()
    return "wall %.2f s, AlignPairFlat lists: library %s s %s calls, %s, MD5 %s" % (wall, lib.group(1), lib.group(2), uc.group(0) if uc else "no uclust windows row", md5)


def main():
    other, n, runs = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    window = sys.argv[4] if len(sys.argv) > 4 else "64"
    mine = os.path.join(ROOT, "hostcxx", "_build", "muscle_gpu")
    with tempfile.TemporaryDirectory() as d:
        fasta = os.path.join(d, "in.fa")
        write_fasta(fasta, make_family(n, 150, seed=1))
        for r in range(runs):
            print("n %d run %d other build: %s" % (n, r, one(other, fasta, d, {})), flush=True)
            print("n %d run %d this build W=%s: %s" % (n, r, window, one(mine, fasta, d, {"MUSCLE_GPU_UCLUST_WINDOW": window})), flush=True)
        print("n %d this build W=0: %s" % (n, one(mine, fasta, d, {"MUSCLE_GPU_UCLUST_WINDOW": "0"})), flush=True)
        print("n %d this build W=8: %s" % (n, one(mine, fasta, d, {"MUSCLE_GPU_UCLUST_WINDOW": "8"})), flush=True)


main()
