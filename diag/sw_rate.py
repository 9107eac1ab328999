"""diag/sw_rate.py — the measurements of the Smith-Waterman guide tree (kernels_sw.h), one line each:
  rate N L     kernel time of mpcgpu_sw_scores for all pairs of an N x L~ synthetic X-terminated family, as DP cells per second
  ref N L T    wall time of the compiled reference's `muscle -swdistmx` on the same family with T threads, per pair
  e2e N L      wall time of `muscle_gpu -super7 in.fa` from a bare FASTA (no tree option), with the MUSCLE_GPU_TIMING report
usage: python diag/sw_rate.py rate 2000 250 | ref 512 250 16 | e2e 10000 250"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from muscle_amd.synth import make_family, write_fasta  # noqa: E402

what, n, L = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
seqs = [s + "X" for s in make_family(n, L, seed=13)]
npairs = n * (n - 1) // 2

if what == "rate":
    import _golden as G
    import _sw
    from muscle_amd._lib import MpcGpu
    g = MpcGpu(0)
    s, t, m, i, thr = G.hmm_tables()
    g.set_hmm(s, t, m, i, thr)
    g.set_seqs_registry(seqs)
    g.sw_set_scores(*_sw.tables())
    for rep in range(3):
        t0 = time.perf_counter()
        sc = g.sw_scores()
        wall = time.perf_counter() - t0
        pairs, cells, batches, chains, long_chains, ns = g.sw_info()
        print("sw_scores %d x L~%d rep %d: %d pairs, %d cells, %d chains, %d batches: kernel %.3f ms = %.3e cells/s; call %.3f s; checksum %.6e"
              % (n, L, rep, pairs, cells, chains, batches, ns * 1e-6, cells / (ns * 1e-9), wall, float(sc.astype("float64").sum())), flush=True)
    g.close()
elif what == "ref":
    import _msa
    th = sys.argv[4]
    with tempfile.TemporaryDirectory() as d:
        write_fasta(os.path.join(d, "in.fa"), seqs)
        t0 = time.perf_counter()
        subprocess.run([_msa.REF_MUSCLE, "-swdistmx", "in.fa", "-guidetreeout", "t.nwk", "-threads", th, "-quiet"], check=True, cwd=d,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=3000)
        dt = time.perf_counter() - t0
    print("reference -swdistmx %d x L~%d, %s threads: %.2f s wall (UPGMA5 included) = %.3f us per pair" % (n, L, th, dt, dt / npairs * 1e6), flush=True)
elif what == "e2e":
    import _msa
    from muscle_amd.hostinfo import usable_cores
    with tempfile.TemporaryDirectory() as d:
        write_fasta(os.path.join(d, "in.fa"), seqs)
        t0 = time.perf_counter()
        subprocess.run([_msa.GPU_MUSCLE, "-super7", "in.fa", "-output", "out.afa", "-threads", str(usable_cores()), "-quiet"], check=True, cwd=d,
                       stdout=subprocess.DEVNULL, env=dict(os.environ, MUSCLE_GPU_TIMING="1"), timeout=3000)
        dt = time.perf_counter() - t0
    print("muscle_gpu -super7 %d x L~%d from a bare FASTA: %.2f s wall" % (n, L, dt), flush=True)
