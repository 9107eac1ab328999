#!/usr/bin/env python3
"""A/B of the record store's long form (MPCGPU_RELAX_LONG) on one GPU: bench.py with the library of the parent commit
(--parent-lib: its gather relax for long sequences) and with this build, alternately, RUNS runs each, a process per run.

  python diag/relax_long_ab.py --parent-lib PATH/libmpcgpu.so [--runs 3] [--shape 24x6000 --shape 64x4500 --shape default] [--align 24x6000]

Per shape and side: relax_ms_per_iteration of every run, the layout string and is_fallback of the last one. --align NxL: wall time
and MD5 of `muscle_gpu -align` on the synthetic family with MPCGPU_RELAX_LONG=0 (the parent's path through this build) and unset.
One line of JSON per run on stdout; the tables of DESIGN.md 4.3 are made of them. Every child runs under its own time limit; after a
child that died of a signal or ran into its limit nothing more is started."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench(lib, shape, limit):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1"]
    if shape != "default":
        n, ln = shape.split("x")
        cmd += ["--n", n, "--len", ln]
    env = dict(os.environ)
    if lib:
        env["MPCGPU_LIB"] = lib
    t0 = time.time()
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit)
    if r.returncode != 0:
        print(r.stderr[-3000:], file=sys.stderr)
        raise SystemExit("bench.py ended with status %d: nothing more is started" % r.returncode)
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    geo = out.get("relax_geometry", {})
    ks = {k: round(v, 3) for k, v in out.get("kernel_ms_per_step", {}).items() if v}
    # (the step runs MPCFlat's two consistency iterations: the relax family's device time per step / 2)
    return {"relax_ms_per_iteration": round(ks.get("relax", 0.0) / 2, 3), "kernel_ms_per_step": ks, "value": out.get("value"), "unit": out.get("unit"),
            "layout": geo.get("layout"), "fallback": geo.get("fallback"), "wall_s": round(time.time() - t0, 1)}


def align(shape, knob, limit):
    from muscle_amd.synth import make_family, write_fasta
    n, ln = shape.split("x")
    seqs = make_family(int(n), int(ln), seed=1)
    binary = os.path.join(ROOT, "hostcxx", "_build", "muscle_gpu")
    env = dict(os.environ)
    env.pop("MPCGPU_RELAX_LONG", None)
    if knob is not None:
        env["MPCGPU_RELAX_LONG"] = knob
    with tempfile.TemporaryDirectory() as d:
        fa, out = os.path.join(d, "in.fa"), os.path.join(d, "out.afa")
        write_fasta(fa, seqs, None)
        t0 = time.time()
        r = subprocess.run([binary, "-align", fa, "-output", out, "-threads", "16"], env=env, cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                           text=True, timeout=limit)
        wall = time.time() - t0
        if r.returncode != 0:
            print(r.stderr[-3000:], file=sys.stderr)
            raise SystemExit("muscle_gpu ended with status %d: nothing more is started" % r.returncode)
        with open(out, "rb") as f:
            md5 = hashlib.md5(f.read()).hexdigest()
    return {"wall_s": round(wall, 2), "md5": md5, "gather_note": "gather" in r.stderr.lower()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--shape", action="append", default=[])
    ap.add_argument("--align", action="append", default=[])
    ap.add_argument("--limit", type=int, default=420, help="seconds per child")
    a = ap.parse_args()
    for shape in a.shape:
        for run in range(a.runs):
            for side, lib in (("parent", a.parent_lib), ("this", None)):
                print(json.dumps(dict(bench(lib, shape, a.limit), shape=shape, side=side, run=run)), flush=True)
    for shape in a.align:
        for run in range(a.runs):
            for side, knob in (("RELAX_LONG=0", "0"), ("default", None)):
                print(json.dumps(dict(align(shape, knob, a.limit), shape=shape, side=side, run=run, what="muscle_gpu -align")), flush=True)


if __name__ == "__main__":
    main()
