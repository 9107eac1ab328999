"""The drop-in's UClust::Run by windows (hostcxx/mpcflat_gpu.cpp; MUSCLE_GPU_UCLUST_WINDOW) — shared by tests/test_gpu_dropin_uclust.py
(the device), tests/test_dropin_uclust_emu.py (the emulator build of the library) and tests/golden/make_uclust_golden.py (which runs the
compiled reference on the same sets and writes tests/golden/uclust_dropin.json).

Three sets of 40 .. 64 sequences of 60 .. 120 positions (muscle_amd.synth):
  dups        four unrelated founders, each with twelve near-duplicates (3 % substitutions): most queries become members
  unrelated   forty sequences without a common ancestor: every query becomes a centroid, so with W > 1 every window's second query
              finds another index than its list was made on
  mixed       eight founders of falling length, each followed IN LENGTH ORDER by seven near-duplicates a few residues shorter, so that
              new centroids arrive between members
The emulator (tens of milliseconds a pair) runs thin forms of the same three, twelve sequences of 52 .. 82 positions each (SETS_EMU: two
founders with five near-duplicates; twelve unrelated; three founders each followed by three near-duplicates).
`muscle_gpu -super5` (and `-uclust in.fa -output c.fa -minea 0.9` where the reference's own run exits 0: the fixture says) must write the
reference's bytes under every window size, with -threads 1 and -threads 4. TEST INFRASTRUCTURE."""
import hashlib
import json
import os
import random
import re
import subprocess
import tempfile

from muscle_amd.synth import AMINO, make_family, write_fasta

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uclust_dropin.json")
SETS = ["dups", "unrelated", "mixed"]
SETS_EMU = ["dups_s", "unrelated_s", "mixed_s"]
WINDOWS = [0, 1, 4, 64]
ROW = re.compile(r"^\[muscle_gpu\] uclust windows (\d+), cut (\d+), pairs sent (\d+), pairs sent for queries that were sent again (\d+), library calls (\d+)$", re.M)


def near(seq, rng, p_sub=0.03):
    return "".join(rng.choice(AMINO) if rng.random() < p_sub else c for c in seq)


def input_set(name):
    small = name.endswith("_s")
    kind = name[:-2] if small else name
    rng = random.Random({"dups": 5, "unrelated": 6, "mixed": 7}[kind] + (10 if small else 0))
    if kind == "dups":
        seqs = []
        for f in range(2 if small else 4):
            founder = make_family(1, (66 if small else 100) - 6 * f, seed=300 + f)[0]
            seqs += [founder] + [near(founder, rng) for _ in range(5 if small else 12)]
    elif kind == "unrelated":
        seqs = [make_family(1, 60 + (7 * k) % (23 if small else 61), seed=400 + k)[0] for k in range(12 if small else 40)]
    elif kind == "mixed":
        seqs = []
        for f in range(3 if small else 8):
            founder = make_family(1, 140, seed=500 + f)[0][:(76 if small else 120) - 8 * f]
            seqs += [founder] + [near(founder, rng, 0.02 + 0.01 * j)[:len(founder) - j] for j in range(1, 4 if small else 8)]
    else:
        raise KeyError(name)
    order = list(range(len(seqs)))
    rng.shuffle(order)  # (the file order is not the length order)
    return [seqs[k] for k in order]


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def run(binary, name, cmd, threads, window, timeout=600):
    """-> (MD5 of the output file, the five figures of the `uclust windows` row)"""
    seqs = input_set(name)
    with tempfile.TemporaryDirectory() as d:
        write_fasta(os.path.join(d, "in.fa"), seqs)
        args = {"super5": ["-super5", "in.fa", "-output", "out", "-threads", str(threads), "-quiet"],
                "uclust": ["-uclust", "in.fa", "-output", "out", "-minea", "0.9", "-threads", str(threads), "-quiet"]}[cmd]
        env = dict(os.environ, MUSCLE_GPU_TIMING="1")
        if window is None:
            env.pop("MUSCLE_GPU_UCLUST_WINDOW", None)
        else:
            env["MUSCLE_GPU_UCLUST_WINDOW"] = str(window)
        r = subprocess.run([binary] + args, cwd=d, timeout=timeout, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env)
        err = r.stderr.decode(errors="replace")
        assert r.returncode == 0, (name, cmd, threads, window, err[-2000:])
        with open(os.path.join(d, "out"), "rb") as f:
            md5 = hashlib.md5(f.read()).hexdigest()
    m = ROW.search(err)
    assert m, "no `uclust windows` row in the timing report:\n" + err[-2000:]
    return md5, tuple(int(x) for x in m.groups())


def check(binary, name, cmd, threads):
    """every window size writes the reference's bytes; what the report row must say of the route"""
    fx = fixture()[name]
    if cmd == "uclust" and not fx["uclust_exit0"]:
        return
    want = fx[cmd + "_md5"]
    n = None  # sequences UClust::Run sees (-super5 dereplicates first): the windows of the W = 1 run, one per query
    for w in WINDOWS:
        md5, (windows, cuts, sent, resent, calls) = run(binary, name, cmd, threads, w)
        print(name, cmd, "threads", threads, "W", w, "windows", windows, "cut", cuts, "pairs", sent, "resent", resent, "calls", calls)
        assert md5 == want, (name, cmd, threads, w, md5, want)
        if w == 0:  # the parent's route: the reference's Run over the drop-in Search
            assert (windows, cuts, sent, resent, calls) == (0, 0, 0, 0, 0)
            continue
        if w == 1:
            n = windows
            assert 2 <= n <= len(input_set(name)) and cuts == 0 and resent == 0 and calls <= n
            if cmd == "uclust":
                assert n == len(input_set(name))
            continue
        assert windows >= (n + w - 1) // w and calls <= windows and cuts < windows
        kind = name[:-2] if name.endswith("_s") else name
        if w == 64 and kind == "mixed":
            assert cuts >= 1 and calls < n, (cuts, calls, n)
        if w == 64 and kind == "dups":
            assert calls < n
        if kind == "unrelated":  # every query becomes a centroid, so a window is cut wherever a later query's list is no longer the one it was sent with
            assert cuts >= 1, (w, windows, cuts)
