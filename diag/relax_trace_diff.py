"""diag/relax_trace_diff.py — do two builds of the library take the same decisions on the host side of the relax?

usage: python diag/relax_trace_diff.py LIB_A LIB_B [--gpu] [--only SUBSTRING[,SUBSTRING...]] [--keep DIR]

Runs a fixed list of (input, environment) cases on each library, one child process per library, with MPCGPU_TRACE=3 and stderr
captured, and compares, case by case,
  * the trace lines that start with "[mpcgpu] band tiles", "[mpcgpu] tile ", "[mpcgpu] relax band", "[mpcgpu] relax var"
    (every cut the shape search tries, the fit rounds, the first 64 tiles word by word, the launch geometry),
  * mpcgpu_relax_info's string and fallback flag (or the error a case ends with).
Only the number in "cut, checked and uploaded in ... ms" is masked. Exit status 1 on any difference.

The cases are the environment tables of tests/test_emu_parity.py (test_emu_relax_band_tiles, test_emu_relax_var_geometries,
test_emu_relax_small_lds_shapes, test_emu_relax_tile_splitting, test_emu_relax_two_slots_per_pair, test_emu_relax_band_tiles_races),
RELAX_ENVS of tests/_pair_order.py on generated orders with the relax in two position ranges, and InitPairs order in two ranges
(k0 > 0: the cutter drops the super-tiles outside the range). --gpu adds two cases at production size, for libmpcgpu.so on a
device: bench.py's 1000 x L~400 family and the first 1000 records of tests/golden/rdrp_first1000.fa.gz (one relax each).
Without --gpu the libraries are emulator builds (tests/emu)."""
import argparse
import difflib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KEPT = ("[mpcgpu] band tiles", "[mpcgpu] tile ", "[mpcgpu] relax band", "[mpcgpu] relax var", "@@")
MASK = re.compile(r"(cut, checked and uploaded in )[0-9.]+( ms)")

VAR_PRIMARY = {"MPCGPU_RELAX_TILES": "pairs"}
VAR_FALLBACK = {"MPCGPU_RELAX_TILES": "pairs", "MPCGPU_RELAX_LDS_KB": "1", "MPCGPU_RELAX_LDS_KB_1024": "160"}
BAND_TILES_ENVS = [  # test_emu_relax_band_tiles
    {"MPCGPU_RELAX_SHAPE": "8,8"},
    {"MPCGPU_RELAX_SHAPE": "8,8", "MPCGPU_RELAX_SLOTS": "1"},
    {"MPCGPU_RELAX_SHAPE": "4,2", "MPCGPU_RELAX_SLOTS": "2"},
    {"MPCGPU_RELAX_SHAPE": "1,1"},
    {"MPCGPU_RELAX_LDS_KB": "10"},
    {"MPCGPU_RELAX_LDS_KB": "8"},
    {"MPCGPU_RELAX_LDS_KB": "12", "MPCGPU_RELAX_SHAPE": "2,2,5"},
    {"MPCGPU_RELAX_TILES": "pairs"},
    {"MPCGPU_RELAX_FORM": "walk"},
    {"MPCGPU_RELAX_FORM": "walk", "MPCGPU_RELAX_SHAPE": "4,2", "MPCGPU_RELAX_SLOTS": "2"},
    {"MPCGPU_RELAX_WIN_PCT": "100000"},
    {"MPCGPU_RELAX_WIN_PCT": "100000", "MPCGPU_RELAX_SHAPE": "2,2,8", "MPCGPU_RELAX_LDS_KB": "20"},
    {"MPCGPU_RELAX_WIN_PCT": "100000", "MPCGPU_RELAX_LDS_KB": "9"},
    {"MPCGPU_RELAX_ORDER": "pairs"},
    {"MPCGPU_RELAX_ORDER": "1"},
    {"MPCGPU_RELAX_ORDER": "3", "MPCGPU_RELAX_SHAPE": "8,8", "MPCGPU_RELAX_SLOTS": "1"},
    {"MPCGPU_RELAX_ORDER": "pairs", "MPCGPU_RELAX_FORM": "walk", "MPCGPU_RELAX_SHAPE": "4,2", "MPCGPU_RELAX_SLOTS": "2"},
]
VAR_GEOMETRY_ENVS = [  # test_emu_relax_var_geometries
    VAR_PRIMARY, VAR_FALLBACK, dict(VAR_FALLBACK, MPCGPU_RELAX_LDS_KB_1024="12"), {"MPCGPU_RELAX_TILES": "pairs", "MPCGPU_RELAX_LDS_KB": "12"},
    {"MPCGPU_RELAX_SLOTS": "3"}, {"MPCGPU_RELAX_LDS_KB": "6"}]
RACE_FORMS = [{"MPCGPU_RELAX_WIN_PCT": "100000"}, {"MPCGPU_RELAX_FORM": "walk"}, {"MPCGPU_RELAX_WIN_PCT": "100000", "MPCGPU_RELAX_ORDER": "1"}]


def cases(gpu):
    """-> [(name, sequences, environment, rectangles of a custom pair order or None, relax in two position ranges?)]"""
    import numpy as np
    import _pair_order as PO
    from muscle_amd.synth import make_family, read_fasta
    long70 = make_family(1, 70, seed=9)[0]
    out = []
    band = make_family(7, 75, seed=11) + make_family(3, 18, seed=5) + [long70, "MKV"]
    for i, env in enumerate(BAND_TILES_ENVS):
        out.append(("band_tiles[%d]" % i, band, env, None, False))
    var = make_family(9, 18, seed=5) + [long70, "MKV"]
    for i, env in enumerate(VAR_GEOMETRY_ENVS):
        out.append(("var_geometries[%d]" % i, var, env, None, False))
    po = make_family(8, 40, seed=21) + ["MKV", long70]
    for i, env in enumerate(PO.RELAX_ENVS):
        out.append(("pair_order_relax_kernels[%d]" % i, po, env, PO.random_order(len(po), np.random.default_rng(11 + i)), True))
    for kb in (2, 1):
        out.append(("small_lds_shapes[%d]" % kb, make_family(6, 18, seed=6), {"MPCGPU_RELAX_LDS_KB": str(kb)}, None, False))
    out.append(("tile_splitting", make_family(8, 16, seed=8), {"MPCGPU_RELAX_SLOTS": "3"}, None, False))
    out.append(("two_slots_per_pair", ["AC" * 165, "AC" * 162 + "A", "CA" * 164], {}, None, False))
    races = make_family(6, 40, seed=3) + make_family(3, 18, seed=5)
    for mode in ("late", "reverse", "random"):
        for f, form in enumerate(RACE_FORMS):
            env = {"MPCGPU_RELAX_SHAPE": "4,4,3", "MPCGPU_RELAX_LDS_KB": "10"}
            env.update(form)
            env.update({"EMU_DMA": "late"} if mode == "late" else {"EMU_SCHED": mode})
            out.append(("band_tiles_races[%s,%d]" % (mode, f), races, env, None, False))
    out.append(("sharded_range", band, {}, None, True))
    out.append(("sharded_range_search", band, {"MPCGPU_RELAX_LDS_KB": "10"}, None, True))
    # more than 64 sequences: past the few-sequences route, to the 8x8 cut and what follows it
    out.append(("many_sequences", make_family(70, 14, seed=17), {}, None, False))
    out.append(("many_sequences_search", make_family(66, 14, seed=18) + [long70], {"MPCGPU_RELAX_LDS_KB": "10"}, None, False))
    if gpu:
        out.append(("bench_1000x400", make_family(1000, 400, seed=1), {}, None, False))
        out.append(("rdrp_1000", read_fasta(os.path.join(ROOT, "tests", "golden", "rdrp_first1000.fa.gz"))[:1000], {}, None, False))
    return out


def say(text):
    os.write(2, (text + "\n").encode())  # unbuffered, like the library's stderr: the markers stay in order with its lines


def child(lib, gpu, only):
    import _golden as G
    import _pair_order as PO
    from muscle_amd._lib import MpcGpu
    big = ("bench_1000x400", "rdrp_1000")
    for name, seqs, env, rects, halves in cases(gpu):
        if only and not any(o in name for o in only.split(",")):
            continue
        say("@@case %s %s" % (name, sorted(env.items())))
        try:
            with PO.Env(env):
                g = MpcGpu(0, lib)
                g.set_hmm(*G.hmm_tables())
                g.set_seqs(seqs)
                if rects is not None:
                    g.set_pair_order(rects)
                g.calc_posteriors()
                g.build_store()
                N = g.npairs
                for _ in range(1 if name in big else 2):
                    if halves:
                        g.cons_iter(0, N // 3)
                        g.cons_iter(N // 3, N)
                    else:
                        g.cons_iter()
                    g.cons_commit()
                say("@@info %s fallback=%s" % g.relax_info())
                g.close()
        except Exception as e:  # a case may end in an error: the same error on both sides
            say("@@error %s: %s" % (type(e).__name__, e))
    say("@@done")


def run(lib, gpu, only, keep, tag):
    env = dict(os.environ, MPCGPU_TRACE="3")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(lib)] + (["--gpu"] if gpu else []) + (["--only", only] if only else [])
    p = subprocess.run(cmd, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=1500)
    text = p.stderr.decode(errors="replace")
    if keep:
        os.makedirs(keep, exist_ok=True)
        with open(os.path.join(keep, "relax_trace_%s.log" % tag), "w") as f:
            f.write(text)
    lines = [MASK.sub(r"\1*\2", ln) for ln in text.split("\n") if ln.startswith(KEPT)]
    if p.returncode != 0 or "@@done" not in lines:
        sys.exit("relax_trace_diff: the run on %s ended with status %d:\n%s" % (lib, p.returncode, text[-3000:]))
    per_case, name = {}, None
    for ln in lines:
        if ln.startswith("@@case "):
            name = ln.split()[1]
            per_case[name] = []
        if name is not None and ln != "@@done":
            per_case[name].append(ln)
    return per_case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--child")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--keep", default="", help="directory that receives the two full traces")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.gpu, a.only)
    if len(a.libs) != 2:
        ap.error("two library paths")
    A, B = run(a.libs[0], a.gpu, a.only, a.keep, "a"), run(a.libs[1], a.gpu, a.only, a.keep, "b")
    differing = []
    for name in sorted(set(A) | set(B), key=lambda k: list(A).index(k) if k in A else len(A)):
        la, lb = A.get(name, []), B.get(name, [])
        if la != lb:
            differing.append(name)
            print("DIFFERENT: %s" % name)
            for d in list(difflib.unified_diff(la, lb, a.libs[0], a.libs[1], lineterm="", n=1))[:40]:
                print("    " + d[:300])
    nlines = sum(len(v) for v in A.values())
    print("relax_trace_diff: %d cases, %d compared lines, %d cases differ%s" % (len(A), nlines, len(differing), (": " + ", ".join(differing)) if differing else ""))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
