"""One timing run of the EA of a list of long pairs, for A/B runs of two trees in separate processes (profiles/r19a_ea_wide.log):

    python diag/ea_wide_time.py <root of the tree to import muscle_amd from> <ea|ap> <p12200|p300x20000|p64x13000> [nowarm]

ea = mpcgpu_ea_scores (export MPCGPU_EA_WIDE=1 for lists beyond the row-list arrays), ap = mpcgpu_align_pairs (the route CalcEADistMx had
before it became one call; for the parent commit, point the first argument at a checkout of it with its library built). Lists: one pair
12 200 x 12 200, one pair 300 x 20 000, 64 pairs of 12 related sequences of 13 000. One warm-up call unless `nowarm`, then one timed
call: host wall, time and launches of the finishing ("post") and forward/backward ("fb") families, EA bits. No other knob is set."""
import os, sys, time
root, route, lst = sys.argv[1:4]
warm = "nowarm" not in sys.argv
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))  # the PairHMM tables (tests/_golden.py)
import numpy as np
from muscle_amd._lib import MpcGpu
from muscle_amd.synth import make_family
import _golden as G

def related(lengths, seed):
    top = max(lengths)
    fam = make_family(len(lengths), top + top // 4 + 16, seed=seed)
    return [s[:L] for s, L in zip(fam, lengths)]

if lst == "p12200":
    seqs = related([12200, 12200], 71); pairs = [(0, 1)]
elif lst == "p300x20000":
    seqs = related([300, 20000], 72); pairs = [(0, 1)]
elif lst == "p64x13000":
    seqs = related([13000] * 12, 73); pairs = [(i, j) for i in range(12) for j in range(i + 1, 12)][:64]
s, t, m, i, thr = G.hmm_tables()
g = MpcGpu(0)
g.set_hmm(s, t, m, i, thr)
g.set_seqs_registry(seqs)
s1, s2 = [x for x, _ in pairs], [y for _, y in pairs]
def call():
    if route == "ea":
        return g.ea_scores(s1, s2)
    return np.array([r[2] for r in g.align_pairs(s1, s2)], np.float32)
if warm:
    call()
g.timers_reset()
t0 = time.perf_counter()
ea = call()
dt = time.perf_counter() - t0
tm = g.timers_get()
extra = ""
if route == "ea" and hasattr(g, "ea_wide_info"):
    extra = " info %s wide %s" % (g.ea_info(), g.ea_wide_info())
print("RESULT %s %s %s warm=%d call %.1f ms, post family %.2f ms in %d launches, fb family %.2f ms in %d launches, ea[0] bits %08x sum bits %08x%s"
      % (os.path.basename(os.path.normpath(root)) or "branch", route, lst, warm, dt * 1e3, tm["post"][0], tm["post"][1], tm["fb"][0], tm["fb"][1],
         int(ea.view(np.uint32)[0]), int(np.bitwise_xor.reduce(ea.view(np.uint32))), extra), flush=True)
g.close()
