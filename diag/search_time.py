"""mpcgpu_search_pairs against one mpcgpu_align_pairs call on the same pairs: G groups of K candidates of L ~ 150,
the candidates of a query drawn from a family of related sequences (a clustering pass's word-count hits are related to the query). min_ea
is the median EA of the list, so that about half of the first candidates qualify. Whole-call wall time of both, the device time of pick +
dense posteriors + alignments from mpcgpu_search_info, and the number of dense posteriors / trace-backs each side ran; both sides must
agree on every EA and on every accepted path. Run on the GPU box: python diag/search_time.py [groups] [candidates] [repeats]"""
import os
import sys
import time

import numpy as np

ROOT = os.environ.get("MPCGPU_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # MPCGPU_TREE: another checkout (its binding and library)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from muscle_amd._lib import MpcGpu
from muscle_amd.synth import make_family
import _golden as G  # hmm tables only (no oracle compute)


def main():
    ng = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    seqs = make_family(64, 150, seed=11) + make_family(64, 150, seed=12)
    rng = np.random.default_rng(7)
    groups = []
    for q in range(ng):
        x = int(rng.integers(0, len(seqs)))
        groups.append([(x, int(y)) for y in rng.choice([y for y in range(len(seqs)) if y != x], k, replace=False)])
    flat = [p for g in groups for p in g]
    s, t, m, i, thr = G.hmm_tables()
    g = MpcGpu(0)
    g.set_hmm(s, t, m, i, thr)
    g.set_seqs_registry(seqs)
    g.timers_enable(False)
    ref = g.align_pairs([x for x, _ in flat], [y for _, y in flat])  # warm: buffers, code objects
    ea_ref = np.array([r[2] for r in ref], np.float32)
    min_ea = float(np.median(ea_ref))
    if not hasattr(g, "search_pairs"):  # a checkout from before the call: its mpcgpu_align_pairs alone, for the alternating runs
        for r in range(reps):
            t0 = time.perf_counter()
            g.align_pairs([x for x, _ in flat], [y for _, y in flat])
            print("run %d: mpcgpu_align_pairs of %s: %.2f ms (%d dense posteriors + trace-backs)" % (r, ROOT, (time.perf_counter() - t0) * 1e3, len(flat)), flush=True)
        g.close()
        return
    acc, hits, ea = g.search_pairs(groups, min_ea)
    assert np.array_equal(ea.view(np.uint32), ea_ref.view(np.uint32))
    for gi, a in enumerate(acc):
        want = next((t for t in range(k) if ea_ref[gi * k + t] >= np.float32(min_ea)), None)
        assert a == want and (a is None or hits[gi][0] == ref[gi * k + a][0]), gi
    print("groups %d x %d candidates = %d pairs, L ~ 150, min_ea %.4f: %d groups accepted" % (ng, k, len(flat), min_ea, sum(a is not None for a in acc)), flush=True)
    for r in range(reps):
        t0 = time.perf_counter()
        g.align_pairs([x for x, _ in flat], [y for _, y in flat])
        t1 = time.perf_counter()
        g.search_pairs(groups, min_ea)
        t2 = time.perf_counter()
        info = g.search_info()
        print("run %d: mpcgpu_align_pairs %.2f ms (%d dense posteriors + trace-backs), mpcgpu_search_pairs %.2f ms (%d; chunks %d, general %d; "
              "pick + dense + alignment on the device %.3f ms)" % (r, (t1 - t0) * 1e3, len(flat), (t2 - t1) * 1e3, info[2], info[3], info[4], info[5] / 1e6), flush=True)
    os.environ["MPCGPU_SEARCH_FUSED"] = "0"
    for r in range(reps):
        t1 = time.perf_counter()
        g.search_pairs(groups, min_ea)
        t2 = time.perf_counter()
        info = g.search_info()
        print("run %d, MPCGPU_SEARCH_FUSED=0: mpcgpu_search_pairs %.2f ms (%d; chunks %d, general %d; dense + alignment on the device %.3f ms)"
              % (r, (t2 - t1) * 1e3, info[2], info[3], info[4], info[5] / 1e6), flush=True)
    g.close()


main()
