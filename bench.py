#!/usr/bin/env python3
"""bench.py — sequence-pairs/sec of the MPCFlat all-pairs posterior stage on MI355X.

One "step" = one full pass of the hot path over the workload: fwd + bwd + posterior (+ sparsify +
EA score) for ALL N(N-1)/2 pairs, then 2 consistency-relax iterations (BASELINE.json metric;
timed region = MPCFlat::CalcPosteriors + MPCFlat::Consistency, mpcflat.cpp:313,328). Inputs
(sequences, HMM tables) are resident on the device before the timed region. Synthetic protein
family (muscle_amd/synth.py, seed 1), default N=1000 L~400 = BASELINE configs[2].

  python bench.py [--gpus N --steps K --warmup W] [--n 1000 --len 400] [--dump-outputs DIR] [--full]
  N>1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
       (pairs sharded over ranks, RCCL all-gather of sparse posteriors before relax; weak=no:
        total work is fixed, so "scaling": "strong")
Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the K steps and prints the line (roofline figures included: they come from the
timed steps' own device timers and committed counter passes). --full adds what takes work of its own after the timed
region: the digest self-check against the compiled reference's output, the real-data leg and the CPU baseline
(--no-parity / --no-real-data / --no-cpu-baseline leave out one of them). --dump-outputs DIR writes what the last timed
step computed (dump_outputs below) so that two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
FP32_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: FP32 vector == FP32 MFMA dense peak


def load_hmm():
    z = np.load(os.path.join(ROOT, "tests", "golden", "hmm_amino.npz"))
    return z["start"], z["trans"], z["match"], z["ins"], np.float32(z["min_sparse_score"])


def stage_a_flops(lens):
    """F_A = 164*(LX+1)(LY+1) + 5*LX*LY FP32 ops per pair."""
    from muscle_amd.mpcflat import pair_lengths
    lx, ly = pair_lengths(lens)
    return float(np.sum(164.0 * (lx + 1) * (ly + 1) + 5.0 * lx * ly))


def stage_b_bytes(lens, nnz):
    """per (pair,Z) the operands read once = 8*(nnz_XZ+nnz_YZ) + 4*(LX+LY+2) bytes,
    summed over all pairs and all Z != X,Y; plus 4*nnz written per pair."""
    lens = np.asarray(lens, np.int64)
    n = len(lens)
    ii, jj = np.triu_indices(n, 1)
    nnz = np.asarray(nnz, np.int64)
    per_seq = np.zeros(n, np.int64)
    np.add.at(per_seq, ii, nnz)
    np.add.at(per_seq, jj, nnz)
    ent = 8 * (per_seq[ii] + per_seq[jj] - 2 * nnz)
    ptr = 4 * (n - 2) * (lens[ii] + lens[jj] + 2)
    return float(np.sum(ent + ptr + 4 * nnz))


def pmc_entry(kernel, n, length):
    """Committed PMC figures of `kernel` for this workload (profiles/pmc_traffic.json, written by scripts/pmc_summary.py from separate
    `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` / SQ passes of this same command); None when no pass exists for it."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        with open(path) as f:
            return json.load(f).get("%s@%dx%d" % (kernel, n, length))
    except (OSError, ValueError):
        return None


def parity_check(g, a):
    """Self-check after the timed region: the store left by the last timed step (stage 2 = after both relax
    iterations) and the EA values against the digests the compiled reference produced for this exact workload
    (tests/golden/mpcbig_*.npz, tests/golden/make_golden.py big). -> ("match" | "MISMATCH" | None, detail)."""
    import _bigdigest as D
    name = D.fixture_for_fasta(a.fasta, a.n) if a.fasta else D.fixture_for(a.n, a.len, a.seed)
    if name is None:
        return None, "no reference-generated digest fixture for this workload (fixtures: %s)" % ", ".join(sorted(D.BIG_SETS))
    z = D.load(name)
    err = D.compare_ea(z, g.get_ea()) or D.compare_stage(z, 2, g)
    return ("match", "EA bits and stage-2 sparse posteriors (offsets, columns, float bits) of all pairs equal the "
            "reference's: tests/golden/mpcbig_%s.npz" % name) if err is None else ("MISMATCH", err)


DUMP_BYTES = 64 * 10**6     # --dump-outputs: at most this much in all
DUMP_EA_PAIRS = 1 << 20     # per-pair figures of every pair up to this many pairs, else of a seeded sample of this many
DUMP_STORE_PAIRS = 1024     # sparse posterior matrices of a seeded sample of this many pairs


def dump_outputs(g, d):
    """--dump-outputs: what a caller of the timed path (MPCFlat::CalcPosteriors + Consistency) receives after the last timed step,
    as .npy files in d; pairs are numbered in InitPairs order, integers are stored as float64 (exact):
      ea.npy (f32), nnz.npy (f64)    per pair: the expected-accuracy score and the number of stored posteriors — of every pair, or
                                     of the pairs listed in pairs.npy (seeded sample, sorted) when there are more than DUMP_EA_PAIRS
      store_pairs.npy (f64)          a seeded sample of pairs (sorted) whose sparse posterior matrices follow, back to back:
      store_offsets.npy (f64)        LX + 1 row offsets per pair
      store_post.npy (f32), store_col.npy (f64)   posterior and column of every stored cell
    The matrix sample ends early where the files would pass DUMP_BYTES in all. The same arguments give the same inputs, so two
    builds can be compared file by file."""
    os.makedirs(d, exist_ok=True)
    npairs = g.npairs
    ea, nnz = g.get_ea(), g.get_nnz()
    files = {}
    if npairs > DUMP_EA_PAIRS:
        pick = np.sort(np.random.default_rng(1).choice(npairs, DUMP_EA_PAIRS, replace=False))
        files["pairs"] = pick.astype(np.float64)
        ea, nnz = ea[pick], nnz[pick]
    files["ea"] = ea.astype(np.float32)
    files["nnz"] = nnz.astype(np.float64)
    used = sum(v.nbytes for v in files.values()) + 128 * (len(files) + 4)  # + the .npy headers
    ks, offs, post, col = [], [], [], []
    for k in np.sort(np.random.default_rng(2).choice(npairs, min(npairs, DUMP_STORE_PAIRS), replace=False)):
        (o, v), = g.get_sparse_range(int(k), int(k) + 1)
        size = 8 + 8 * len(o) + 6 * len(v)  # pair number + offsets + 12 bytes per cell (v holds two words per cell)
        if used + size > DUMP_BYTES:
            break
        used += size
        ks.append(k)
        offs.append(o)
        post.append(v[0::2].view(np.float32))
        col.append(v[1::2])

    def cat(parts, dtype):
        return np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)

    files["store_pairs"] = np.asarray(ks, np.float64)
    files["store_offsets"] = cat(offs, np.float64)
    files["store_post"] = cat(post, np.float32)
    files["store_col"] = cat(col, np.float64)
    for name, arr in files.items():
        np.save(os.path.join(d, name + ".npy"), arr)


def real_data_leg(g, torch, run_stage, steps=1):
    """The realistic input beside the synthetic headline ("also report one realistic set"): the first 1000 records of the
    reference's test_data/rdrp/rdrp.fa (tests/golden/rdrp_first1000.fa.gz; ~6.8 stored cells per row against ~2). One pass that doubles
    as warm-up and SAMPLED parity pin (tests/golden/mpcbig_rdrp1000_sampled.npz: the compiled reference's stage A for all 499 500
    pairs — EA and stage-0 digests — and ConsPair of iteration 1 for 2048 seeded pairs), then `steps` timed steps. -> dict."""
    import _bigdigest as D
    from muscle_amd.mpcflat import CONSISTENCY_ITERS
    from muscle_amd.synth import read_fasta
    path = os.path.join(ROOT, "tests", "golden", "rdrp_first1000.fa.gz")
    n = 1000
    seqs = read_fasta(path)[:n]
    lens = [len(s) for s in seqs]
    npairs = n * (n - 1) // 2
    g.set_seqs(seqs)
    # pass 1 (untimed): the stage step by step, checked against the reference where a pin exists
    parity, detail = None, "no sampled fixture (tests/golden/make_golden.py big-sampled)"
    name = D.sampled_fixture_for_fasta(path, n)
    g.calc_posteriors(0, npairs)
    g.build_store()
    if name is not None:
        z = D.load(name)
        err = D.compare_ea(z, g.get_ea()) or D.compare_stage(z, 0, g)
    g.cons_iter(0, npairs)
    g.cons_commit()
    if name is not None:
        err = err or D.compare_sample(z, g)
        parity = "match" if err is None else "MISMATCH"
        detail = ("EA bits and stage-0 sparse posteriors of ALL %d pairs, and the stage-1 matrices (one relax iteration) of %d seeded pairs, equal the "
                  "compiled reference's: tests/golden/mpcbig_%s.npz" % (npairs, len(z["sample_k"]), name)) if err is None else err
    g.cons_iter(0, npairs)
    g.cons_commit()
    name2 = D.stage2_fixture_for_fasta(path, n)
    if name2 is not None and parity == "match":
        # the second iteration too: the stage-2 matrices of the pairs among 6 seeded sequences (tests/golden/make_golden.py big-stage2)
        err2 = D.compare_stage2_clique(D.load(name2), g)
        if err2 is None:
            detail += "; and the stage-2 matrices (two relax iterations) of the %d pairs among 6 seeded sequences: tests/golden/mpcbig_%s.npz" % (len(D.load(name2)["stage2_k"]), name2)
        else:
            parity, detail = "MISMATCH", err2
    g.synchronize()
    g.timers_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run_stage(g, lens, None, torch_mod=torch)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    timers = g.timers_get()
    geo, fallback = g.relax_info()
    nnz = g.get_nnz()
    iters = max(steps * CONSISTENCY_ITERS, 1)
    relax_ms = timers["relax"][0] / iters
    launched = geo.split("kernel=")[1].split(";")[0].strip() if "kernel=" in geo else None
    out = {"workload": "first %d records of rdrp_first1000.fa.gz (real proteins, mean L %.0f): %d pairs, %d stored posteriors (%.1f per row)"
                       % (n, float(np.mean(lens)), npairs, int(nnz.sum()), float(nnz.sum()) / max(sum(lens[i] * (n - 1 - i) for i in range(n)), 1)),
           "value": npairs * steps / el, "unit": "pairs/s", "steps": steps, "ms_per_step": 1000.0 * el / steps,
           "relax_ms_per_iteration": relax_ms, "kernel_ms_per_step": {k: v[0] / steps for k, v in timers.items()},
           "relax_geometry": {"layout": geo, "fallback": fallback},
           "parity_sample": parity, "parity_detail": detail}
    pmc = None
    for key in (("relax_band_kernel/MpcRbBlocksAsm" if launched and "MpcRbBlocks" in launched else "relax_band_kernel"), "relax_band_kernel"):
        pmc = pmc or pmc_entry(key, n, 0)
    if pmc is not None and launched is not None and launched in pmc.get("kernel", ""):
        avg_s = relax_ms * 1e-3
        clock = float(pmc.get("clock_hz") or 2.1e9)
        fr = {"hbm": float(pmc["hbm_bytes_per_launch"]) / avg_s / 1e9 / HBM_PEAK_GBS}
        sq = pmc.get("sq_per_launch", {})
        if "SQ_INSTS_VALU" in sq:
            try:
                with open(os.path.join(ROOT, "muscle_amd", "csrc", "isa_cost.json")) as f:
                    cost = float(json.load(f)["relax_band_kernel/MpcRbBlocksAsm" if "MpcRbBlocks" in launched else "relax_band_kernel"]["mean_issue_cost"])
            except (OSError, ValueError, KeyError):
                cost = 1.19
            fr["valu_issue"] = sq["SQ_INSTS_VALU"] * cost * 2.0 / (1024 * clock) / avg_s
        if "SQ_LDS_IDX_ACTIVE" in sq:
            fr["lds"] = sq["SQ_LDS_IDX_ACTIVE"] / (256 * clock) / avg_s
            if "SQ_LDS_BANK_CONFLICT" in sq:
                fr["lds_net_of_conflicts"] = (sq["SQ_LDS_IDX_ACTIVE"] - sq["SQ_LDS_BANK_CONFLICT"]) / (256 * clock) / avg_s
        out["measured_fractions"] = fr
        out["counter_source"] = pmc.get("source")
        si = g.store_info()
        min_bytes = float(si["record_bytes"] + si["window_bytes"] + 16 * si["own_entries"])
        out["min_bytes_per_launch"] = min_bytes
        out["traffic_over_min_bytes"] = float(pmc["hbm_bytes_per_launch"]) / min_bytes
        gross = {k: v for k, v in fr.items() if k != "lds_net_of_conflicts"}
        b = max(gross, key=gross.get)
        out["bound"], out["frac"] = b, (fr["lds_net_of_conflicts"] if b == "lds" and "lds_net_of_conflicts" in fr else gross[b])
    else:
        out["measured_fractions"] = None
        out["pmc_rejected"] = "no committed PMC pass of %r for this input" % launched
    return out


def cpu_baseline(seqs, n_full, budget_s=20.0):
    """Reference (oracle/_ref/libmuscle_ref.so = the reference's own MPCFlat::CalcPosteriors +
    ConsIter, OpenMP over all host cores) on a bounded sample of the same family, extrapolated to
    the full N: stage A scales per pair, relax per (pair,Z) triple. Falls back to the C oracle
    ("port") if the compiled reference is not shipped."""
    from muscle_amd.hostinfo import usable_cores
    cores = usable_cores()
    n_s = min(len(seqs), 192)  # stage A ~19 s + 2 relax iterations ~6 s of the compiled reference on the box's 16-core quota (128: 8.4 + 1.6 s measured)
    sample = seqs[:n_s]
    np_s = n_s * (n_s - 1) // 2
    try:
        import _ref as R
        if not R.available():
            raise RuntimeError("no libmuscle_ref.so")
        R.init_hmm(False, 0)
        import ctypes as C
        L = R.lib()
        arr = (C.c_char_p * len(sample))(*[s.encode() for s in sample])
        if L.ref_mpc_begin(len(sample), arr, cores) != 0:
            raise RuntimeError("ref_mpc_begin failed")
        t0 = time.perf_counter(); L.ref_mpc_calc_posteriors(); tA = time.perf_counter() - t0
        t0 = time.perf_counter(); L.ref_mpc_cons_iter(0); L.ref_mpc_cons_iter(1); tB = time.perf_counter() - t0
        kind = "reference"
    except Exception as e:  # noqa: BLE001
        import _oracle as O
        s, t, m, i, thr = load_hmm()
        h = O.make_hmm(s, t, m, i)
        st = O.Store(sample)
        t0 = time.perf_counter(); st.calc_posteriors(h, threads=cores); tA = time.perf_counter() - t0
        t0 = time.perf_counter(); c1 = st.cons_iter(threads=cores); c1.cons_iter(threads=cores); tB = time.perf_counter() - t0
        kind = "port"
    per_pair_a = tA / np_s
    per_triple = tB / (2.0 * np_s * (n_s - 2))
    per_pair_full = per_pair_a + 2.0 * (n_full - 2) * per_triple
    out = {"value": 1.0 / per_pair_full, "unit": "pairs/s", "cores": cores, "kind": kind,
           "extrapolated": n_s < n_full,
           "sample": "%s on the first %d sequences of the same family (%d pairs) on this box: stage A %.2f s, 2 relax iterations %.2f s; "
                     "EXTRAPOLATED to N=%d as t_pair = tA/pairs + 2*(N-2)*t_triple (stage A scales per pair, relax per (pair,Z) triple) — "
                     "not a timed N=%d run" % ("compiled reference (MPCFlat::CalcPosteriors + ConsIter, OpenMP)" if kind == "reference"
                                               else "C restatement (oracle/, reference binary not shipped)", n_s, np_s, tA, tB, n_full, n_full)}
    # the same reference TIMED (nothing extrapolated) on a GPU box's host cores, and what this formula predicted for that size
    # from a 128-sequence sample in the same run: committed by diag/ref_time.py (scripts/gpu.sh ... sh:python diag/ref_time.py)
    try:
        src = "r04g_ref_time_1000.json" if os.path.exists(os.path.join(ROOT, "profiles", "r04g_ref_time_1000.json")) else "r03i_ref_time_512.json"
        with open(os.path.join(ROOT, "profiles", src)) as f:
            m = json.load(f)
        out["measured_reference_run"] = {
            "n": m["timed"]["n"], "pairs": m["timed"]["pairs"], "pairs_per_s": m["timed"]["pairs_per_s"], "cores": m["cores"], "cpu": m.get("cpu"),
            "stage_a_s": m["timed"]["stage_a_s"], "relax_2it_s": m["timed"]["relax_2it_s"], "extrapolated": False,
            "extrapolation_formula_error_at_this_size": m["extrapolation_error"],
            "source": "profiles/%s (diag/ref_time.py on an MI355X box: EPYC 9575F, 16-core quota)" % src}
        # beside `value`: how far the extrapolation formula was off where it could be checked against a TIMED run of the same size,
        # and how far this run's live figure is from that timed run's (box to box, core quota to core quota)
        out["extrapolation_error"] = m["extrapolation_error"]
        if m["timed"]["n"] == n_full:
            out["live_vs_timed_run"] = out["value"] / m["timed"]["pairs_per_s"] - 1.0
    except (OSError, ValueError, KeyError):
        pass
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", "--nseqs", dest="n", type=int, default=1000)  # --nseqs/--seqlen: spellings torchrun's parser does not trip over
    ap.add_argument("--len", "--seqlen", dest="len", type=int, default=400)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--fasta", default=None, help="real sequences instead of the synthetic family: first --n records of this FASTA "
                    "(.gz accepted), e.g. tests/golden/rdrp_first1000.fa.gz (first 1000 records of the reference's test_data/rdrp/rdrp.fa)")
    ap.add_argument("--full", action="store_true", help="after the timed region also run the digest self-check, the real-data leg "
                    "and the CPU baseline (a plain run measures the headline figure only)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-parity", action="store_true", help="with --full: skip the digest self-check after the timed region")
    ap.add_argument("--no-real-data", action="store_true", help="with --full: skip the real-data leg (rdrp, first 1000 records) after the synthetic timed region")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed as DIR/<name>.npy "
                    "(one GPU only)")
    a = ap.parse_args()
    if a.steps < 1:
        raise SystemExit("bench.py: --steps must be >= 1")
    if a.dump_outputs and a.gpus != 1:
        raise SystemExit("bench.py: --dump-outputs needs --gpus 1 (a rank of a sharded run holds part of the store)")

    from muscle_amd.hostinfo import pin_openmp_team
    pin_openmp_team()
    import torch
    import torch.distributed as dist
    from muscle_amd._lib import MpcGpu
    from muscle_amd.mpcflat import CONSISTENCY_ITERS, TorchExchange, run_stage
    from muscle_amd.synth import make_family

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch N>1 through torch.distributed.run)" % (a.gpus, world))
    # MPCGPU_BENCH_DRYRUN=<path of tests/emu/libmpcgpu_emu.so>: tests only (tests/test_sharding_gloo.py) — the same
    # control flow on CPU tensors, gloo and the SIMT-emulator build of the library, so the N>1 path of this file is
    # exercised without GPUs. The line it prints carries "dry_run": true and measures nothing.
    dry = os.environ.get("MPCGPU_BENCH_DRYRUN") or None
    if dry:
        device = "cpu"
    else:
        torch.cuda.set_device(local)
        device = "cuda:%d" % local
    exchange = None
    if world > 1:
        if dry:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device(device))
        exchange = TorchExchange(dist, device)

    if a.fasta:
        from muscle_amd.synth import read_fasta
        seqs = read_fasta(a.fasta)[:a.n]
        if len(seqs) < a.n:
            raise SystemExit("bench.py: %s holds only %d records" % (a.fasta, len(seqs)))
        family = "first %d records of %s (real data)" % (a.n, os.path.basename(a.fasta))
    else:
        seqs = make_family(a.n, a.len, seed=a.seed)
        family = "%d synthetic protein seqs L~%d (seed %d)" % (a.n, a.len, a.seed)
    lens = [len(s) for s in seqs]
    npairs = a.n * (a.n - 1) // 2
    g = MpcGpu(0 if dry else local, dry)
    g.set_hmm(*load_hmm())
    g.set_seqs(seqs)  # inputs resident in HBM from here on

    def barrier():
        if not dry:
            torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        if not dry:
            torch.cuda.synchronize()

    for _ in range(a.warmup):
        run_stage(g, lens, exchange, torch_mod=torch)
    g.timers_reset()
    g._exchange_seconds = 0.0
    g._phase = {}  # host seconds per phase of a sharded step (muscle_amd/mpcflat.py: run_stage)
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        run_stage(g, lens, exchange, torch_mod=torch)
    barrier()
    el = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([el], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    timers = g.timers_get()
    if a.dump_outputs:
        dump_outputs(g, a.dump_outputs)
    rc = 0
    # every rank's phases (host seconds between the points where run_stage waits for the device anyway), and how many ranks the
    # collective backend really connected: rank 0 prints the maximum over ranks and the list
    per_rank = None
    if world > 1:
        mine = {k: 1000.0 * v / a.steps for k, v in getattr(g, "_phase", {}).items()}
        mine["kernels"] = {k: v[0] / a.steps for k, v in timers.items() if v[0]}
        mine["rank"], mine["device"] = rank, ("cpu" if dry else torch.cuda.get_device_name(local))
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)

    if rank == 0:
        nnz = g.get_nnz()
        ms_step = 1000.0 * el / a.steps
        # dominant kernel family of THIS rank over the timed steps (hipEvents on the library's stream)
        my_frac = 1.0 / world  # this rank's share of the pair-sharded work
        geo, _fallback = g.relax_info()
        kname = ("relax_band_kernel" if "relax_band_kernel" in geo else "relax_var_kernel" if "relax_var_kernel" in geo
                 else "relax_kernel")
        fixture_shape = (a.n, a.len) if not a.fasta else (a.n, 0)

        CHIP_SIMDS, CHIP_CUS, CLOCK_ASSUMED_HZ = 1024, 256, 2.1e9  # MI355X: 256 CUs x 4 SIMDs; clock only when no counter pass gives one

        def clock_of(pmc):
            """(Hz, where it comes from): the clock the chip sustained under this kernel, from the committed counter pass
            (scripts/pmc_summary.py: SQ_BUSY_CYCLES / 32 shader engines / launch duration of the --kernel-trace --stats pass)."""
            if pmc and pmc.get("clock_hz"):
                return float(pmc["clock_hz"]), pmc.get("clock_method", "counter pass")
            return CLOCK_ASSUMED_HZ, "ASSUMED 2.1 GHz (no counter pass with launch durations for this kernel)"

        def issue_cost_of(kernel, fallback):
            """(mean issue cost of the kernel's VALU mix in full-rate ops, source): muscle_amd/csrc/isa_cost.json, written at build time
            by scripts/isa_cost.py --json from the gfx950 listing of the shipped instantiations (make asm)."""
            try:
                with open(os.path.join(ROOT, "muscle_amd", "csrc", "isa_cost.json")) as f:
                    e = json.load(f)[kernel]
                return float(e["mean_issue_cost"]), "scripts/isa_cost.py over %s of %s (%d VALU instructions)" % (e["region"], e["mangled"], e["valu_instructions"])
            except (OSError, ValueError, KeyError):
                return fallback, "literal %.2f (muscle_amd/csrc/isa_cost.json missing: run __graft_entry__.build())" % fallback

        def issue_fraction(pmc, avg_s, units_per_inst):
            """VALU issue time / launch time from the committed SQ pass: wave-instructions x issue cost (diag/pkbench: a full-rate
            VALU op = 2 cycles per wave on a SIMD; units_per_inst = the mix's mean cost in such ops from scripts/isa_cost.py)
            over 1024 SIMDs at the 2.1 GHz the chip sustains under this load."""
            if not pmc or "sq_per_launch" not in pmc or "SQ_INSTS_VALU" not in pmc["sq_per_launch"]:
                return None
            return pmc["sq_per_launch"]["SQ_INSTS_VALU"] * units_per_inst * 2.0 / (CHIP_SIMDS * clock_of(pmc)[0]) / avg_s

        def lds_fraction(pmc, avg_s):
            """LDS-array cycles (SQ_LDS_IDX_ACTIVE, conflicts included) / cycles of the launch, per CU."""
            if not pmc or "SQ_LDS_IDX_ACTIVE" not in pmc.get("sq_per_launch", {}):
                return None
            return pmc["sq_per_launch"]["SQ_LDS_IDX_ACTIVE"] / (CHIP_CUS * clock_of(pmc)[0]) / avg_s

        def measured_roof(r, pmc, avg_s, kernel_for_cost, cost_fallback, launched_kernel):
            """roofline.bound / frac from MEASURED counters: the binding resource is the one with the largest measured fraction of
            its own roof (HBM bytes per launch / 8 TB/s, VALU issue time / launch time, LDS-array cycles / launch cycles); frac is
            that fraction, always <= 1. Counters are taken only from a committed PMC pass of the SAME kernel instantiation that just
            ran (profiles/pmc_traffic.json records rocprofv3's kernel name; mpcgpu_relax_info reports what was launched)."""
            if pmc is not None and launched_kernel is not None and launched_kernel not in pmc.get("kernel", ""):
                r["pmc_rejected"] = "committed PMC pass is of %r, this run launched %r" % (pmc.get("kernel"), launched_kernel)
                pmc = None
            if pmc is not None and world > 1:
                # the committed counter passes are of the ONE-GPU launch; a rank of `world` launches its share of the tiles / pairs: the
                # counters are scaled by that share (an approximation: the fractions are those of the one-GPU kernel unless the rank's
                # tiles behave differently) and the record says so
                pmc = dict(pmc)
                pmc["hbm_bytes_per_launch"] = float(pmc["hbm_bytes_per_launch"]) * my_frac
                pmc["sq_per_launch"] = {k: v * my_frac for k, v in pmc.get("sq_per_launch", {}).items()}
                r["counters_scaled_from_one_gpu_pass"] = my_frac
            units_per_inst, cost_src = issue_cost_of(kernel_for_cost, cost_fallback)
            r["issue_cost"] = {"mean_valu_issue_cost": units_per_inst, "source": cost_src}
            r["clock"] = dict(zip(("hz", "source"), clock_of(pmc)))
            traffic = None if pmc is None else float(pmc["hbm_bytes_per_launch"])
            fr = {"hbm": None if traffic is None else traffic / avg_s / 1e9 / HBM_PEAK_GBS,
                  "valu_issue": issue_fraction(pmc, avg_s, units_per_inst), "lds": lds_fraction(pmc, avg_s)}
            r["traffic"] = traffic
            r["measured_fractions"] = fr
            known = {k: v for k, v in fr.items() if v is not None}
            # beside `lds` (LDS-array cycles, bank conflicts included — a kernel that wasted more cycles on conflicts would score higher):
            # the same without the conflict cycles; not a candidate for `bound`
            sq = (pmc or {}).get("sq_per_launch", {})
            if fr["lds"] is not None and "SQ_LDS_BANK_CONFLICT" in sq:
                fr["lds_net_of_conflicts"] = (sq["SQ_LDS_IDX_ACTIVE"] - sq["SQ_LDS_BANK_CONFLICT"]) / (CHIP_CUS * clock_of(pmc)[0]) / avg_s
            if known:
                b = max(known, key=known.get)
                r["bound"], r["frac"] = b, known[b]
                if b == "lds" and fr.get("lds_net_of_conflicts") is not None:
                    # the LDS array is the busiest resource — but a third of its cycles are bank conflicts of the look-ups, and a
                    # fraction that RISES when a kernel wastes more cycles cannot be its quality (round-5 review, item 3): frac is the
                    # LDS cycles that did work; the gross figure stays beside it
                    r["frac"], r["frac_gross_with_bank_conflicts"] = fr["lds_net_of_conflicts"], known[b]
                if b == "hbm":
                    r["achieved"], r["peak"], r["unit"] = traffic / avg_s / 1e9, HBM_PEAK_GBS, "GB/s"
                else:
                    r["achieved"], r["peak"], r["unit"] = r["frac"], 1.0, "fraction of %s cycles" % ("VALU issue" if b == "valu_issue" else "LDS array (net of bank conflicts)")
                r["counter_source"] = pmc.get("source")
            else:
                r["bound"], r["frac"], r["achieved"], r["peak"], r["unit"] = None, None, None, None, None
            return r

        n_seqs_ge3 = a.n >= 3

        def relax_roof():
            ms, launches = timers["relax"]
            # per relax ITERATION: real data runs two launches per iteration (the pairs whose records only fit the 160 KB geometry
            # get a second, tiny one — relax_geometry says so); the counters in pmc_traffic.json are those of the dominant launch
            iters = max(a.steps * CONSISTENCY_ITERS, 1) if n_seqs_ge3 else max(launches, 1)
            measured_launches = launches
            launches = iters  # the figures below are per relax ITERATION (relax_band_kernel: one launch each; `launches_measured` says)
            avg_s = ms * 1e-3 / max(launches, 1)
            per_launch = stage_b_bytes(lens, nnz) * my_frac  # one launch = one relax iteration over this rank's pairs
            launched = geo.split("kernel=")[1].split(";")[0].strip() if "kernel=" in geo else None
            si = g.store_info()
            # the least a launch can move: every record of the store read once, the own pairs' {P, col, row} read once, the new values
            # written — against the bytes the launch really moved (traffic) this is the re-read factor of the LDS tiling
            min_bytes = float(si["record_bytes"] + si["window_bytes"] + 12 * si["own_entries"] + 4 * si["own_entries"])
            r = {"kernel": (launched or kname) + " (consistency relax: sampled sparse product over the all-pairs store, LDS-tiled)",
                 "launches": launches, "iterations": iters, "launches_measured": measured_launches, "avg_launch_ms": ms / max(launches, 1),
                 "avg_iteration_ms": ms / max(iters, 1),
                 "min_bytes_per_launch": min_bytes, "min_bytes_rate_GBs": min_bytes / avg_s / 1e9, "min_bytes_frac_of_hbm_peak": min_bytes / avg_s / 1e9 / HBM_PEAK_GBS,
                 "survey_8d_streaming_bytes_per_launch": per_launch, "survey_8d_streaming_rate_GBs": per_launch / avg_s / 1e9,
                 "note": "bound / frac: the resource with the largest MEASURED fraction of its roof (see measured_fractions): HBM = "
                         "(2*FETCH_SIZE + WRITE_SIZE) KiB per launch from separate rocprofv3 --pmc passes / launch time / 8 TB/s "
                         "(MI355X_MICROARCH.md HBM section); valu_issue = SQ_INSTS_VALU x mean issue cost (issue_cost) x 2 cycles / (1024 SIMDs x clock) "
                         "/ launch time; lds = SQ_LDS_IDX_ACTIVE / (256 CUs x clock) / launch time; clock: see `clock` (derived from counters). Launch time: hipEvents on the "
                         "library's stream (profiles/*kernel_stats*.csv agrees). survey_8d_streaming_rate_GBs = SURVEY.md 8d stage-B bytes "
                         "(survey_8d_streaming_*: every (pair,Z) reads both operand matrices once: sum of 8*(nnz_XZ+nnz_YZ)+4*(LX+LY+2), + 4*nnz written) / "
                         "launch time: a progress figure, NOT a fraction of a roof and NOT a lower bound (the LDS tiling serves up to 64 pairs' row bands from 16 "
                         "partial records, so far fewer bytes cross the fabric: it exceeds 8 TB/s). min_bytes_per_launch = the store read once + the own "
                         "pairs' entries + the values written: the real lower bound; traffic_over_min_bytes = measured HBM bytes / that = how often the "
                         "tiling re-reads the store. frac: the binding resource's fraction; for the LDS array NET of bank-conflict cycles "
                         "(frac_gross_with_bank_conflicts beside it). null = no committed PMC pass for this workload and this kernel."}
            cost_key = kname + "/MpcRbBlocksAsm" if kname == "relax_band_kernel" and launched and "MpcRbBlocks" in launched else kname
            r = measured_roof(r, pmc_entry(cost_key, *fixture_shape) or pmc_entry(kname, *fixture_shape), avg_s, cost_key, 1.20, launched)
            r["traffic_over_min_bytes"] = None if r.get("traffic") is None else r["traffic"] / min_bytes
            return r

        def fb_roof():
            ms, launches = timers["fb"]
            avg_s = ms * 1e-3 / max(launches, 1)
            per_launch = stage_a_flops(lens) * my_frac * a.steps / max(launches, 1)  # all pairs of this rank per step, over launches/steps batches
            achieved = per_launch / avg_s / 1e12
            sa_pairs, sa_chained, sa_chains = g.stage_a_info()
            chained = sa_chained > 0
            fb_name = "fb_chain_kernel" if chained else "fb_kernel"
            r = {"kernel": ("fb_chain_kernel<H> (pair-HMM fwd+bwd+posterior threshold; one wave sweeps a chain of pairs that share their row "
                            "sequence, no systolic fill/drain in between: %d of %d pairs in %d chains of 2..16)" % (sa_chained, sa_pairs, sa_chains))
                           if chained else "fb_kernel<H> (pair-HMM fwd+bwd+posterior threshold, one wave per pair)",
                 "launches": launches, "avg_launch_ms": ms / max(launches, 1),
                 "algorithmic_TFLOPs": achieved, "frac_of_fp32_vector_peak": achieved / FP32_PEAK_TFLOPS, "no_fma_add_mul_peak_TFLOPs": 63.0,
                 "note": "FP32 vector-ALU bound log-space recurrence: no contraction (parity), no MFMA shape. bound / frac as for the relax "
                         "kernel (measured fractions; valu_issue = how much of the launch the VALU is issuing). algorithmic_TFLOPs = sum over "
                         "the launch's pairs of 164(LX+1)(LY+1)+5LXLY flop (SURVEY.md 8d) / launch time; frac_of_fp32_vector_peak is against "
                         "157.3 TFLOP/s, which counts v_pk_fma_f32 — measured on this chip (diag/pkbench, profiles/r02b_pkbench.log) plain "
                         "add/mul issue at 63 Tlane-op/s and min/max/cvt/select at 0.6 of that, so 63 TFLOP/s is the ceiling of an FMA-free stream."}
            return measured_roof(r, pmc_entry(fb_name, *fixture_shape), avg_s, fb_name, 1.18, fb_name)

        roof = relax_roof() if timers["relax"][0] >= timers["fb"][0] else fb_roof()
        roof_other = fb_roof() if timers["relax"][0] >= timers["fb"][0] else relax_roof()
        out = {
            "metric": "sequence-pairs/sec (fwd+bwd+posterior+relax)", "value": npairs * a.steps / el, "unit": "pairs/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms_step, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "real (rdrp)" if a.fasta else "synthetic",
            "config": {"workload": "MPCFlat posterior stage: %s, %d pairs, "
                                   "fwd+bwd+posterior+sparsify+EA + 2 relax iterations" % (family, npairs),
                       "n_seqs": a.n, "mean_len": float(np.mean(lens)), "pairs": npairs,
                       "stored_posteriors": int(nnz.sum()), "parallelism": "pair-shard x%d" % world},
            "kernel_ms_per_step": {k: v[0] / a.steps for k, v in timers.items()},
            # host time of rank 0 inside the two exchanges of a step (all-gather of the packed shards, all-gather of the values per
            # relax iteration), waits included; 0 on one GPU
            "exchange_ms": 1000.0 * getattr(g, "_exchange_seconds", 0.0) / a.steps,
            "relax_geometry": dict(zip(("layout", "fallback"), g.relax_info())),
            "roofline": roof,
            "roofline_stage_a" if roof["kernel"].startswith("relax") else "roofline_relax": roof_other,
        }
        if world > 1:
            from muscle_amd.mpcflat import PIECES, plan
            rects, pos, px, py = plan(g, lens, world)
            phases = sorted({k for pr in per_rank for k in pr if k not in ("kernels", "rank", "device")})
            out["multi_gpu"] = {
                "backend": dist.get_backend(), "rccl_ranks": dist.get_world_size(), "transport": "gloo (dry run)" if dry else "RCCL point-to-point (torch.distributed nccl backend), one process per GPU",
                "partition": ("%d blocks of the pair triangle (mpcgpu_plan_partition), a rank's store holds the matrices of its blocks' sequences" % len(rects))
                             if len(rects) else "contiguous InitPairs ranges",
                "stage_a_pieces": str(os.environ.get("MPC_PIECES", PIECES)),
                "pairs_per_rank": [int(pos[r + 1] - pos[r]) for r in range(world)],
                "sequences_held_per_rank": [int(len(set(px[pos[r]:pos[r + 1]].tolist()) | set(py[pos[r]:pos[r + 1]].tolist()))) for r in range(world)],
                "phase_ms_max_over_ranks": {k: max(pr.get(k, 0.0) for pr in per_rank) for k in phases},
                "phase_ms_per_rank": [{k: round(pr.get(k, 0.0), 3) for k in phases} for pr in per_rank],
                "kernel_ms_per_rank": [pr["kernels"] for pr in per_rank],
                "devices": [pr["device"] for pr in per_rank],
                "note": "phase_ms: host wall time of rank r between the points where a step waits for the device anyway (stage_a: its pieces; "
                        "exchange_shards: size exchange, copy of the own piece, and what of the all-gather is NOT hidden under the next piece; "
                        "import_store; relax: kernel + the copy of the own slice; exchange_values: all-gather of the values with the own slice's "
                        "commit under it; commit: the other ranks' slices)"}
        if dry:
            out["dry_run"] = True
        elif a.full and not a.no_parity:
            out["parity_digest"], out["parity_detail"] = parity_check(g, a)
        # the realistic input, after the synthetic timed region and its self-check (one GPU, the default workload only)
        if a.full and world == 1 and not dry and not a.fasta and not a.no_real_data and a.n == 1000 and a.len == 400:
            try:
                out["real_data"] = real_data_leg(g, torch, run_stage)
            except Exception as e:  # noqa: BLE001 - the headline line must still be printed
                out["real_data"] = {"error": "%s: %s" % (type(e).__name__, e)}
        if a.full and world == 1 and not a.no_cpu_baseline and not dry:
            out["cpu_baseline"] = cpu_baseline(seqs, a.n)
        print(json.dumps(out), flush=True)
        if out.get("parity_digest") == "MISMATCH" or (out.get("real_data") or {}).get("parity_sample") == "MISMATCH":
            rc = 3  # a fast wrong answer is not a result
    g.close()
    if world > 1:
        dist.destroy_process_group()
    if rc:
        raise SystemExit(rc)


if __name__ == "__main__":
    main()
