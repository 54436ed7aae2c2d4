"""Time of one mode-resolved marginal sample (include/bisbm.h, "Mode-resolved marginals") at BASELINE configs[2] -- N = 10^6
(5e5 + 5e5), E = 10^7, 32 + 32 blocks, 1024 chains -- with the chains split evenly (chain c -> mode c mod M) into M = 1, 4 and 32
modes, beside the yardstick: one pooled aligned bisbm_marginals_accumulate of the same handle (what tools/align_bench.py
times as aligned_ms_default).  A split into modes reads the same label bytes and solves the same assignments.  The chains sit
on the planted partition, each in its own random numbering, after two sweeps, as in tools/align_bench.py.  The four
configurations are timed in turn, `--rounds` times over, so that a drift of the machine shows in every figure alike.  Prints
one JSON line: per figure the median, the least and the largest of all its repetitions in ms (host clock around the call,
which ends in a device synchronise).
Per-kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/mode_marginals_bench.py --reps 2`.

    python tools/mode_marginals_bench.py [--chains 1024] [--rounds 3] [--reps 10] [--modes 1 4 32]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = importlib.import_module("bipartitesbm-mcmc_amd")
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")


def timed(fn, reps):
    fn()  # warm-up (first launches, buffers allocated on the first sample)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def summary(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--modes", type=int, nargs="+", default=[1, 4, 32])
    ap.add_argument("--n", type=int, default=1_000_000, help="nodes (half of each type)")
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--blocks", type=int, default=32, help="blocks per type")
    args = ap.parse_args()
    na = nb = args.n // 2
    k, chains = args.blocks, args.chains
    a, b = syn.planted_edges(na, nb, args.edges, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), na + nb)
    truth = syn.contiguous_labels(na, nb, k, k)
    m = B.BlockModel(truth, syn.types_vector(na, nb), 2 * k, k, k, 1.0, (rp, cl), n_chains=chains, seed=1)
    st = np.random.default_rng(0)
    for c in range(chains):
        perm = np.concatenate([st.permutation(k), k + st.permutation(k)]).astype(np.uint32)
        m.set_memberships(perm[truth], chain=c)
    m.init_bisbm()
    m.run_sweeps(2)
    out = {"tool": "mode_marginals_bench", "shape": "%d+%d" % (k, k), "n": na + nb, "edges": args.edges, "chains": chains,
           "rounds": args.rounds, "reps": args.reps, "label_bytes_per_sample": chains * (na + nb)}
    times = {}
    for _ in range(args.rounds):
        m.marginals_reset()
        m.marginals_set_modes(None)
        m.marginals_set_alignment(True)
        times.setdefault("aligned_pooled_ms", []).extend(timed(m.marginals_accumulate, args.reps))
        for M in args.modes:
            m.marginals_reset()
            m.marginals_set_modes(np.arange(chains, dtype=np.uint32) % M, n_modes=M)
            times.setdefault("modes_%d_ms" % M, []).extend(timed(m.marginals_accumulate, args.reps))
            assert m.marginals_modes()["terms"].sum() == (args.reps + 1) * chains
    out.update({k: summary(t) for k, t in times.items()})
    m.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
