"""Time of bisbm_partition_distances (include/bisbm.h, "Partition distances and posterior modes") at BASELINE configs[2] -- N = 10^6
(5e5 + 5e5), E = 10^7, 32 + 32 blocks -- over 128 and 1024 chains (the first 128 of the same handle), in two states:
  planted   every chain on the planted partition in its own random numbering, after two sweeps: near-identical partitions, whole
            waves of the counting kernel land on one diagonal cell (the conflict-heavy case);
  shuffled  after shuffle_bisbm(): the cells are spread.
Prints one JSON line per (state, chains): median and min ms of `--reps` calls (host clock around the call, which returns after its
kernels and the copy of the results), ps per (pair . node), and the call in sweeps of the same handle (ms of one run_sweeps(1)).
--comparator adds two aligned marginal samples on the planted state, so that a run under
`rocprofv3 --kernel-trace --stats -- python tools/partition_distance_bench.py --quick --comparator` holds align_overlap_kernel (the
existing kernel for the same per-node work, per chain . node) beside partition_count_kernel (per pair . node) in one trace.

    python tools/partition_distance_bench.py [--quick] [--comparator] [--chains 128,1024] [--reps 5]"""
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
    fn()  # warm-up (first launches, scratch allocated on the first call)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="two calls per case (profiler runs)")
    ap.add_argument("--comparator", action="store_true", help="also two aligned marginal samples on the planted state")
    ap.add_argument("--chains", default="128,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=32)
    args = ap.parse_args()
    reps = 2 if args.quick else args.reps
    counts = sorted(int(x) for x in args.chains.split(","))
    na = nb = args.nodes // 2
    k, n, total = args.k, 2 * (args.nodes // 2), counts[-1]
    a, b = syn.planted_edges(na, nb, args.edges, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), n)
    truth = syn.contiguous_labels(na, nb, k, k)
    m = B.BlockModel(truth, syn.types_vector(na, nb), 2 * k, k, k, 1.0, (rp, cl), n_chains=total, seed=1)
    st = np.random.default_rng(0)
    for c in range(total):
        perm = np.concatenate([st.permutation(k), k + st.permutation(k)]).astype(np.uint32)
        m.set_memberships(perm[truth], chain=c)
    m.init_bisbm()
    m.run_sweeps(2)
    for state in ("planted", "shuffled"):
        if state == "shuffled":
            m.shuffle_bisbm()
        sweep_ms = float(np.median(timed(lambda: m.run_sweeps(1), 2))) if not args.quick else None
        for chains in counts:
            sel = np.arange(chains, dtype=np.uint32)
            t = timed(lambda: m.partition_distances(sel), reps)
            vi, H = m.partition_distances(sel)
            pairs = chains * (chains - 1) // 2
            med = float(np.median(t))
            out = {"state": state, "shape": "%d+%d" % (k, k), "n": n, "edges": args.edges, "chains": chains, "pairs": pairs,
                   "reps": reps, "ms_median": med, "ms_min": float(min(t)), "ms_all": [round(x, 3) for x in t],
                   "ps_per_pair_node": med * 1e9 / (pairs * n), "vi_mean": float(vi[np.triu_indices(chains, 1)].mean()),
                   "H_mean": float(H.mean())}
            if sweep_ms is not None:
                out["sweep_ms_%d_chains" % total] = sweep_ms
                out["call_in_sweeps"] = med / sweep_ms
            print(json.dumps(out), flush=True)
        if state == "planted" and args.comparator:
            m.marginals_reset()
            m.marginals_set_alignment(True)
            t = timed(m.marginals_accumulate, 2)
            print(json.dumps({"state": state, "comparator": "aligned bisbm_marginals_accumulate", "chains": total, "ms_median": float(np.median(t)),
                              "note": "its align_overlap_kernel time per (chain . node) is read from the kernel trace"}), flush=True)
            m.marginals_reset()
            m.marginals_set_alignment(False)
    m.close()


if __name__ == "__main__":
    main()
