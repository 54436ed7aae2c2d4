"""Cost of the edge probabilities (include/bisbm.h, "Edge probabilities") on the bench graph of tools/pair_scores_bench.py --
N = 10^6 (5e5 + 5e5), E = 10^7, 32 + 32 blocks, 1024 chains -- for one sample of P = 10^6 ADD pairs, beside one
pair_scores_accumulate on the same pairs in the same process, alternated, 15 repeats each (a warm-up round first, dropped).
Host clock around each call, which returns after its kernels have finished.  Writes profiles/edge_probs_bench.json and prints
it: the medians, their ratio and ns per (pair, chain).

    python tools/edge_probs_bench.py [--quick] [--chains 1024] [--pairs 1000000] [--reps 15]"""
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


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a 10^5-node graph instead of the bench graph (a first look)")
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_probs_bench.json"))
    args = ap.parse_args()
    na = nb = 50_000 if args.quick else 500_000
    E, k, C, P = 20 * na, 32, args.chains, args.pairs
    a, b = syn.planted_edges(na, nb, E, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), na + nb)
    m = B.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k, 1.0, (rp, cl), n_chains=C, seed=1)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    rs = np.random.default_rng(5)
    pairs = np.stack([rs.integers(0, na, P), na + rs.integers(0, nb, P)], axis=1)
    out = {"n": na + nb, "edges": E, "blocks": "%d+%d" % (k, k), "chains": C, "pairs": P, "reps": args.reps, "kind": "ADD"}
    out["edge_probs_set_ms"] = ms(lambda: m.edge_probs_set(pairs))
    out["pair_scores_set_ms"] = ms(lambda: m.pair_scores_set(pairs))
    edge, pair = [], []
    for rep in range(args.reps + 1):  # (alternated; the first round is the warm-up and is dropped)
        t_edge = ms(m.edge_probs_accumulate)
        t_pair = ms(m.pair_scores_accumulate)
        if rep:
            edge.append(t_edge)
            pair.append(t_pair)
    out["edge_probs_accumulate_ms_all"], out["pair_scores_accumulate_ms_all"] = edge, pair
    out["edge_probs_accumulate_ms"] = float(np.median(edge))
    out["pair_scores_accumulate_ms"] = float(np.median(pair))
    out["edge_over_pair"] = out["edge_probs_accumulate_ms"] / out["pair_scores_accumulate_ms"]
    out["edge_ns_per_pair_chain"] = out["edge_probs_accumulate_ms"] * 1e6 / (P * C)
    out["pair_ns_per_pair_chain"] = out["pair_scores_accumulate_ms"] * 1e6 / (P * C)
    r = m.edge_probs()
    out["terms"] = int(r["terms"])
    out["all_finite"] = bool(np.isfinite(r["dS_sum"]).all() and np.isfinite(r["log_prob"]).all())
    m.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
