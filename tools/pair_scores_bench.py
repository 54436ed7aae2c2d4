"""Cost of the pair scores (include/bisbm.h, "Posterior-predictive pair scores") at BASELINE configs[2] -- N = 10^6 (5e5 + 5e5),
E = 10^7, 32 + 32 blocks, 1024 chains -- for P = 10^6 random pairs.  Writes profiles/pair_scores_bench.json and prints it:
  * ms of one pair_scores_accumulate (host clock around the call, which returns after its kernels have finished) and pair-chain
    terms per second, against ms of one sweep of the same handle, alternated in one process: the bar is accumulate <= sweep;
    (what the sort of the pairs and the slab-per-XCD order of the workgroups are worth was measured with the two switches of
    profiles/pair_scores_ab_switches.diff applied: profiles/pair_scores_ab.json);
  * the host route a user had before: get_memberships / get_m / get_m_r + numpy_pair_scores, timed on 8 chains and SCALED to
    the chain count (said so in the file).

    python tools/pair_scores_bench.py [--quick] [--chains 1024] [--pairs 1000000] [--reps 3]"""
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
    ap.add_argument("--quick", action="store_true", help="a 10^5-node graph instead of configs[2] (a first look)")
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_scores_bench.json"))
    args = ap.parse_args()
    na = nb = 50_000 if args.quick else 500_000
    E, k, C, P = 20 * na, 32, args.chains, args.pairs
    a, b = syn.planted_edges(na, nb, E, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), na + nb)
    deg = np.diff(rp.astype(np.int64))
    m = B.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k, 1.0, (rp, cl), n_chains=C, seed=1)
    m.shuffle_bisbm()
    m.run_sweeps(2)  # (warm-up: first launches, the pass-depth policy's first look)
    rs = np.random.default_rng(5)
    pairs = np.stack([rs.integers(0, na, P), na + rs.integers(0, nb, P)], axis=1)
    out = {"n": na + nb, "edges": E, "blocks": "%d+%d" % (k, k), "chains": C, "pairs": P, "reps": args.reps}

    m.pair_scores_set(pairs)
    times, sweeps = [], []
    for rep in range(args.reps + 1):  # (alternated; the first round is the warm-up and is dropped)
        t_acc = ms(m.pair_scores_accumulate)
        t_sweep = ms(lambda: m.run_sweeps(1))
        if rep:
            times.append(t_acc)
            sweeps.append(t_sweep)
    out["sweep_ms"] = sweeps
    out["accumulate_ms_all"] = times
    acc = float(np.median(times))
    out["accumulate_ms"] = acc
    out["sweep_ms_median"] = float(np.median(sweeps))
    out["accumulate_over_sweep"] = acc / out["sweep_ms_median"]
    out["meets_bar_accumulate_le_sweep"] = bool(acc <= out["sweep_ms_median"])
    out["pair_chain_terms_per_s"] = P * C / (acc * 1e-3)
    out["terms"] = int(m.pair_scores()[1])

    # the host route: labels and block state of every chain to the host, the arithmetic in numpy
    hc = min(8, C)
    t0 = time.perf_counter()
    labs = [m.get_memberships(c) for c in range(hc)]
    ms_ = [m.get_m(c) for c in range(hc)]
    mrs = [m.get_m_r(c) for c in range(hc)]
    t1 = time.perf_counter()
    B.numpy_pair_scores(labs, ms_, mrs, deg, pairs)
    t2 = time.perf_counter()
    out["host_route"] = {"timed_chains": hc, "getters_ms": (t1 - t0) * 1e3, "numpy_ms": (t2 - t1) * 1e3,
                         "scaled_to_all_chains_ms": (t2 - t0) * 1e3 * C / hc, "note": "timed on %d chains, scaled linearly to %d" % (hc, C)}
    out["host_route_over_accumulate"] = out["host_route"]["scaled_to_all_chains_ms"] / acc
    # (a check on the way: the first chains' terms through the device equal numpy's)
    one = B.BlockModel(labs[0], syn.types_vector(na, nb), 2 * k, k, k, 1.0, (rp, cl), n_chains=1, seed=1)
    one.init_bisbm()
    one.pair_scores_set(pairs[:100_000])
    one.pair_scores_accumulate()
    out["one_chain_bit_equal_to_numpy"] = bool((one.pair_scores()[0] == B.numpy_pair_scores(labs[:1], ms_[:1], mrs[:1], deg, pairs[:100_000])).all())
    one.close()
    m.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
