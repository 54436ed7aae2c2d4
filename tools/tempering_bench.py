"""Cost of replica exchange (include/bisbm.h, "Replica exchange") at BASELINE configs[2] -- N = 10^6 (5e5 + 5e5), E = 10^7,
32 + 32 blocks, 1024 chains -- with ensembles of L = 8 and an exchange round after every sweep.  Writes
profiles/tempering_bench.json and prints it:
  * the per-chain temperature path against the constant one: the same chains (a ladder of ones is T = 1 for every chain) run
    through run_sweeps and through tempering_run(s, 0), kernel ms per sweep (bisbm_last_sweep_timing) and host ms per sweep,
    alternated;
  * ms per exchange round: host time of tempering_run(s, 1) minus tempering_run(s, 0) over the same number of sweeps, per round
    (the entropy kernel when it runs, the exchange kernel, one more sweep call per round) -- against a sweep's time;
  * swap acceptance per rung pair on a geometric ladder 1 .. 2 after a burn-in.

    python tools/tempering_bench.py [--quick] [--chains 1024] [--sweeps 6]"""
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


def timed(m, fn, sweeps):
    t0 = time.perf_counter()
    fn(sweeps)
    wall = (time.perf_counter() - t0) * 1e3
    return wall / sweeps, m.last_sweep_timing()[0] / sweeps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a 10^5-node graph instead of configs[2] (a first look)")
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--sweeps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tempering_bench.json"))
    args = ap.parse_args()
    na = nb = 50_000 if args.quick else 500_000
    E, k, L, s = 20 * na, 32, 8, args.sweeps
    a, b = syn.planted_edges(na, nb, E, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), na + nb)
    m = B.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k, 1.0, (rp, cl), n_chains=args.chains, seed=1)
    m.shuffle_bisbm()
    m.run_sweeps(2)  # (warm-up: first launches, the pass-depth policy's first look)
    out = {"n": na + nb, "edges": E, "blocks": "%d+%d" % (k, k), "chains": args.chains, "L": L, "exchange_every": 1, "sweeps": s}

    def tempered(every):
        return lambda n: m.tempering_run(n, every)

    plain, ones = [], []
    for _ in range(2):  # alternated: the chain moves on between the measurements, both paths see the same regime
        m.set_tempering(None)
        plain.append(timed(m, m.run_sweeps, s))
        m.set_tempering([1.0] * L)
        ones.append(timed(m, tempered(0), s))
    out["plain_ms_per_sweep"] = [float(np.mean([x[0] for x in plain])), float(np.mean([x[1] for x in plain]))]
    out["ones_ms_per_sweep"] = [float(np.mean([x[0] for x in ones])), float(np.mean([x[1] for x in ones]))]
    out["per_chain_T_kernel_ratio"] = out["ones_ms_per_sweep"][1] / out["plain_ms_per_sweep"][1]
    # exchange rounds: the same ladder of ones, every sweep followed by a round
    ex0 = timed(m, tempered(0), s)
    ex1 = timed(m, tempered(1), s)
    out["host_ms_per_sweep_without_rounds"] = ex0[0]
    out["host_ms_per_sweep_with_rounds"] = ex1[0]
    out["ms_per_exchange_round"] = ex1[0] - ex0[0]
    out["exchange_round_fraction_of_sweep"] = out["ms_per_exchange_round"] / ex0[0]
    # acceptance on a realistic ladder
    ladder = [float(x) for x in np.geomspace(1.0, 2.0, L)]
    m.set_tempering(ladder)
    m.tempering_run(2 * s, 1)
    att, acc, rounds = m.tempering_stats()
    out["ladder"] = ladder
    out["rounds"] = int(rounds)
    out["swap_acceptance"] = [float(x) / float(y) if y else None for x, y in zip(acc, att)]
    m.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
