"""Time of one anchored-mode marginal sample (include/bisbm.h, "Anchored modes") and of bisbm_partition_distances_to at BASELINE
configs[2] -- N = 10^6 (5e5 + 5e5), E = 10^7, 32 + 32 blocks, 1024 chains -- beside their yardsticks measured in the same
process: the static-mode sample with the chains split evenly into M = 1, 4 and 32 modes (tools/mode_marginals_bench.py) for the
anchored sample with M anchors, and the all-pairs bisbm_partition_distances of the same chains, per (pair * node), for the
rectangular call of 1024 chains x 4 and x 32 references.  The chains sit on the planted partition, each in its own random
numbering, after two sweeps; anchor g is the labels of chain g, the threshold is +inf, so every chain is counted.  The
configurations are timed in turn, `--rounds` times over, so that a drift of the machine shows in every figure alike.  Prints one
JSON line: per figure the median, the least and the largest of all its repetitions in ms (host clock around the call, which
ends in a device synchronise), the picoseconds per (pair * node) of both distance calls and their ratio.

    python tools/anchored_modes_bench.py [--chains 1024] [--rounds 3] [--reps 10] [--modes 1 4 32] [--refs 4 32]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
B = importlib.import_module("bipartitesbm-mcmc_amd")
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")
from mode_marginals_bench import summary, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--modes", type=int, nargs="+", default=[1, 4, 32])
    ap.add_argument("--refs", type=int, nargs="+", default=[4, 32])
    ap.add_argument("--square_reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=1_000_000, help="nodes (half of each type)")
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--blocks", type=int, default=32, help="blocks per type")
    args = ap.parse_args()
    na = nb = args.n // 2
    n = na + nb
    k, chains = args.blocks, args.chains
    a, b = syn.planted_edges(na, nb, args.edges, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), n)
    truth = syn.contiguous_labels(na, nb, k, k)
    m = B.BlockModel(truth, syn.types_vector(na, nb), 2 * k, k, k, 1.0, (rp, cl), n_chains=chains, seed=1)
    st = np.random.default_rng(0)
    for c in range(chains):
        perm = np.concatenate([st.permutation(k), k + st.permutation(k)]).astype(np.uint32)
        m.set_memberships(perm[truth], chain=c)
    m.init_bisbm()
    m.run_sweeps(2)
    most = max(max(args.modes), max(args.refs))
    rows = np.array([m.get_memberships(c) for c in range(most)], dtype=np.uint32)
    out = {"tool": "anchored_modes_bench", "shape": "%d+%d" % (k, k), "n": n, "edges": args.edges, "chains": chains,
           "rounds": args.rounds, "reps": args.reps, "label_bytes_per_sample": chains * n}
    times, split = {}, {}
    for _ in range(args.rounds):
        for M in args.modes:
            m.marginals_reset()
            m.marginals_set_modes(np.arange(chains, dtype=np.uint32) % M, n_modes=M)
            times.setdefault("static_%d_ms" % M, []).extend(timed(m.marginals_accumulate, args.reps))
            m.marginals_reset()
            m.marginals_set_mode_anchors(rows[:M], float("inf"))
            times.setdefault("anchored_%d_ms" % M, []).extend(timed(m.marginals_accumulate, args.reps))
            state = m.marginals_modes()
            assert state["terms"].sum() == (args.reps + 1) * chains and state["unassigned"] == 0
            split[M] = np.bincount(state["mode_of_chain"], minlength=M).tolist()
        for R in args.refs:
            times.setdefault("distances_to_%d_ms" % R, []).extend(timed(lambda: m.partition_distances_to(rows[:R]), args.reps))
        times.setdefault("distances_square_ms", []).extend(timed(m.partition_distances, args.square_reps))
    m.marginals_reset()
    m.marginals_set_mode_anchors(None, 0.0)
    out.update({key: summary(t) for key, t in times.items()})
    out["anchored_split"] = {str(M): s for M, s in split.items()}
    square_ps = out["distances_square_ms"]["median"] * 1e9 / (chains * (chains - 1) / 2 * n)
    out["square_ps_per_pair_node"] = square_ps
    for R in args.refs:
        ps = out["distances_to_%d_ms" % R]["median"] * 1e9 / (chains * R * n)
        out["to_%d_ps_per_pair_node" % R] = ps
        out["to_%d_over_square" % R] = ps / square_ps
    m.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
