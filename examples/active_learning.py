"""Active learning with held conditionals: on the shipped 1000-node data set a few nodes' planted labels are known at the start,
64 chains sample with those nodes clamped, and every round asks which nodes are the least settled under what is held -- the
held conditionals of all nodes (conditionals_held), ranked on the device (least_settled) -- has their labels revealed and
clamps them too.  Beside it the same budget spent on seeded random picks.  Printed per round: the share of all nodes whose
pooled MAP label (the unaligned histogram: the clamped seeds pin the numbering) is the planted one.  Whether uncertainty picks
beat random ones here is reported, not asserted."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bisbm = importlib.import_module("bipartitesbm-mcmc_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--per_round", type=int, default=40, help="labels revealed per round")
ap.add_argument("--sweeps", type=int, default=10, help="sweeps before each of the 3 samples of a round")
args = ap.parse_args()

edges = bisbm.load_edge_list(os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist"))
na = nb = 500
n = na + nb
adj = bisbm.edge_to_adj(edges, n)
types = [0] * na + [1] * nb
planted = np.array(np.repeat(np.arange(4), 125).tolist() + (4 + np.repeat(np.arange(6), [84, 84, 83, 83, 83, 83])).tolist(), dtype=np.uint32)
seeds = np.arange(0, n, 25)  # known at the start: 40 nodes, every block among them


def run(pick):
    """pick(model, known mask, k) -> k nodes to reveal; returns the agreement with the planted partition after every round"""
    model = bisbm.BlockModel(planted, types, 10, 4, 6, 1.0, adj, n_chains=64, rng="philox", seed=1)
    known = np.zeros(n, dtype=bool)
    known[seeds] = True
    model.clamp(known)       # held at the labels the chains have now: the planted ones
    model.shuffle_bisbm()    # the open nodes' labels are permuted among themselves
    agreement = []
    for _ in range(args.rounds):
        # three samples: the label histogram, and the held conditionals of all nodes under the clamp as it is now
        labels = bisbm.marginalize(model, args.sweeps, 3, args.sweeps, conditionals=(None, 1.0), conditionals_held=True)[0]
        agreement.append(float((labels == planted).mean()))
        reveal = pick(model, known, args.per_round)
        # a revealed label is set in every chain, then held: the clamp takes the labels the chains have at the call
        for c in range(model.n_chains):
            lab = model.get_memberships(c)
            lab[reveal] = planted[reveal]
            model.set_memberships(lab, chain=c)
        model.init_bisbm()
        known[reveal] = True
        model.clamp(known)
    model.close()
    return agreement


def by_uncertainty(model, known, k):
    idx, nodes, values, terms = model.least_settled(k, "entropy")  # (a clamped node's entropy is 0.0: it is never among them)
    nodes = nodes[values > 0.0]
    spare = np.flatnonzero(~known)
    spare = spare[~np.isin(spare, nodes)]
    return np.concatenate([nodes, spare[:k - len(nodes)]]).astype(np.int64)  # (every open node settled: any open ones)


rng = np.random.default_rng(7)


def at_random(model, known, k):
    return rng.choice(np.flatnonzero(~known), k, replace=False)


a, b = run(by_uncertainty), run(at_random)
print("%d nodes known at the start, %d revealed per round, 64 chains; share of nodes whose pooled MAP label is the planted one" % (len(seeds), args.per_round))
print("round  known  uncertainty  random")
for i, (x, y) in enumerate(zip(a, b)):
    print("%5d  %5d  %11.3f  %6.3f" % (i, len(seeds) + i * args.per_round, x, y))
