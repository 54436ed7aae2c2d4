"""Nodes like this node, with the co-assignment counts: sample partitions of the shipped 1000-node data set with 64 chains and
ask, for a few nodes of either type, which 20 nodes of the SAME type share their block most often.  A query's candidates are
ALL nodes of its own type; a candidate's probability is the fraction of (sample, chain) pairs in which it sits in the query's
block -- one row of the consensus matrix, which never depends on how a chain numbers its blocks, so the 64 chains pool without
any alignment -- and the ranking, the query itself left out, is made on the device (include/bisbm.h, "Co-assignment")."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bisbm = importlib.import_module("bipartitesbm-mcmc_amd")

K = 20
a, b = bisbm.load_edge_list(os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist"))
na = nb = 500
adj = bisbm.edge_to_adj((a, b), na + nb)
start = np.concatenate([np.arange(na) * 4 // na, 4 + np.arange(nb) * 6 // nb])
model = bisbm.BlockModel(start, [0] * na + [1] * nb, 10, 4, 6, 1.0, adj, n_chains=64, rng="philox", seed=1)
model.shuffle_bisbm()
queries = np.array([3, 260, 499, na + 3, na + 260, na + 499])
# burn-in 200 sweeps, 20 samples 5 sweeps apart; every sample counts, in every chain, the nodes that share each query's block
_, _, (nodes, prob, terms) = bisbm.marginalize(model, 200, 20, 5, similar=(queries, K))

print("%d queries, %d chain terms per count (64 chains x 20 samples)" % (len(queries), terms))
for i, q in enumerate(queries):
    row, _ = model.coassignment(i)
    often = int((row >= 0.5 * terms).sum()) - 1
    print("%d nodes share the block of node %d in at least half of the samples; the closest: %s"
          % (often, q, " ".join("%d (%.3f)" % (n, p) for n, p in zip(nodes[i][:5], prob[i][:5]))))
    assert row[q - (0 if q < na else na)] == terms and q not in nodes[i]
    assert ((nodes[i] < na) == (q < na)).all() and (np.diff(prob[i]) <= 0).all() and prob[i].max() <= 1.0
assert terms == 64 * 20
