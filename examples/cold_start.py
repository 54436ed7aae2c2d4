"""Recommendations for a node that is not in the graph, with the fold-in queries: hold 25 type-a nodes of the shipped 1000-node
data set OUT of the graph altogether, fit the rest with 64 chains, and hand each held-out node back as a virtual node that
names only 5 of its neighbours.  Every chain gives the virtual node a posterior over its blocks -- the naive-Bayes rule the
engine draws its proposals with, applied to the neighbours' labels --, from it an expected edge count to every node of the
other type and a probability of sharing a block with every node of its own type; neither depends on how a chain numbers its
blocks, so the 64 chains pool without any alignment, and the ranking is made on the device (include/bisbm.h, "Fold-in
queries").  Printed at the end: how many of the neighbours the virtual nodes did NOT name are among their recommendations,
beside what a random choice of as many candidates would find."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bisbm = importlib.import_module("bipartitesbm-mcmc_amd")

K, SHOWN = 50, 5
a, b = bisbm.load_edge_list(os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist"))
na = nb = 500
a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
deg = np.bincount(a, minlength=na)
held = np.flatnonzero(deg >= 2 * SHOWN)[::7][:25]                        # the new nodes: they keep no edge in the fitted graph
keep = ~np.isin(a, held)
adj = bisbm.edge_to_adj((a[keep].astype(np.uint64), b[keep].astype(np.uint64)), na + nb)
start = np.concatenate([np.arange(na) * 4 // na, 4 + np.arange(nb) * 6 // nb])
model = bisbm.BlockModel(start, [0] * na + [1] * nb, 10, 4, 6, 1.0, adj, n_chains=64, rng="philox", seed=1)
model.shuffle_bisbm()
nodes, hidden = [], []
for u in held:
    nbrs = b[a == u]
    nodes.append(("a", nbrs[:SHOWN].tolist()))                            # what the new node tells about itself
    hidden.append(np.setdiff1d(nbrs[SHOWN:], nbrs[:SHOWN]))               # what it keeps to itself
# burn-in 200 sweeps, 20 samples 5 sweeps apart; every sample folds every virtual node into every chain
_, _, ((rec, score, terms), (peers, prob, _)) = bisbm.marginalize(model, 200, 20, 5, foldin=(nodes, K))

hits = sum(int(np.isin(rec[i], hidden[i]).sum()) for i in range(len(held)))
total = sum(len(h) for h in hidden)
chance = total * K / nb
print("%d virtual nodes of %d named neighbours each, %d chain terms per sum (64 chains x 20 samples)" % (len(held), SHOWN, terms))
print("%d of their %d hidden neighbours are in the top %d of %d candidates (chance: %.1f)" % (hits, total, K, nb, chance))
for i in range(3):
    post = model.foldin_posteriors(i)
    print("node %d: recommended %s; peers %s; block posterior of chain 0: %s" % (
        held[i], " ".join("%d (%.3f)" % (v, s) for v, s in zip(rec[i][:4], score[i][:4])),
        " ".join("%d (%.2f)" % (v, p) for v, p in zip(peers[i][:4], prob[i][:4])), np.round(post[0], 3)))
    assert not np.isin(rec[i], nodes[i][1]).any() and (rec[i] >= na).all() and (peers[i] < na).all()
    assert (np.diff(score[i]) <= 0).all() and (np.diff(prob[i]) <= 0).all() and prob[i].max() <= 1.0 + 1e-12
    assert abs(post.sum(axis=1) - 1.0).max() < 1e-12
assert terms == 64 * 20
