"""Recommendation with the query scores: hide a tenth of the edges of the shipped 1000-node data set, sample partitions of the
rest with 64 chains, and ask for every type-a node that lost an edge which 20 type-b nodes it should be linked to.  A query's
candidates are ALL nodes of the other type; a candidate's score is the expected number of edges between the two given the
partition, averaged over samples and chains, and the ranking -- without the neighbours the node already has -- is made on the
device (include/bisbm.h, "Query scores").  Reported: how many hidden edges come back among the 20, against a ranking by the
candidates' degrees alone."""
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
rng = np.random.default_rng(1)
held = rng.choice(len(a), len(a) // 10, replace=False)
keep = np.ones(len(a), dtype=bool)
keep[held] = False
kept = set(zip(a[keep].tolist(), b[keep].tolist()))
hidden = sorted({(int(u), int(v)) for u, v in zip(a[held], b[held])} - kept)  # (an edge that is still there is not hidden)
queries = np.unique([u for u, _ in hidden])

adj = bisbm.edge_to_adj((a[keep], b[keep]), na + nb)
start = np.concatenate([np.arange(na) * 4 // na, 4 + np.arange(nb) * 6 // nb])
model = bisbm.BlockModel(start, [0] * na + [1] * nb, 10, 4, 6, 1.0, adj, n_chains=64, rng="philox", seed=1)
model.shuffle_bisbm()
# burn-in 200 sweeps, 20 samples 5 sweeps apart; every sample adds every chain's term to every (query, candidate) sum
_, _, (nodes, scores, terms) = bisbm.marginalize(model, 200, 20, 5, recommend=(queries, K))

row_of = {int(q): i for i, q in enumerate(queries)}
hits = sum(v in nodes[row_of[u]] for u, v in hidden)
# the same question answered by the candidates' degrees alone (the one-block model)
deg = np.diff(adj[0].astype(np.int64))
by_degree = na + np.lexsort((np.arange(nb), -deg[na:]))
degree_hits = 0
for u, v in hidden:
    mine = set(adj[1][int(adj[0][u]):int(adj[0][u + 1])].tolist())
    degree_hits += v in [int(c) for c in by_degree if int(c) not in mine][:K]

print("%d queries, %d candidates each, %d chain terms per score (64 chains x 20 samples)" % (len(queries), nb, terms))
print("held-out edges in the top %d: %d of %d (ranking by degree alone: %d)" % (K, hits, len(hidden), degree_hits))
best = int(np.argmax(scores[:, 0]))
print("node %d -> %s" % (queries[best], " ".join("%d (%.3f)" % (n, s) for n, s in zip(nodes[best][:5], scores[best][:5]))))
assert terms == 64 * 20 and hits > degree_hits
