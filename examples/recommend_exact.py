"""Recommendation by exact edge odds, beside the query scores: hide a tenth of the edges of the shipped 1000-node data set,
sample partitions of the rest with 32 chains, and ask for every type-a node that lost an edge which 20 type-b nodes it should be
linked to -- once by `recommend` (the plug-in expected edge count of include/bisbm.h, "Query scores") and once by
`recommend_edges` (exp(-dS) of the exact change of the description length when the edge is added, "Edge queries": it carries
the degree part, the multiplicity term and the edge-count prior, and its logarithm is a log-probability).  Both rank ALL nodes
of the other type on the device, without the neighbours the node already has, in the same run.  Reported for both: how many
hidden edges come back among the 20.  Nothing is asserted about which of the two wins."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bisbm = importlib.import_module("bipartitesbm-mcmc_amd")

K, CHAINS, SAMPLES = 20, 32, 10
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
model = bisbm.BlockModel(start, [0] * na + [1] * nb, 10, 4, 6, 1.0, adj, n_chains=CHAINS, rng="philox", seed=1)
model.shuffle_bisbm()
# burn-in 100 sweeps, 10 samples 5 sweeps apart; every sample adds every chain's term to every (query, candidate) sum of both
_, _, (nodes, scores, terms), (e_nodes, w_sum, log_prob) = bisbm.marginalize(model, 100, SAMPLES, 5, recommend=(queries, K),
                                                                            recommend_edges=(queries, K))
row_of = {int(q): i for i, q in enumerate(queries)}
hits = sum(v in nodes[row_of[u]] for u, v in hidden)
e_hits = sum(v in e_nodes[row_of[u]] for u, v in hidden)
shared = np.mean([len(set(x.tolist()) & set(y.tolist())) for x, y in zip(nodes, e_nodes)])

print("%d queries, %d candidates each, %d chain terms per cell (%d chains x %d samples)" % (len(queries), nb, terms, CHAINS, SAMPLES))
print("held-out edges in the top %d: recommend %d of %d, recommend_edges %d of %d" % (K, hits, len(hidden), e_hits, len(hidden)))
print("the two lists share %.1f of %d nodes on average" % (shared, K))
best = int(np.argmax(w_sum[:, 0]))
print("node %d -> %s" % (queries[best], " ".join("%d (ln P = %.3f)" % (n, lp) for n, lp in zip(e_nodes[best][:5], log_prob[best][:5]))))
assert terms == CHAINS * SAMPLES == model.edge_queries(0)["terms"]
