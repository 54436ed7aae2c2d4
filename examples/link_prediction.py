"""Held-out link prediction with the pair scores: hide a tenth of the edges of the shipped 1000-node data set, sample
partitions of the rest with 64 chains, and score the hidden edges against as many random non-edges.  A pair's score is its
expected number of edges given the partition, d(u) d(v) m[b_u][b_v] / (m_r[b_u] m_r[b_v]), averaged over samples and chains on
the device (include/bisbm.h, "Posterior-predictive pair scores"); it needs no label alignment."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bisbm = importlib.import_module("bipartitesbm-mcmc_amd")

a, b = bisbm.load_edge_list(os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist"))
na = nb = 500
rng = np.random.default_rng(1)
held = rng.choice(len(a), len(a) // 10, replace=False)
keep = np.ones(len(a), dtype=bool)
keep[held] = False
edges = set(zip(a.tolist(), b.tolist()))
negatives = []
while len(negatives) < len(held):
    u, v = int(rng.integers(0, na)), int(na + rng.integers(0, nb))
    if (u, v) not in edges:
        negatives.append((u, v))
pairs = np.concatenate([np.stack([a[held], b[held]], axis=1).astype(np.int64), np.array(negatives)])

adj = bisbm.edge_to_adj((a[keep], b[keep]), na + nb)
start = np.concatenate([np.arange(na) * 4 // na, 4 + np.arange(nb) * 6 // nb])
model = bisbm.BlockModel(start, [0] * na + [1] * nb, 10, 4, 6, 1.0, adj, n_chains=64, rng="philox", seed=1)
model.shuffle_bisbm()
# burn-in 200 sweeps, 20 samples 5 sweeps apart; every sample adds every chain's term to every pair's sum
bisbm.marginalize(model, 200, 20, 5, score_pairs=pairs)
total, terms = model.pair_scores()
score = total / terms

deg = np.diff(adj[0].astype(np.int64))
positive = np.arange(len(pairs)) < len(held)


def auc(s):
    """probability that a hidden edge scores above a non-edge (ties count half)"""
    pos, neg = s[positive][:, None], s[~positive][None, :]
    return float((pos > neg).mean() + 0.5 * (pos == neg).mean())


print("terms per pair: %d (64 chains x 20 samples)" % terms)
print("AUC of the pooled pair scores: %.3f; of the degree product alone: %.3f"
      % (auc(score), auc(deg[pairs[:, 0]].astype(float) * deg[pairs[:, 1]])))
assert terms == 64 * 20 and auc(score) > auc(deg[pairs[:, 0]].astype(float) * deg[pairs[:, 1]])
