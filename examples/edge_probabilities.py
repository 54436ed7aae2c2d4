"""Exact edge probabilities: hide 5 % of the edges of the shipped 1000-node data set, sample partitions of the rest with 32
chains, and ask for every hidden pair and as many random non-edges what ADDING the edge does to the description length.  One
chain's answer is dS = S(G + e, b) - S(G, b), exact and O(1) (include/bisbm.h, "Edge probabilities"); exp(-dS) averaged over
samples and chains is the posterior-predictive odds of the edge, and its logarithm (`log_prob`) can be added up over the hidden
edges into a held-out log-likelihood -- which the plug-in pair scores cannot.  The same call with kind "-" weighs the edges that
are there: the ones whose removal costs least are the candidates for spurious links."""
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
held = rng.choice(len(a), len(a) // 20, replace=False)
keep = np.ones(len(a), dtype=bool)
keep[held] = False
edges = set(zip(a.tolist(), b.tolist()))
negatives = []
while len(negatives) < len(held):
    u, v = int(rng.integers(0, na)), int(na + rng.integers(0, nb))
    if (u, v) not in edges:
        negatives.append((u, v))
hidden = np.stack([a[held], b[held]], axis=1).astype(np.int64)
present = np.unique(np.stack([a[keep], b[keep]], axis=1).astype(np.int64), axis=0)
pairs = np.concatenate([hidden, np.array(negatives), present])
kinds = ["+"] * (2 * len(held)) + ["-"] * len(present)

adj = bisbm.edge_to_adj((a[keep], b[keep]), na + nb)
start = np.concatenate([np.arange(na) * 4 // na, 4 + np.arange(nb) * 6 // nb])
model = bisbm.BlockModel(start, [0] * na + [1] * nb, 10, 4, 6, 1.0, adj, n_chains=32, rng="philox", seed=1)
model.shuffle_bisbm()
# burn-in 100 sweeps, 10 samples 5 sweeps apart; every sample adds every chain's dS and exp(-dS) to every pair's sums
bisbm.marginalize(model, 100, 10, 5, edge_probs=(pairs, kinds))
r = model.edge_probs()
H = len(held)
log_prob = r["log_prob"]
positive = np.arange(2 * H) < H


def auc(s):
    """probability that a hidden edge scores above a non-edge (ties count half)"""
    pos, neg = s[positive][:, None], s[~positive][None, :]
    return float((pos > neg).mean() + 0.5 * (pos == neg).mean())


print("terms per pair: %d (32 chains x 10 samples)" % r["terms"])
print("mean log odds of adding: hidden edges %.3f, random non-edges %.3f; AUC %.3f"
      % (log_prob[:H].mean(), log_prob[H:2 * H].mean(), auc(log_prob[:2 * H])))
print("held-out log-likelihood of the hidden edges (sum of log_prob): %.2f" % log_prob[:H].sum())
cost = r["mean_dS"][2 * H:]  # what removing each present edge does to the description length
order = np.argsort(cost)
print("present edges whose removal costs least (mean dS): " + ", ".join("%d-%d %.2f" % (*present[i], cost[i]) for i in order[:5]))
assert r["terms"] == 32 * 10 and log_prob[:H].mean() > log_prob[H:2 * H].mean()
