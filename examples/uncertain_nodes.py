"""Which nodes are not settled, with the node conditionals: a planted 600 + 600 graph with 4 + 4 blocks and few edges per node,
32 chains, and for EVERY node its full conditional over the blocks of its type given all other labels, in every chain, at 5
samples.  `stay` is the probability of the block the node sits in, the entropy says how flat the conditional is, the margin what
the cheapest other block costs in nats -- none of them depends on how a chain numbers its blocks, so the 32 chains pool without
any alignment.  With align=True the conditional rows also go through the alignment into a SOFT marginal: after 5 samples the
hard histogram resolves 1 / 160, the soft one carries every chain's whole row (include/bisbm.h, "Node conditionals")."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bisbm = importlib.import_module("bipartitesbm-mcmc_amd")
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

na = nb = 600
ka = kb = 4
chains, samples = 32, 5
a, b = syn.planted_edges(na, nb, 3600, ka, kb, seed=3, p_in=0.7)
adj = bisbm.edge_to_adj((a, b), na + nb)
model = bisbm.BlockModel(syn.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, 1.0, adj, n_chains=chains,
                         rng="philox", seed=1)
model.init_bisbm()  # (the planted partition as the start: the chains stay in one mode, which is what pooling a marginal assumes)
labels, counts, stats, (soft, soft_terms) = bisbm.marginalize(model, 100, samples, 5, align=True, conditionals=(None, 1.0))

terms = stats["terms"]
stay, entropy = stats["stay"] / terms, stats["entropy"] / terms
margin = np.where(stats["free"] > 0, stats["margin"] / np.maximum(stats["free"], 1), np.nan)
hard = counts / counts.sum(axis=1, keepdims=True)
soft = soft / soft_terms
deg = np.diff(np.asarray(adj[0]).astype(np.int64))
print("%d nodes, %d chain terms per sum (%d chains x %d samples); mean stay %.3f, mean entropy %.3f nats" % (na + nb, terms, chains, samples, stay.mean(), entropy.mean()))
print("the 20 least settled nodes (lowest mean probability of the node's own block):")
print("  node  deg   stay  entropy  margin   hard top / terms   soft marginal")
for v in np.argsort(stay, kind="stable")[:20]:
    k = ka if v < na else kb
    print("  %4d  %3d  %.3f   %.3f  %+6.2f   %16.3f   %s" % (v, deg[v], stay[v], entropy[v], margin[v], hard[v].max(), " ".join("%.3f" % x for x in soft[v, :k])))
settled = stay > 0.99
print("%d nodes have stay > 0.99; among them the soft and the hard marginal agree on the block of %d" % (settled.sum(), (soft.argmax(axis=1) == hard.argmax(axis=1))[settled].sum()))
assert terms == soft_terms == chains * samples and np.allclose(soft.sum(axis=1), 1.0, atol=1e-9)
assert (stay > 0).all() and (stay <= 1 + 1e-12).all() and (entropy >= 0).all() and (entropy <= np.log(max(ka, kb)) + 1e-9).all()
assert (soft.argmax(axis=1) == hard.argmax(axis=1))[settled].mean() > 0.99
