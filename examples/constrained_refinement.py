"""Refining a coarse fit inside its own blocks with block constraints: the shipped 1000-node data set (planted: 4 + 6 blocks) is
first fitted with 2 + 3 blocks; every coarse block then gets two children, every node is allowed the children of its parent only
(BlockModel.constrain), and the model is refitted with 4 + 6 blocks from a start that deals each parent's nodes over its children.
The description lengths of the coarse fit, the constrained refit and an unconstrained refit from the same start are printed; in
the constrained one no node has left its parent."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bisbm = importlib.import_module("bipartitesbm-mcmc_amd")

edges = bisbm.load_edge_list(os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist"))
na = nb = 500
n = na + nb
adj = bisbm.edge_to_adj(edges, n)
types = [0] * na + [1] * nb
CHAINS = 16


def fit(model):
    """a short anneal, then greedy polishing; the labels and the description length of the best chain"""
    model.run_sweeps(30, temperature=1.0)
    model.polish(50)
    S = model.entropy()
    best = int(np.argmin(S))
    return model.get_memberships(best).astype(np.int64), float(S[best])


# 1. the coarse fit: 2 + 3 blocks from a shuffled start
ka0, kb0 = 2, 3
start = np.concatenate([np.arange(na) * ka0 // na, ka0 + np.arange(nb) * kb0 // nb]).astype(np.uint32)
coarse_model = bisbm.BlockModel(start, types, ka0 + kb0, ka0, kb0, 1.0, adj, n_chains=CHAINS, rng="philox", seed=1)
coarse_model.shuffle_bisbm()
coarse, S_coarse = fit(coarse_model)
coarse_model.close()

# 2. every coarse block gets two children: parent p of type a -> blocks 2p, 2p + 1; parent ka0 + q of type b -> 2 ka0 + 2q, + 1
ka, kb = 2 * ka0, 2 * kb0
children = {p: [2 * p, 2 * p + 1] for p in range(ka0 + kb0)}  # (for type b this is 2 ka0 + 2q as well: 2 (ka0 + q))
class_of_node, allowed = bisbm.constraints_from_lists(n, ka + kb, {v: children[int(coarse[v])] for v in range(n)}, na=na, ka=ka)
refined_start = bisbm.admissible_start(na, nb, ka, kb, class_of_node, allowed)


def refit(constrained):
    model = bisbm.BlockModel(refined_start, types, ka + kb, ka, kb, 1.0, adj, n_chains=CHAINS, rng="philox", seed=2)
    if constrained:
        model.constrain(class_of_node, allowed)
    model.shuffle_bisbm()  # (under constraints: within every parent's nodes)
    labels, S = fit(model)
    inside = all(allowed[class_of_node, model.get_memberships(c)].all() for c in range(CHAINS))
    model.close()
    return labels, S, inside


fine, S_fine, inside = refit(True)
free, S_free, _ = refit(False)
print("coarse fit, %d + %d blocks:                description length %.2f" % (ka0, kb0, S_coarse))
print("constrained refit, %d + %d blocks:         description length %.2f (%d classes)" % (ka, kb, S_fine, len(allowed)))
print("unconstrained refit from the same start: description length %.2f" % S_free)
print("every node inside its parent's children: %s" % (inside and bool((fine // 2 == coarse).all())))
