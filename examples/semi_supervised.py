"""Semi-supervised inference with clamped nodes: every 20th node of the shipped 1000-node data set is held at its planted
block in all chains, the rest is shuffled and sampled by 64 chains, and the chains' label histograms are pooled WITHOUT an
alignment.  Every block holds clamped seeds with the same label in every chain, so a label means the same block in every chain
and the raw histogram is a marginal over chains.  Beside it the same run without a clamp: every chain numbers its blocks its
own way (label switching), and the unaligned pool says little."""
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
# the planted partition: contiguous blocks, 4 of type a and 6 of type b
planted = np.array(np.repeat(np.arange(4), 125).tolist() + (4 + np.repeat(np.arange(6), [84, 84, 83, 83, 83, 83])).tolist(), dtype=np.uint32)
seeds = np.arange(0, n, 20)
is_open = np.ones(n, dtype=bool)
is_open[seeds] = False


def run(clamp):
    model = bisbm.BlockModel(planted, types, 10, 4, 6, 1.0, adj, n_chains=64, rng="philox", seed=1)
    if clamp is not None:
        model.clamp(clamp)    # held at the labels the chains have now: the planted ones
    model.shuffle_bisbm()     # the open nodes' labels are permuted among themselves, the clamped ones stay
    labels, counts = bisbm.marginalize(model, 40, 20, 2, align=False)
    if clamp is not None:
        assert (model.clamped() == ~is_open).all()
        assert all((model.get_memberships(c)[seeds] == planted[seeds]).all() for c in range(model.n_chains))
        assert (labels[seeds] == planted[seeds]).all()
    model.close()
    return float((labels[is_open] == planted[is_open]).mean())


held = run(seeds)
free = run(None)
print("%d of %d nodes clamped to the planted partition, 64 chains, unaligned pool" % (len(seeds), n))
print("open nodes whose MAP label is the planted one, clamped seeds: %.3f" % held)
print("open nodes whose MAP label is the planted one, no clamp:      %.3f" % free)
