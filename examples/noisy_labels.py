"""Partly wrong labels as soft priors, with block fields: on the shipped 1000-node data set (planted: 4 + 6 blocks) a share of the
nodes gets a hint of its planted block, and some of the hints are wrong.  The model is fitted once with the hints as weights
(BlockModel.set_fields: a hinted block has WEIGHT times the prior weight of the others) and once with the same hints clamped
(BlockModel.clamp: a hinted node stays where its hint puts it).  For each fit the agreement with the planted partition is printed,
over all nodes and over the wrongly hinted ones: a clamp locks a wrong hint in, a weight can be outvoted by the node's edges.
Nothing is asserted about who wins."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bisbm = importlib.import_module("bipartitesbm-mcmc_amd")

edges = bisbm.load_edge_list(os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist"))
na = nb = 500
n, ka, kb = na + nb, 4, 6
adj = bisbm.edge_to_adj(edges, n)
types = [0] * na + [1] * nb
planted = np.concatenate([np.arange(na) * ka // na, ka + np.arange(nb) * kb // nb]).astype(np.int64)
CHAINS, SHARE, WRONG, WEIGHT = 16, 0.3, 0.2, 20.0

rng = np.random.default_rng(1)
hinted = np.flatnonzero(rng.random(n) < SHARE)
wrong = hinted[rng.random(len(hinted)) < WRONG]
hint = planted.copy()
hint[wrong] = np.where(wrong < na, (planted[wrong] + 1 + rng.integers(0, ka - 1, len(wrong))) % ka,
                       ka + (planted[wrong] - ka + 1 + rng.integers(0, kb - 1, len(wrong))) % kb)
# the start: a hinted node at its hint (what a clamp holds it at), the others dealt over the blocks of their type
start = np.concatenate([np.arange(na) % ka, ka + np.arange(nb) % kb]).astype(np.int64)
start[hinted] = hint[hinted]


routes = []  # (BlockModel.last_route() of each fit's MH sweeps)


def fit(prepare):
    """a short anneal, then greedy polishing; the labels of the chain with the lowest description length"""
    model = bisbm.BlockModel(start.astype(np.uint32), types, ka + kb, ka, kb, 1.0, adj, n_chains=CHAINS, rng="philox", seed=3)
    model.init_bisbm()
    prepare(model)
    model.run_sweeps(40, temperature=1.0)
    routes.append(model.last_route())
    model.polish(50)
    best = int(np.argmin(model.entropy()))
    labels = model.get_memberships(best).astype(np.int64)
    model.close()
    return labels


def report(what, labels):
    print("%-17s agreement with the planted partition: %.3f of all nodes, %.3f of the %d wrongly hinted nodes"
          % (what + ":", (labels == planted).mean(), (labels[wrong] == planted[wrong]).mean(), len(wrong)))


class_of_node, field = bisbm.fields_from_weights(n, ka + kb, {int(v): {int(hint[v]): WEIGHT} for v in hinted}, na=na, ka=ka)
mask = np.zeros(n, dtype=bool)
mask[hinted] = True
print("%d of %d nodes hinted, %d of the hints wrong; weight of a hinted block %g (%d field classes)" % (len(hinted), n, len(wrong), WEIGHT, len(field)))
report("hints as weights", fit(lambda model: model.set_fields(class_of_node, field)))
report("hints clamped", fit(lambda model: model.clamp(mask)))
# which kernel ran the sweeps: both fits take the production kernel, the fielded one its one-step pass
print("MH sweeps ran the %s" % ", ".join("%s kernel (%s)" % ("production" if r & bisbm.ROUTE_PRODUCTION else "generic",
                                                            "fields" if r & bisbm.ROUTE_FIELDS else "a clamp" if r & bisbm.ROUTE_HELD else "nothing held")
                                         for r in routes))
