"""Greedy polishing: anneal as python_api.py does, then move every node to its block of least description length until a whole
sweep moves nothing.  The anneal's last sweeps accept a move only if the ONE proposed target is downhill; polish() looks at all
targets of every node, so what it returns is a local minimum of the description length under single-node moves."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bisbm = importlib.import_module("bipartitesbm-mcmc_amd")

edges = bisbm.load_edge_list(os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist"))
na = nb = 500
adj = bisbm.edge_to_adj(edges, na + nb)
types = [0] * na + [1] * nb
start = np.repeat(np.arange(4), 125).tolist() + (4 + np.repeat(np.arange(6), [84, 84, 83, 83, 83, 83])).tolist()

# 64 chains, 4 + 6 blocks: 20 sweeps at T = 1, then an exponential cooling of 30 sweeps
model = bisbm.BlockModel(start, types, 10, 4, 6, 1.0, adj, n_chains=64, rng="philox", seed=1)
model.shuffle_bisbm()
mh = bisbm.MetropolisHasting()
mh.anneal(model, bisbm.constant_schedule, [1.0], 20 * 1000, 1 << 60)
mh.anneal(model, bisbm.exponential_schedule, [1.0, 0.9997], 30 * 1000, 1 << 60)
before = model.entropy()

moved, sweeps = model.polish(100)
after = model.entropy()
assert (sweeps < 100).all(), "a chain did not settle within 100 sweeps"
assert (after <= before).all() and (after[moved > 0] < before[moved > 0]).all()
best = int(np.argmin(after))
print("description length before polish: best %.2f, mean %.2f" % (before.min(), before.mean()))
print("description length after polish:  best %.2f, mean %.2f (chain %d)" % (after.min(), after.mean(), best))
print("moves per chain %d .. %d, sweeps until settled %d .. %d" % (moved.min(), moved.max(), sweeps.min(), sweeps.max()))

again, one = model.polish(100)
assert (again == 0).all() and (one == 1).all()
print("a second polish moves nothing: %d moves, %d sweep(s) per chain" % (again.sum(), one.max()))
