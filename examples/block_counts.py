"""Split and merge moves: the chains sample the block counts with the partition.  The n_1000 data set (planted with 4 + 6
blocks) is started at a wrong shape, 2 + 2; rounds of MH sweeps and split / merge moves then change (Ka, Kb) chain by chain, each
move accepted or rejected as a whole so that exp(-S) stays exactly invariant over the partitions of every shape, and the visited
shapes are counted.  The running sum of dS keeps tracking the description length across the shapes."""
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
start = np.repeat(np.arange(2), 250).tolist() + (2 + np.repeat(np.arange(2), 250)).tolist()

# 32 chains at the wrong shape 2 + 2, 10 MH sweeps at T = 1 from a random start
model = bisbm.BlockModel(start, types, 4, 2, 2, 1.0, adj, n_chains=32, rng="philox", seed=1)
model.shuffle_bisbm()
model.run_sweeps(10)
S0, sum0 = model.entropy(), model.get_entropy()

# rounds of {2 MH sweeps, 4 split / merge moves with 3 scans}, block counts between 1 + 1 and 12 + 12
for _ in range(30):
    model.run_sweeps(2)
    model.split_merge(4, scans=3, beta=1.0, k_min=(1, 1), k_max=(12, 12))
S1, sum1 = model.entropy(), model.get_entropy()
assert np.allclose(S1 - S0, sum1 - sum0, rtol=0, atol=1e-9 * np.abs(S0).max())
total = model.split_merge_total().sum(axis=0)
print("split / merge moves: splits %d of %d accepted, merges %d of %d accepted over 32 chains" % (total[1], total[0], total[3], total[2]))
print("description length: mean %.2f -> %.2f, best %.2f -> %.2f" % (S0.mean(), S1.mean(), S0.min(), S1.min()))

# the shape histogram over samples and chains, as marginalize(..., split_merges=m) counts it
shape_counts, best = bisbm.marginalize(model, 0, 10, 2, split_merges=4, k_min=(1, 1), k_max=(12, 12))
print("visited (Ka, Kb) over 10 samples of 32 chains:")
for shape, count in sorted(shape_counts.items(), key=lambda kv: -kv[1]):
    print("  %2d + %-2d  %4d   lowest description length seen %.2f" % (shape[0], shape[1], count, best[shape][0]))
print("the running sum tracks the description length through every change of shape")
