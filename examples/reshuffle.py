"""Pair reshuffles: chains at T = 1 that sit in different modes are given moves that re-divide the nodes of two blocks at once.
Every sampler besides moves one node at a time; a reshuffle proposes a whole new division of two blocks' nodes (a few restricted
Gibbs scans from a random start) and accepts or rejects it as one move, so exp(-S) stays exactly invariant.  The running sum of
dS keeps tracking the description length through accepted and rejected moves alike."""
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

# 64 chains, 4 + 6 blocks, 30 MH sweeps at T = 1 from a random start
model = bisbm.BlockModel(start, types, 10, 4, 6, 1.0, adj, n_chains=64, rng="philox", seed=1)
model.shuffle_bisbm()
model.run_sweeps(30)
S0, sum0 = model.entropy(), model.get_entropy()

# 21 moves per chain (there are C(4,2) + C(6,2) = 21 pairs; a move draws one), 3 scans before the proposal (the convention of
# the literature, not a measurement), beta = 1
accepted = model.reshuffle(21, scans=3, beta=1.0)
S1, sum1 = model.entropy(), model.get_entropy()
assert (model.reshuffles_total() == 21).all()
assert np.allclose(S1 - S0, sum1 - sum0, rtol=0, atol=1e-9 * np.abs(S0).max())
last = model.reshuffle_last()[0]
print("pair reshuffles: %d of %d accepted over 64 chains" % (accepted.sum(), 21 * 64))
print("description length: mean %.2f -> %.2f, best %.2f -> %.2f" % (S0.mean(), S1.mean(), S0.min(), S1.min()))
print("chain 0, last move: type %s, blocks %d and %d, %d members, dS %.3f, A %.3g, %s"
      % ("ab"[last["type"]], last["r"], last["s"], last["M"], last["dS_fwd"] - last["dS_rev"], last["A"],
         "accepted" if last["accepted"] else "rejected"))

# interleaved with sweeps, as marginalize(..., reshuffles=m) and `mcmc --marginalize --reshuffle M` run them
labels, counts = bisbm.marginalize(model, 5, 4, 2, align=True, reshuffles=5)
print("marginalize with reshuffles: %d of %d accepted" % (model.reshuffle_stats["accepted"], model.reshuffle_stats["proposed"]))
print("the running sum tracks the description length through every move")
