"""Replica exchange with mixed moves: every chain of an ensemble runs MH sweeps, heat-bath sweeps and pair reshuffles at its own
rung's temperature, and neighbouring rungs trade temperatures after every round.  A reshuffle re-divides the nodes of two blocks in
one accepted or rejected move; it is accepted most often on the hot rungs, and the exchange is how an accepted re-division
reaches the cold rung that is sampled.  The per-rung table says what each move did where."""
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

# 64 chains as 16 ensembles of 4 rungs, 4 + 6 blocks, from a random start
ladder = [1.0, 1.25, 1.6, 2.0]
model = bisbm.BlockModel(start, types, 10, 4, 6, 1.0, adj, n_chains=64, rng="philox", seed=1)
model.shuffle_bisbm()
model.set_tempering(ladder)

# 30 rounds: one MH sweep, one heat-bath sweep and two reshuffles of 3 scans per chain, then one exchange
S0 = model.entropy()
model.tempering_rounds(30, mh=1, heatbath=1, reshuffles=2, scans=3)
S1 = model.entropy()
rung, T = model.tempering_state()
stats = model.tempering_rung_stats()
attempted, accepted, rounds = model.tempering_stats()
print("%d rounds; description length on rung 0: mean %.2f, best %.2f (start: mean %.2f)" % (rounds, S1[rung == 0].mean(), S1[rung == 0].min(), S0.mean()))
print("rung  T      MH accepted  heat-bath moved  reshuffles accepted  swaps with the next rung")
for i, t in enumerate(ladder):
    swap = "%d / %d" % (accepted[i], attempted[i]) if i + 1 < len(ladder) else "-"
    print("%4d  %-5g  %10.3f  %15.3f  %8d / %-8d  %s" % (i, t, stats["mh_accepted"][i] / stats["mh_steps"][i],
                                                      stats["heatbath_moves"][i] / stats["heatbath_steps"][i],
                                                      stats["reshuffles_accepted"][i], stats["reshuffles"][i], swap))
assert stats["reshuffles"].sum() == model.reshuffles_total().sum() == 30 * 2 * 64

# the same rounds as the sampler of a marginalization: burn-in and the gaps between samples count rounds
labels, counts = bisbm.marginalize(model, 5, 4, 2, align=True, tempering=ladder, rung_moves={"mh": 1, "heatbath": 1, "reshuffles": 2, "scans": 3})
print("marginalize with rung_moves: %d samples of %d cold chains, %d exchange rounds" % (4, 16, model.tempering_stats()[2]))
