"""Chains that cooperate: population annealing (include/bisbm.h, "Population annealing") against 64 independent anneals at the
same sweep budget, on the shipped 1000-node data set.  Both cool from T = 4 to T = 0.5 in 68 sweeps per chain: the independent
chains along one exponential schedule each, the population through 17 temperatures with 4 sweeps at each -- and between two
temperatures the chains are resampled by description length, so the sweeps of a chain that sits in a poor basin go to a copy of a
chain that does not.  The run also estimates ln Z(1/0.5) - ln Z(1/4), Z(beta) = the sum of exp(-beta S) over partitions."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bisbm = importlib.import_module("bipartitesbm-mcmc_amd")

a, b = bisbm.load_edge_list(os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist"))
na = nb = 500
n = na + nb
adj = bisbm.edge_to_adj((a, b), n)
start = np.concatenate([np.arange(na) * 4 // na, 4 + np.arange(nb) * 6 // nb])
chains, sweeps_per_step = 64, 4
temps = np.geomspace(4.0, 0.5, 17)
budget = len(temps) * sweeps_per_step  # sweeps per chain, the burn-in at temps[0] included


def fresh():
    model = bisbm.BlockModel(start, [0] * na + [1] * nb, 10, 4, 6, 1.0, adj, n_chains=chains, rng="philox", seed=1)
    model.shuffle_bisbm()
    return model


# 64 independent anneals: T = 4 alpha^step, alpha chosen to reach 0.5 at the last step; no early stop
model = fresh()
alpha = (temps[-1] / temps[0]) ** (1.0 / (budget * n))
bisbm.MetropolisHasting().anneal(model, bisbm.exponential_schedule, [temps[0], alpha], budget * n, 1 << 60)
independent = model.entropy()
model.close()

# the population: the same budget
model = fresh()
out = bisbm.population_anneal(model, temps, sweeps_per_step, burn_in_sweeps=sweeps_per_step)
state = model.population_state()
print("%d chains, %d sweeps each, T = %g -> %g" % (chains, budget, temps[0], temps[-1]))
print("independent anneals:  best description length %.2f, median %.2f" % (independent.min(), np.median(independent)))
print("population annealing: best description length %.2f (chain %d), median %.2f"
      % (out["entropy"][out["best_chain"]], out["best_chain"], np.median(out["entropy"])))
print("distinct ancestors after every step: %s" % out["distinct"].tolist())
print("evidence estimate ln Z(beta = %g) - ln Z(beta = %g) = %.3f" % (1 / temps[-1], 1 / temps[0], state["log_ratio_total"]))
# what is structurally true: the totals add up, and families only die out
assert state["rounds"] == len(temps) - 1 and len(out["log_ratio"]) == len(temps) - 1
assert abs(state["log_ratio_total"] - np.cumsum(out["log_ratio"])[-1]) <= 1e-12 * abs(state["log_ratio_total"])
assert (np.diff(out["distinct"].astype(np.int64)) <= 0).all() and out["distinct"][0] <= chains
assert len(np.unique(state["ancestor"])) == out["distinct"][-1]
assert out["entropy"][out["best_chain"]] == out["entropy"].min()
