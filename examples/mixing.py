"""Chain traces: how fast does a chain forget its partition?  Metropolis-Hastings sweeps and heat-bath sweeps start from the same
partitions of the n_1000 data set; each model records after every sweep, and the lag curves -- the mean variation of information
and the share of relabelled nodes between a chain now and the same chain k records ago -- are printed side by side with the
integrated autocorrelation time of the description length.  Lags are in sweeps; a heat-bath sweep costs more than an MH sweep
(tools/trace_bench.py compares them per unit time)."""
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
DEPTH, BURN_IN, RECORDS = 8, 50, 200

curves = {}
for name in ("mh", "heatbath"):
    # the same seed: both models shuffle to the same partitions and burn in with the same MH sweeps
    model = bisbm.BlockModel(start, types, 10, 4, 6, 1.0, adj, n_chains=32, rng="philox", seed=1)
    model.shuffle_bisbm()
    model.run_sweeps(BURN_IN)
    model.trace_set(DEPTH)
    for _ in range(RECORDS):
        if name == "mh":
            model.run_sweeps(1)
        else:
            model.heatbath_sweeps(1)
        model.trace_record()
    lags = model.trace_lags()
    assert lags["records"] == RECORDS and lags["pairs"].tolist() == [RECORDS - a for a in range(1, DEPTH + 1)]
    tau, window, rhat = bisbm.trace_summary(model.trace_series("S"))
    curves[name] = (lags["vi_mean"].mean(axis=0), lags["changed"].mean(axis=0), tau, window, rhat)
    model.close()

print("lag (sweeps)   VI mh    VI heatbath   changed mh   changed heatbath")
for a in range(DEPTH):
    print("%12d   %.4f   %.4f        %.4f       %.4f" % (a + 1, curves["mh"][0][a], curves["heatbath"][0][a], curves["mh"][1][a], curves["heatbath"][1][a]))
for name in ("mh", "heatbath"):
    _, _, tau, window, rhat = curves[name]
    short = int((window >= RECORDS // 2).sum())
    print("%-8s tau_S (sweeps): median %.2f, max %.2f over 32 chains (%d too short to tell); split R-hat of S: %.4f"
          % (name, float(np.median(tau)), float(tau.max()), short, rhat))
