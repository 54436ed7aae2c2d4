"""How many different answers did the chains find?  64 chains sample partitions of the shipped 1000-node data set from
independent shuffles; their partitions are compared pair by pair on the device (variation of information, in nats: include/bisbm.h,
"Partition distances and posterior modes") and grouped into modes: chains joined by a path of pairs with VI <= the threshold share
a mode.  The threshold is the caller's resolution; here a tenth of the mean partition entropy.  Then every mode gets a marginal
of its own (include/bisbm.h, "Mode-resolved marginals"): one histogram per mode, aligned to the mode's own reference -- first with
the chains' modes fixed by the grouping, then anchored: every sample goes to the mode of its nearest anchor partition."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bisbm = importlib.import_module("bipartitesbm-mcmc_amd")

a, b = bisbm.load_edge_list(os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist"))
na = nb = 500
adj = bisbm.edge_to_adj((a, b), na + nb)
start = np.concatenate([np.arange(na) * 4 // na, 4 + np.arange(nb) * 6 // nb])
model = bisbm.BlockModel(start, [0] * na + [1] * nb, 10, 4, 6, 1.0, adj, n_chains=64, rng="philox", seed=1)
model.shuffle_bisbm()
model.run_sweeps(200)

vi, H = model.partition_distances()
threshold = 0.1 * H.mean()
found = model.partition_modes(threshold)
S = model.entropy()
print("64 chains, mean partition entropy %.3f nats, VI between chains %.3f .. %.3f, threshold %.3f" % (H.mean(), vi[vi > 0].min() if (vi > 0).any() else 0.0, vi.max(), threshold))
print("modes: %d" % len(found["medoids"]))
for k, (medoid, weight, low) in enumerate(zip(found["medoids"], found["weights"], found["lowest_entropy"])):
    print("mode %d: share %.3f, medoid chain %d, lowest description length chain %d (%.1f)" % (k, weight, medoid, low, S[low]))
# the table behind one distance: how the blocks of the two most different chains overlap
c, d = np.unravel_index(np.argmax(vi), vi.shape)
print("chains %d and %d, VI %.3f, contingency table:" % (c, d, vi[c, d]))
print(model.partition_contingency(c, d))
assert (vi == vi.T).all() and (np.diag(vi) == 0).all() and abs(found["weights"].sum() - 1) < 1e-12
assert model.partition_contingency(c, d).sum() == na + nb

# each answer by itself: the chains are counted into the histogram of their mode, 10 samples a sweep apart
out = bisbm.marginalize_modes(model, 0, 10, 1, mode_of_chain=found)
for g, (weight, ref, terms) in enumerate(zip(out["weights"], out["ref_chain"], out["terms"])):
    settled = out["top"][g] / terms
    sizes = np.bincount(out["labels"][g], minlength=10)
    print("mode %d: share %.3f, aligned to chain %d, %d chain samples, mean top/terms %.3f, %d nodes below 0.9, block sizes %s"
          % (g, weight, ref, terms, settled.mean(), int((settled < 0.9).sum()), sizes.tolist()))
assert (out["counts"].sum(axis=2) == out["terms"][:, None]).all() and out["terms"].sum() == 10 * 64

# the same with anchored modes (include/bisbm.h, "Anchored modes"): the grouping only picks one anchor partition per mode, and every
# sample counts each chain into the mode of its nearest anchor within the threshold, so a chain that hops is counted where it
# is and a mode's weight is its share of the samples
out = bisbm.marginalize_modes(model, 0, 10, 1, threshold=threshold, reassign=True)
print("anchored: %d mode(s), sample shares %s, %d chain sample(s) beyond the threshold, %d chain(s) counted into more than one mode"
      % (len(out["terms"]), np.round(out["weights"], 3).tolist(), out["unassigned"], out["moved"]))
assert out["terms"].sum() + out["unassigned"] == 10 * 64 and (out["visits"].sum(axis=0) == out["terms"]).all()
# how far is every chain from a partition that is no chain: here the contiguous start
to_start, H_start = model.partition_distances_to(start)
print("VI to the contiguous start partition (entropy %.3f): %.3f .. %.3f" % (H_start[0], to_start.min(), to_start.max()))
