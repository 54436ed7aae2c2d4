"""Time of one marginal sample with and without label alignment (include/bisbm.h, "Label alignment before pooling") at
BASELINE configs[2] -- N = 10^6 (5e5 + 5e5), E = 10^7, 32 + 32 blocks, 1024 chains -- and at 128 + 128 blocks on the same
sizes.  The chains sit on the planted partition, each in its own random numbering (the state a long run aligns), after two
sweeps.  Prints one JSON line per shape: ms per unaligned / aligned bisbm_marginals_accumulate (host clock around the
call, which ends in a device synchronise), the aligned one per overlap-table kernel (BISBM_ALIGN_TABLE) where it fits.
Per-kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/align_bench.py --quick`.

    python tools/align_bench.py [--quick] [--chains 1024] [--reps 5]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = importlib.import_module("bipartitesbm-mcmc_amd")
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")


def timed(fn, reps):
    fn()  # warm-up (first launches, buffers allocated on the first aligned sample)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t))


def one_shape(na, nb, E, k, chains, reps, quick):
    a, b = syn.planted_edges(na, nb, E, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), na + nb)
    truth = syn.contiguous_labels(na, nb, k, k)
    m = B.BlockModel(truth, syn.types_vector(na, nb), 2 * k, k, k, 1.0, (rp, cl), n_chains=chains, seed=1)
    st = np.random.default_rng(0)
    for c in range(chains):
        perm = np.concatenate([st.permutation(k), k + st.permutation(k)]).astype(np.uint32)
        m.set_memberships(perm[truth], chain=c)
    m.init_bisbm()
    m.run_sweeps(2)
    out = {"shape": "%d+%d" % (k, k), "n": na + nb, "edges": E, "chains": chains,
           "label_bytes_per_pass": chains * (na + nb)}
    m.marginals_reset()
    out["plain_ms"] = timed(m.marginals_accumulate, reps)[0]
    m.marginals_reset()
    m.marginals_set_alignment(True)
    modes = ["default"] if quick else ["default", "wave", "block", "hbm"]
    for mode in modes:
        if mode == "default":
            os.environ.pop("BISBM_ALIGN_TABLE", None)
        else:
            os.environ["BISBM_ALIGN_TABLE"] = mode
        out["aligned_ms_" + mode] = timed(m.marginals_accumulate, reps)[0]
    os.environ.pop("BISBM_ALIGN_TABLE", None)
    perm, tot = m.marginals_alignment(chains - 1)
    out["last_chain_overlap"] = int(tot)
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="the default table kernel only, fewer repetitions (profiler runs)")
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    reps = 2 if args.quick else args.reps
    for k in (32, 128):
        print(json.dumps(one_shape(500_000, 500_000, 10_000_000, k, args.chains, reps, args.quick)), flush=True)


if __name__ == "__main__":
    main()
