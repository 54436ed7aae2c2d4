"""What the block summaries (include/bisbm.h, "Block summaries") add to an aligned sample at BASELINE configs[2] -- N = 10^6
(5e5 + 5e5), E = 10^7, 32 + 32 blocks, 1024 chains: one bisbm_marginals_accumulate with the sums off (the yardstick, the same
sample in the same run), on, and on with BISBM_BLOCK_KEEP_LAST; pooled (one mode of every chain) and with the chains split evenly
(chain c -> mode c mod M) into M = 4 and 32 static modes, all in one process.  The chains sit on the planted partition, each
in its own random numbering, after two sweeps, as in tools/align_bench.py.  The configurations are timed in turn, `--rounds`
times over, so that a drift of the machine shows in every figure alike; per figure the median, the least and the largest of all
its repetitions in ms (host clock around the call, which ends in a device synchronise; one warm-up call before every series).
BISBM_BLOCK_SPLIT=1 in the environment times the form with one owner per cell.  Prints one JSON line and writes it to
profiles/block_summary_bench.json.

    python tools/block_summary_bench.py [--chains 1024] [--rounds 3] [--reps 5] [--modes 1 4 32] [--out profiles/block_summary_bench.json]"""
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
    fn()  # warm-up (first launches, buffers allocated on the first sample)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def summary(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t)), "count": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--modes", type=int, nargs="+", default=[1, 4, 32])
    ap.add_argument("--n", type=int, default=1_000_000, help="nodes (half of each type)")
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--blocks", type=int, default=32, help="blocks per type")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_summary_bench.json"))
    args = ap.parse_args()
    na = nb = args.n // 2
    k, chains = args.blocks, args.chains
    a, b = syn.planted_edges(na, nb, args.edges, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), na + nb)
    truth = syn.contiguous_labels(na, nb, k, k)
    m = B.BlockModel(truth, syn.types_vector(na, nb), 2 * k, k, k, 1.0, (rp, cl), n_chains=chains, seed=1)
    st = np.random.default_rng(0)
    for c in range(chains):
        perm = np.concatenate([st.permutation(k), k + st.permutation(k)]).astype(np.uint32)
        m.set_memberships(perm[truth], chain=c)
    m.init_bisbm()
    m.run_sweeps(2)
    cells = k * k + 4 * k
    out = {"tool": "block_summary_bench", "shape": "%d+%d" % (k, k), "n": na + nb, "edges": args.edges, "chains": chains,
           "rounds": args.rounds, "reps": args.reps, "block_state_bytes_per_sample": chains * cells * 4,
           "split": os.environ.get("BISBM_BLOCK_SPLIT", "library")}
    times = {}
    for _ in range(args.rounds):
        for M in args.modes:
            for name, on, keep in (("off", False, False), ("sums", True, False), ("sums_keep_last", True, True)):
                m.block_sums_set(False)
                m.marginals_reset()
                if M == 1:
                    m.marginals_set_modes(None)
                    m.marginals_set_alignment(True)
                else:
                    m.marginals_set_modes(np.arange(chains, dtype=np.uint32) % M, n_modes=M)
                if on:
                    m.block_sums_set(True, keep_last=keep)
                times.setdefault("%s_%s_ms" % ("pooled" if M == 1 else "modes_%d" % M, name), []).extend(timed(m.marginals_accumulate, args.reps))
                if on:
                    assert sum(m.block_sums(g)["terms"] for g in range(M)) == (args.reps + 1) * chains
    out.update({key: summary(t) for key, t in times.items()})
    for M in args.modes:
        pre = "pooled" if M == 1 else "modes_%d" % M
        off = out[pre + "_off_ms"]["median"]
        out[pre + "_added_ms"] = {"sums": out[pre + "_sums_ms"]["median"] - off, "sums_keep_last": out[pre + "_sums_keep_last_ms"]["median"] - off}
    m.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
