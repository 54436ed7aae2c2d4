"""Cost of a chain-trace record and the mixing of the three samplers (include/bisbm.h, "Chain traces") at BASELINE configs[2] --
N = 10^6 (5e5 + 5e5), E = 10^7, 32 + 32 blocks -- in ONE process on ONE handle, after the short anneal of tools/heatbath_bench.py
(--burn sweeps at T = 1, then an exponential cooling of --cool sweeps from T = 1 down to T = 1e-4) and --settle MH sweeps at T = 1:
  (a) per depth of --depths: the ring is filled, then one record with every age held is timed (host clock around the call, which
      returns after its kernels have finished and the sums are on the host): ms, ps per (chain x age x node), the bytes of the
      ring; beside it one MH sweep of the same handle (bisbm_last_sweep_timing);
  (b) from the labels the anneal left, equal wall-time budgets (--budget seconds each) of MH sweeps, heat-bath sweeps, and MH sweeps
      with --inter pair reshuffles (3 scans) after every block: a record after every block (--mh_block MH sweeps, or one heat-bath
      sweep) at depth --depth; per arm the mean VI and the mean share of relabelled nodes at every lag, the lag in seconds (lag x
      the mean seconds per block, records included), and tau_S / split R-hat of the description length (bisbm_trace_summary,
      window factor 5) where the arm made at least 4 records.
Writes profiles/trace_bench.json and prints it.  Every step runs under a time limit of its own, as in tools/heatbath_bench.py: a
step that runs into it ends the process with status 3 after writing what it has.

    python tools/trace_bench.py [--quick] [--chains 1024] [--depths 1 4 16] [--depth 16] [--budget 60] [--mh_block 1] [--inter 1]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
B = importlib.import_module("bipartitesbm-mcmc_amd")
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")
hb = importlib.import_module("heatbath_bench")  # (its watchdog and its output file)
OUT, timed, write_out = hb.OUT, hb.timed, hb.write_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a 10^5-node graph instead of configs[2] (a first look)")
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--depths", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--depth", type=int, default=16, help="the depth of the mixing runs")
    ap.add_argument("--budget", type=float, default=60.0, help="seconds of every arm of the mixing runs")
    ap.add_argument("--mh_block", type=int, default=1, help="MH sweeps between two records")
    ap.add_argument("--inter", type=int, default=1, help="pair reshuffles after every block of the third arm")
    ap.add_argument("--burn", type=int, default=10)
    ap.add_argument("--cool", type=int, default=20)
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--limit", type=int, default=600, help="seconds every step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_bench.json"))
    args = ap.parse_args()
    hb.OUT_PATH[0] = args.out
    na = nb = 50_000 if args.quick else 500_000
    E, k, C = 20 * na, 32, args.chains
    n = na + nb
    a, b = syn.planted_edges(na, nb, E, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), n)
    OUT.update({"n": n, "edges": E, "blocks": "%d+%d" % (k, k), "chains": C, "record": {}, "mixing": {}})
    _, m = timed(args.limit, "create", lambda: B.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k, 1.0,
                                                            (rp, cl), n_chains=C, seed=1))
    timed(args.limit, "shuffle", m.shuffle_bisbm)
    mh = B.MetropolisHasting()
    timed(args.limit, "burn-in", lambda: mh.anneal(m, B.constant_schedule, [1.0], args.burn * n, 1 << 60))
    rate = 1e-4 ** (1.0 / (args.cool * n))
    timed(args.limit, "cooling", lambda: mh.anneal(m, B.exponential_schedule, [1.0, rate], args.cool * n, 1 << 60))
    timed(args.limit, "MH sweeps at T = 1", lambda: m.run_sweeps(args.settle))
    labels = [m.get_memberships(c) for c in range(C)]

    # (a) one record with every age held, beside a sweep of the same handle
    for depth in args.depths:
        timed(args.limit, "ring of depth %d" % depth, lambda: m.trace_set(depth))
        for _ in range(depth):  # (a sweep between the snapshots: the tables are those of chains that move)
            timed(args.limit, "MH sweep", lambda: m.run_sweeps(1))
            timed(args.limit, "record", m.trace_record)
        timed(args.limit, "MH sweep", lambda: m.run_sweeps(1))
        sweep_ms = m.last_sweep_timing()[0]
        ms, _ = timed(args.limit, "record at depth %d" % depth, m.trace_record)
        OUT["record"]["%d" % depth] = {"depth": depth, "ms": ms, "ps_per_chain_age_node": ms * 1e9 / (C * depth * float(n)),
                                       "ring_bytes": depth * C * ((n + 255) // 256 * 256), "mh_sweep_ms": sweep_ms,
                                       "mean_changed_at_lag_1": float(m.trace_lags()["changed"][:, 0].mean())}
        write_out()
    m.trace_set(0)

    # (b) equal wall time: MH sweeps, heat-bath sweeps, MH sweeps with reshuffles, each from the labels of the anneal
    def restore():
        for c in range(C):
            m.set_memberships(labels[c], chain=c)
        m.init_bisbm()
    arms = {"mh": lambda: m.run_sweeps(args.mh_block),
            "heatbath": lambda: m.heatbath_sweeps(1, 1.0),
            "mh_reshuffle": lambda: (m.run_sweeps(args.mh_block), m.reshuffle(args.inter, 3, 1.0))}
    for name, block in arms.items():
        timed(args.limit, "labels of the anneal", restore)
        timed(args.limit, "ring of depth %d" % args.depth, lambda: m.trace_set(args.depth))
        timed(args.limit, "record", m.trace_record)
        t0, blocks = time.perf_counter(), 0
        while blocks == 0 or (time.perf_counter() - t0) * (blocks + 1) / blocks <= args.budget:
            timed(args.limit, "%s block" % name, block)
            timed(args.limit, "record", m.trace_record)
            blocks += 1
        spent = time.perf_counter() - t0
        lags = m.trace_lags()
        S = m.trace_series("S")
        held = lags["pairs"] > 0
        res = {"seconds": spent, "blocks": blocks, "seconds_per_block": spent / blocks, "records": lags["records"],
               "lag_seconds": [(i + 1) * spent / blocks for i in range(args.depth) if held[i]],
               "vi_mean": [float(x) for x in lags["vi_mean"][:, held].mean(axis=0)],
               "changed_mean": [float(x) for x in lags["changed"][:, held].mean(axis=0)],
               "description_length_mean_first": float(S[0].mean()), "description_length_mean_last": float(S[-1].mean())}
        if lags["records"] >= 4:
            tau, window, rhat = B.trace_summary(S)
            res.update({"tau_S_blocks_median": float(np.median(tau)), "tau_S_seconds_median": float(np.median(tau)) * spent / blocks,
                        "chains_with_window_at_half": int((window >= lags["records"] // 2).sum()), "rhat_S": float(rhat)})
        OUT["mixing"][name] = res
        write_out()
    m.close()


if __name__ == "__main__":
    main()
