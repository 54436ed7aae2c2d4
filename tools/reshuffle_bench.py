"""Cost and acceptance of the pair reshuffles (include/bisbm.h, "Pair reshuffles") at BASELINE configs[2] -- N = 10^6 (5e5 + 5e5),
E = 10^7, 32 + 32 blocks -- in ONE process on ONE handle, after the short anneal of tools/heatbath_bench.py (--burn sweeps at
T = 1, then an exponential cooling of --cool sweeps from T = 1 down to T = 1e-4) and --settle MH sweeps at T = 1:
  (a) per scan count of --scans: --moves moves per chain at beta = 1 (host clock around the call, which returns after its kernel
      has finished): the acceptance rate, ms per move, and ns per (chain x member x scan) with (scans + 2) evaluated scans per
      move -- the launch scans, the reverse pass, the forward pass -- and the members taken from the records of the last move
      (about 2 n / K); beside them one MH sweep (bisbm_last_sweep_timing) and one heat-bath sweep of the same handle in ns per
      (chain x step);
  (b) the mean and the best description length after equal wall time of MH sweeps at T = 1 alone and of MH sweeps with --inter
      reshuffles (3 scans) after every sweep: the interleaved run first, --rounds rounds, on the clock; then as many plain MH
      sweeps as fit the same time, from the same labels.
Writes profiles/reshuffle_bench.json and prints it.  Every step runs under a time limit of its own, as in
tools/heatbath_bench.py: a step that runs into it ends the process with status 3 after writing what it has.

    python tools/reshuffle_bench.py [--quick] [--chains 1024] [--scans 0 1 3] [--moves 4] [--rounds 3] [--inter 2] [--limit 600]"""
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
    ap.add_argument("--scans", type=int, nargs="+", default=[0, 1, 3])
    ap.add_argument("--moves", type=int, default=4)
    ap.add_argument("--burn", type=int, default=10)
    ap.add_argument("--cool", type=int, default=20)
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inter", type=int, default=2)
    ap.add_argument("--limit", type=int, default=600, help="seconds every step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reshuffle_bench.json"))
    args = ap.parse_args()
    hb.OUT_PATH[0] = args.out
    na = nb = 50_000 if args.quick else 500_000
    E, k, C = 20 * na, 32, args.chains
    n = na + nb
    a, b = syn.planted_edges(na, nb, E, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), n)
    OUT.update({"n": n, "edges": E, "blocks": "%d+%d" % (k, k), "chains": C, "moves_per_call": args.moves, "scans": {}})
    _, m = timed(args.limit, "create", lambda: B.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k, 1.0,
                                                            (rp, cl), n_chains=C, seed=1))
    timed(args.limit, "shuffle", m.shuffle_bisbm)
    mh = B.MetropolisHasting()
    timed(args.limit, "burn-in", lambda: mh.anneal(m, B.constant_schedule, [1.0], args.burn * n, 1 << 60))
    rate = 1e-4 ** (1.0 / (args.cool * n))
    timed(args.limit, "cooling", lambda: mh.anneal(m, B.exponential_schedule, [1.0, rate], args.cool * n, 1 << 60))
    timed(args.limit, "MH sweeps at T = 1", lambda: m.run_sweeps(args.settle))

    # (a) the moves, beside an MH sweep and a heat-bath sweep of the same handle
    timed(args.limit, "MH sweep", lambda: m.run_sweeps(1))
    OUT["mh_ns_per_chain_step"] = m.last_sweep_timing()[0] * 1e6 / (C * n)
    ms, _ = timed(args.limit, "heat-bath sweep", lambda: m.heatbath_sweeps(1, 1.0))
    OUT["heatbath_ns_per_chain_step"] = ms * 1e6 / (C * n)
    write_out()
    timed(args.limit, "first reshuffle call", lambda: m.reshuffle(1, 0, 1.0))  # (the scratch is allocated here)
    for scans in args.scans:
        ms, acc = timed(args.limit, "%d moves with %d scan(s)" % (args.moves, scans), lambda: m.reshuffle(args.moves, scans, 1.0))
        members = float(np.mean([r["M"] for r in m.reshuffle_last()]))
        OUT["scans"]["%d" % scans] = {"scans": scans, "ms": ms, "ms_per_move": ms / args.moves,
                                      "acceptance": float(acc.sum()) / (C * args.moves), "members_mean_last_move": members,
                                      "ns_per_chain_member_scan": ms * 1e6 / (C * args.moves * members * (scans + 2))}
        write_out()

    # (b) equal wall time: MH sweeps with reshuffles in between, then MH sweeps alone from the same labels
    labels = [m.get_memberships(c) for c in range(C)]
    _, S0 = timed(args.limit, "entropy", m.entropy)
    t0 = time.perf_counter()
    accepted = 0
    for _ in range(args.rounds):
        timed(args.limit, "MH sweep", lambda: m.run_sweeps(1))
        accepted += int(timed(args.limit, "reshuffles", lambda: m.reshuffle(args.inter, 3, 1.0))[1].sum())
    budget = time.perf_counter() - t0
    _, S_with = timed(args.limit, "entropy", m.entropy)
    for c in range(C):
        m.set_memberships(labels[c], chain=c)
    timed(args.limit, "init", m.init_bisbm)
    t0, plain = time.perf_counter(), 0
    while plain == 0 or (time.perf_counter() - t0) * (plain + 1) / plain <= budget:
        timed(args.limit, "MH sweep", lambda: m.run_sweeps(1))
        plain += 1
    spent = time.perf_counter() - t0
    _, S_plain = timed(args.limit, "entropy", m.entropy)
    OUT["equal_wall_time"] = {"seconds_with_reshuffles": budget, "seconds_mh_alone": spent, "rounds": args.rounds,
                              "reshuffles_per_round": args.inter, "reshuffle_acceptance": accepted / float(C * args.rounds * args.inter),
                              "mh_sweeps_alone": plain,
                              "description_length_start_mean": float(S0.mean()), "description_length_start_best": float(S0.min()),
                              "description_length_with_reshuffles_mean": float(S_with.mean()), "description_length_with_reshuffles_best": float(S_with.min()),
                              "description_length_mh_alone_mean": float(S_plain.mean()), "description_length_mh_alone_best": float(S_plain.min())}
    write_out()
    m.close()


if __name__ == "__main__":
    main()
