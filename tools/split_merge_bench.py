"""Cost and acceptance of the split and merge moves (include/bisbm.h, "Split and merge moves") at BASELINE configs[2] -- N = 10^6
(5e5 + 5e5), E = 10^7, 32 + 32 blocks -- in ONE process on ONE handle, after the short anneal of tools/heatbath_bench.py (--burn
sweeps at T = 1, then an exponential cooling of --cool sweeps from T = 1 down to T = 1e-4) and --settle MH sweeps at T = 1.  Per
scan count of --scans, first --moves pair reshuffles per chain (the chains still share one shape), then --moves split / merge moves
per chain, both at beta = 1 with the host clock around the call:
  ms per move for all chains; ns per (chain x member x evaluated scan) -- a split or a merge evaluates scans + 1 scans (the launch
  scans and the forward or the forced pass) where a reshuffle evaluates scans + 2; the members are the mean over the evaluated
  moves of the call's last records, the figure divides the whole call by them, so it carries the copy into the scratch, the
  transits, the read-back and the regrouping as well; the acceptance of splits and of merges at T = 1 (refused proposals
  count as proposed); the share of the call spent regrouping (bisbm_split_merge_get_timing); the groups the handle ends with.
Writes profiles/split_merge_bench.json and prints it.  Every step runs under a time limit of its own, as in
tools/heatbath_bench.py: a step that runs into it ends the process with status 3 after writing what it has.

    python tools/split_merge_bench.py [--quick] [--chains 1024] [--scans 0 1 3] [--moves 4] [--limit 600]"""
import argparse
import importlib
import os
import sys

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
    ap.add_argument("--limit", type=int, default=600, help="seconds every step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_merge_bench.json"))
    args = ap.parse_args()
    hb.OUT_PATH[0] = args.out
    na = nb = 50_000 if args.quick else 500_000
    E, k, C = 20 * na, 32, args.chains
    n = na + nb
    a, b = syn.planted_edges(na, nb, E, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), n)
    OUT.update({"n": n, "edges": E, "blocks_at_the_start": "%d+%d" % (k, k), "chains": C, "moves_per_call": args.moves, "reshuffle": {}, "split_merge": {}})
    _, m = timed(args.limit, "create", lambda: B.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k, 1.0,
                                                            (rp, cl), n_chains=C, seed=1))
    timed(args.limit, "shuffle", m.shuffle_bisbm)
    mh = B.MetropolisHasting()
    timed(args.limit, "burn-in", lambda: mh.anneal(m, B.constant_schedule, [1.0], args.burn * n, 1 << 60))
    rate = 1e-4 ** (1.0 / (args.cool * n))
    timed(args.limit, "cooling", lambda: mh.anneal(m, B.exponential_schedule, [1.0, rate], args.cool * n, 1 << 60))
    timed(args.limit, "MH sweeps at T = 1", lambda: m.run_sweeps(args.settle))

    # the pair reshuffles first: the chains still share one shape
    timed(args.limit, "first reshuffle call", lambda: m.reshuffle(1, 0, 1.0))  # (the scratch is allocated here)
    for scans in args.scans:
        ms, acc = timed(args.limit, "%d reshuffles with %d scan(s)" % (args.moves, scans), lambda: m.reshuffle(args.moves, scans, 1.0))
        members = float(np.mean([r["M"] for r in m.reshuffle_last()]))
        OUT["reshuffle"]["%d" % scans] = {"scans": scans, "ms_per_move": ms / args.moves, "acceptance": float(acc.sum()) / (C * args.moves),
                                          "members_mean_last_move": members, "evaluated_scans": scans + 2,
                                          "ns_per_chain_member_scan": ms * 1e6 / (C * args.moves * members * (scans + 2))}
        write_out()

    # the split and merge moves
    timed(args.limit, "first split / merge call", lambda: m.split_merge(1, 0, 1.0))  # (the scratch is allocated here)
    for scans in args.scans:
        before = m.split_merge_total().sum(axis=0).astype(np.int64)
        ms, acc = timed(args.limit, "%d split / merge moves with %d scan(s)" % (args.moves, scans), lambda: m.split_merge(args.moves, scans, 1.0))
        tot = m.split_merge_total().sum(axis=0).astype(np.int64) - before
        call_ms, regroup_ms = m.split_merge_timing()
        evaluated = [r["M"] for r in m.split_merge_last() if r["refused"] == B.SM_EVALUATED]
        members = float(np.mean(evaluated)) if evaluated else 0.0
        share = len(evaluated) / float(C)  # of the last move's proposals, the part that was evaluated
        OUT["split_merge"]["%d" % scans] = {
            "scans": scans, "ms_per_move": ms / args.moves, "evaluated_scans": scans + 1, "members_mean_last_move_evaluated": members,
            "evaluated_share_last_move": share,
            "ns_per_chain_member_scan": (ms * 1e6 / (C * args.moves * share * members * (scans + 1))) if members and share else None,
            "splits_proposed": int(tot[0]), "splits_accepted": int(tot[1]), "merges_proposed": int(tot[2]), "merges_accepted": int(tot[3]),
            "split_acceptance": float(tot[1]) / max(int(tot[0]), 1), "merge_acceptance": float(tot[3]) / max(int(tot[2]), 1),
            "call_ms_library_clock": call_ms, "regroup_ms": regroup_ms, "regroup_share_of_call": regroup_ms / call_ms if call_ms else None,
            "groups_after": int(len(set(m.chain_groups().tolist()))), "shapes_after": int(len({m.ka_kb(c) for c in range(C)}))}
        write_out()
    m.close()


if __name__ == "__main__":
    main()
