"""Cost of the heat-bath sweeps and what the greedy polishing gains (include/bisbm.h, "Heat-bath sweeps and greedy polishing") at
BASELINE configs[2] -- N = 10^6 (5e5 + 5e5), E = 10^7, 32 + 32 blocks -- in ONE process on ONE handle:
  (a) per temperature of --temps: one MH sweep (bisbm_last_sweep_timing: the kernel's time) and one heat-bath sweep at
      beta = 1 / T (host clock around the call, which returns after its kernel has finished), alternating, medians of --reps
      after a warm-up round of both; ns per (chain x step) of each, their ratio, and how many steps moved a node;
  (b) the standard anneal (--burn sweeps at T = 1, then an exponential cooling of --cool sweeps from T = 1 down to T = 1e-4),
      then polish(--cap): sweeps and moves until a chain has settled -- reported for the chains that settled within the cap, with
      their number beside it; a chain cut at the cap is told from one that settled in its last sweep by one more greedy sweep --
      and the description length it gains.
Writes profiles/heatbath_bench.json and prints it.  Every step runs under a time limit of its own (--limit seconds, a
watchdog thread: the library's calls release the interpreter; it prints a line every minute while a step runs): a step that
runs into it ends the process there with status 3, after writing what it has -- nothing more is started on the device after a
step that hung.  One polish call runs up to --cap greedy sweeps of ~10 s each at the default size: --limit is sized for that.

    python tools/heatbath_bench.py [--quick] [--chains 1024] [--temps 1 0.5] [--reps 3] [--burn 10] [--cool 20] [--cap 45] [--limit 600]"""
import argparse
import importlib
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = importlib.import_module("bipartitesbm-mcmc_amd")
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

OUT = {}
OUT_PATH = [None]


def write_out():
    os.makedirs(os.path.dirname(OUT_PATH[0]), exist_ok=True)
    with open(OUT_PATH[0], "w") as f:
        json.dump(OUT, f)
        f.write("\n")
    print(json.dumps(OUT), flush=True)


def _gave_up(what):
    OUT["timed_out"] = what
    write_out()
    os._exit(3)  # (the step hung: nothing more is started on the device, the handle is not torn down)


def timed(limit, what, fn):
    """(ms of fn(), its result) under its own time limit"""
    dog = threading.Timer(limit, _gave_up, [what])
    dog.daemon = True
    dog.start()
    done = threading.Event()

    def still_running():
        while not done.wait(60):
            print("... %s: still running" % what, flush=True)
    threading.Thread(target=still_running, daemon=True).start()
    try:
        t0 = time.perf_counter()
        res = fn()
        return (time.perf_counter() - t0) * 1e3, res
    finally:
        done.set()
        dog.cancel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a 10^5-node graph instead of configs[2] (a first look)")
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--temps", type=float, nargs="+", default=[1.0, 0.5])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--burn", type=int, default=10)
    ap.add_argument("--cool", type=int, default=20)
    ap.add_argument("--cap", type=int, default=45, help="the largest number of greedy sweeps")
    ap.add_argument("--limit", type=int, default=600, help="seconds every step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heatbath_bench.json"))
    args = ap.parse_args()
    OUT_PATH[0] = args.out
    na = nb = 50_000 if args.quick else 500_000
    E, k, C = 20 * na, 32, args.chains
    n = na + nb
    a, b = syn.planted_edges(na, nb, E, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), n)
    OUT.update({"n": n, "edges": E, "blocks": "%d+%d" % (k, k), "chains": C, "reps": args.reps, "sweeps": {}})
    _, m = timed(args.limit, "create", lambda: B.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k, 1.0,
                                                            (rp, cl), n_chains=C, seed=1))
    timed(args.limit, "shuffle", m.shuffle_bisbm)
    timed(args.limit, "warm-up sweeps", lambda: m.run_sweeps(2))  # (first launches, the pass-depth policy's first look)

    # (a) an MH sweep beside a heat-bath sweep of the same handle at the same temperature, alternating
    for T in args.temps:
        mh_ms, hb_ms, mh_acc, hb_moved = [], [], [], []
        for rep in range(args.reps + 1):
            timed(args.limit, "MH sweep at T = %g" % T, lambda: m.run_sweeps(1, T))
            mh_ms.append(m.last_sweep_timing()[0])
            mh_acc.append(float(m.last_counts()[0].sum()) / (C * n))
            ms, moved = timed(args.limit, "heat-bath sweep at T = %g" % T, lambda: m.heatbath_sweeps(1, 1.0 / T))
            hb_ms.append(ms)
            hb_moved.append(float(moved.sum()) / (C * n))
        r = OUT["sweeps"]["%g" % T] = {"T": T, "beta": 1.0 / T, "mh_ms_all": mh_ms[1:], "heatbath_ms_all": hb_ms[1:]}
        r["mh_ms"], r["heatbath_ms"] = float(np.median(mh_ms[1:])), float(np.median(hb_ms[1:]))
        r["mh_ns_per_chain_step"] = r["mh_ms"] * 1e6 / (C * n)
        r["heatbath_ns_per_chain_step"] = r["heatbath_ms"] * 1e6 / (C * n)
        r["heatbath_over_mh"] = r["heatbath_ms"] / r["mh_ms"]
        r["mh_accepted_per_step"] = float(np.median(mh_acc[1:]))  # (accepted proposals, stays among them)
        r["heatbath_moved_per_step"] = float(np.median(hb_moved[1:]))
        write_out()

    # (b) the standard anneal, then polish
    mh = B.MetropolisHasting()
    p = OUT["polish"] = {"burn_sweeps": args.burn, "cool_sweeps": args.cool, "cap": args.cap}
    p["anneal_ms"] = timed(args.limit, "burn-in", lambda: mh.anneal(m, B.constant_schedule, [1.0], args.burn * n, 1 << 60))[0]
    rate = 1e-4 ** (1.0 / (args.cool * n))
    p["anneal_ms"] += timed(args.limit, "cooling", lambda: mh.anneal(m, B.exponential_schedule, [1.0, rate], args.cool * n, 1 << 60))[0]
    _, before = timed(args.limit, "entropy", m.entropy)
    p["polish_ms"], (moved, sweeps) = timed(args.limit, "polish", lambda: m.polish(args.cap))
    _, after = timed(args.limit, "entropy", m.entropy)
    _, (again, one) = timed(args.limit, "one more greedy sweep", lambda: m.polish(1))
    gain = before - after
    settled = (sweeps < args.cap) | (again == 0)  # (stopped early, or the sweep after the cap's last one moved nothing)
    p.update({"settled_chains": int(settled.sum()), "cut_at_the_cap": int((~settled).sum()),
              "description_length_before_mean": float(before.mean()), "description_length_before_best": float(before.min()),
              "description_length_after_mean": float(after.mean()), "description_length_after_best": float(after.min()),
              "gain_min": float(gain.min()), "gain_mean": float(gain.mean()), "gain_max": float(gain.max()),
              "gain_mean_relative": float((gain / before).mean()),
              "polish_ms_per_sweep": p["polish_ms"] / float(sweeps.max()),
              "one_more_sweep_moves": int(again.sum()), "one_more_sweep_moves_max": int(again.max())})
    if settled.any():  # sweeps and moves until settled: of the chains that did settle
        sw, mv = sweeps[settled], moved[settled]
        p.update({"sweeps_min": int(sw.min()), "sweeps_median": float(np.median(sw)), "sweeps_max": int(sw.max()),
                  "sweeps_histogram": {str(int(k)): int(v) for k, v in zip(*np.unique(sw, return_counts=True))},
                  "moves_min": int(mv.min()), "moves_median": float(np.median(mv)), "moves_max": int(mv.max()),
                  "moves_per_node_median": float(np.median(mv)) / n})
    timed(args.limit, "close", m.close)
    write_out()


if __name__ == "__main__":
    main()
