"""Cost of the node conditionals (include/bisbm.h, "Node conditionals") at BASELINE configs[2] -- N = 10^6 (5e5 + 5e5), E = 10^7,
32 + 32 blocks -- in ONE process, host clock around calls that return after their kernels have finished, medians of --reps
after a warm-up round:
  (a) 4096 queries x all chains of a 1024-chain handle;
  (b) every node x 16 chains (a handle with 16 chains);
  (c) (a) with a reference set: the soft marginals on top (the alignment of every chain and the scatter of the rows).
Every case reports ms per sample, ps per (chain x query x target) and the ratio to one sweep of the same handle timed in the
same process.  Writes profiles/conditionals_bench.json and prints it.
Every timed step runs under a time limit of its own (--limit seconds, a watchdog thread: the library's calls release the
interpreter): a step that runs into it ends the process there with status 3, after writing what it has -- nothing more is
started on the device after a step that hung.

    python tools/conditionals_bench.py [--quick] [--chains 1024] [--few 16] [--queries 4096] [--reps 3] [--limit 120]"""
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
    """ms of fn() under its own time limit"""
    dog = threading.Timer(limit, _gave_up, [what])
    dog.daemon = True
    dog.start()
    try:
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3
    finally:
        dog.cancel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a 10^5-node graph instead of configs[2] (a first look)")
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--few", type=int, default=16, help="chains of the handle of case (b)")
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds every timed step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conditionals_bench.json"))
    args = ap.parse_args()
    OUT_PATH[0] = args.out
    na = nb = 50_000 if args.quick else 500_000
    E, k = 20 * na, 32
    a, b = syn.planted_edges(na, nb, E, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), na + nb)
    OUT.update({"n": na + nb, "edges": E, "blocks": "%d+%d" % (k, k), "reps": args.reps, "runs": {}})

    def handle(C):
        made = []
        timed(args.limit, "create %d" % C, lambda: made.append(B.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k,
                                                                           1.0, (rp, cl), n_chains=C, seed=1)))
        m = made[0]
        timed(args.limit, "shuffle", m.shuffle_bisbm)
        timed(args.limit, "warm-up sweeps", lambda: m.run_sweeps(2))  # (first launches, the pass-depth policy's first look)
        sweep = float(np.median([timed(args.limit, "sweep", lambda: m.run_sweeps(1)) for _ in range(args.reps)]))
        return m, sweep

    def case(tag, m, sweep_ms, C, Q, reference):
        r = OUT["runs"][tag] = {"chains": C, "queries": Q, "targets": k, "reference": bool(reference), "sweep_ms": sweep_ms,
                                "sweep_ns_per_step": sweep_ms * 1e6 / ((na + nb) * C)}
        if reference:
            got = []
            timed(args.limit, "get_memberships", lambda: got.append(m.get_memberships(0)))
            r["set_reference_ms"] = timed(args.limit, "set_reference " + tag, lambda: m.conditionals_set_reference(got[0]))
        ms = [timed(args.limit, "conditionals_accumulate " + tag, m.conditionals_accumulate) for _ in range(args.reps + 1)][1:]
        r["ms_all"], r["ms"] = ms, float(np.median(ms))
        r["ps_per_chain_query_target"] = r["ms"] * 1e9 / (C * Q * k)
        r["ns_per_chain_query"] = r["ms"] * 1e6 / (C * Q)
        r["over_sweep"] = r["ms"] / sweep_ms
        got = {}
        timed(args.limit, "stats " + tag, lambda: got.update(st=m.conditionals_stats()))
        st = got["st"]
        r["terms"] = int(st["terms"])
        r["mean_stay"] = float(st["stay"].sum() / (st["terms"] * Q))
        r["mean_entropy"] = float(st["entropy"].sum() / (st["terms"] * Q))
        if reference:
            timed(args.limit, "marginals " + tag, lambda: got.update(pr=m.conditionals_marginals()))
            prob, terms = got["pr"]
            r["row_sum_over_terms_max_dev"] = float(np.abs(prob.sum(axis=1) / terms - 1.0).max())

    rs = np.random.default_rng(5)
    Q = min(args.queries, na + nb)
    queries = np.sort(rs.choice(na + nb, Q, replace=False)).astype(np.uint32)
    m, sweep = handle(args.chains)
    OUT["set_ms"] = timed(args.limit, "conditionals_set", lambda: m.conditionals_set(queries))
    case("a", m, sweep, args.chains, Q, False)
    case("c", m, sweep, args.chains, Q, True)
    timed(args.limit, "conditionals_set()", lambda: m.conditionals_set([]))
    timed(args.limit, "close", m.close)
    write_out()
    m, sweep = handle(args.few)
    timed(args.limit, "conditionals_set all", lambda: m.conditionals_set(None))
    case("b", m, sweep, args.few, na + nb, False)
    timed(args.limit, "close", m.close)
    write_out()


if __name__ == "__main__":
    main()
