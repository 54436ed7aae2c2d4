"""Cost of the fold-in queries (include/bisbm.h, "Fold-in queries") at BASELINE configs[2] -- N = 10^6 (5e5 + 5e5), E = 10^7,
32 + 32 blocks, 1024 chains -- for Q = 16 and 256 type-a virtual nodes with lists of d = 8 and d = 64 neighbours.  Writes
profiles/foldin_bench.json and prints it.  In ONE process, host clock around calls that return after their kernels have
finished, medians of --reps after a warm-up round, the routes alternated:
  * ms of one foldin_accumulate with the recommend rows only (Q x 5e5 cells per chain: the cells of the yardstick), with the
    similar rows only, and with both kinds;
  * one query_scores_accumulate of the same build on Q existing type-a nodes: the yardstick, which does strictly more per cell
    (two table lookups and an f64 divide against one lookup and a multiply).  All are reported per (node x candidate x chain)
    cell;
  * ms of foldin_topk(k = 100) of either kind;
  * a check on the way: a recommend row's sum over the candidates is terms x d_q to 1e-9 relative (every block of the bench
    graph has edges);
  * ms of one sweep of the same handle, for scale.
Every timed step runs under a time limit of its own (--limit seconds, a watchdog thread: the library's calls release the
interpreter): a step that runs into it ends the process there with status 3, after writing what it has -- nothing more is
started on the device after a step that hung.

    python tools/foldin_bench.py [--quick] [--chains 1024] [--queries 16 256] [--lengths 8 64] [--reps 3] [--limit 120]"""
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
    ap.add_argument("--queries", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--lengths", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--limit", type=int, default=120, help="seconds every timed step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "foldin_bench.json"))
    args = ap.parse_args()
    OUT_PATH[0] = args.out
    na = nb = 50_000 if args.quick else 500_000
    E, k, C = 20 * na, 32, args.chains
    a, b = syn.planted_edges(na, nb, E, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), na + nb)
    made = []
    timed(args.limit, "create", lambda: made.append(B.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k, 1.0,
                                                                 (rp, cl), n_chains=C, seed=1)))
    m = made[0]
    timed(args.limit, "shuffle", m.shuffle_bisbm)
    timed(args.limit, "warm-up sweeps", lambda: m.run_sweeps(2))  # (first launches, the pass-depth policy's first look)
    out = OUT
    out.update({"n": na + nb, "edges": E, "blocks": "%d+%d" % (k, k), "chains": C, "candidates": nb, "k": args.k, "reps": args.reps,
                "alpha": args.alpha, "cand_tile": B.FOLDIN_CAND_TILE, "node_tile": B.FOLDIN_TILE, "runs": {}})
    out["sweep_ms"] = float(np.median([timed(args.limit, "sweep", lambda: m.run_sweeps(1)) for _ in range(args.reps)]))
    rs = np.random.default_rng(5)
    for Q in args.queries:
        queries = np.sort(rs.choice(na, Q, replace=False))
        timed(args.limit, "query_scores_set Q=%d" % Q, lambda: m.query_scores_set(queries))
        for d in args.lengths:
            tag = "Q=%d d=%d" % (Q, d)
            r = out["runs"][tag] = {"Q": Q, "d": d, "cells_per_kind": Q * nb * C}
            nodes = [("a", (na + rs.integers(0, nb, d)).tolist()) for _ in range(Q)]
            t = {}
            for name, what in (("recommend", B.FOLDIN_RECOMMEND), ("similar", B.FOLDIN_SIMILAR), ("both", B.FOLDIN_RECOMMEND | B.FOLDIN_SIMILAR)):
                r["set_%s_ms" % name] = timed(args.limit, "foldin_set %s %s" % (name, tag), lambda: m.foldin_set(nodes, args.alpha, what=what))
                t[name] = []
                if name == "recommend":
                    t["query_scores"] = []
                for rep in range(args.reps + 1):  # (the routes alternated; the first round warms up and is dropped)
                    t[name].append(timed(args.limit, "foldin_accumulate %s %s" % (name, tag), m.foldin_accumulate))
                    if name == "recommend":
                        t["query_scores"].append(timed(args.limit, "query_scores_accumulate %s" % tag, m.query_scores_accumulate))
            for name, ms in t.items():
                r[name + "_ms_all"], r[name + "_ms"] = ms[1:], float(np.median(ms[1:]))
                r[name + "_ps_per_cell"] = r[name + "_ms"] * 1e9 / (r["cells_per_kind"] * (2 if name == "both" else 1))
            r["recommend_over_query_scores"] = r["recommend_ms"] / r["query_scores_ms"]
            r["both_over_sweep"] = r["both_ms"] / out["sweep_ms"]
            for name, what in (("recommend", B.FOLDIN_RECOMMEND), ("similar", B.FOLDIN_SIMILAR)):
                tk = [timed(args.limit, "foldin_topk %s %s" % (name, tag), lambda: m.foldin_topk(what, args.k, name == "recommend"))
                      for _ in range(args.reps + 1)][1:]
                r["topk_%s_ms_all" % name], r["topk_%s_ms" % name] = tk, float(np.median(tk))
            r["sum_bytes"] = 2 * 8 * Q * nb
            got = {}
            timed(args.limit, "foldin_scores %s" % tag, lambda: got.update(row=m.foldin_scores(Q - 1, B.FOLDIN_RECOMMEND)))
            row, terms = got["row"]
            r["terms"] = int(terms)
            r["row_sum_over_terms_d"] = float(row.sum() / (terms * d))
            r["row_sum_ok"] = bool(abs(r["row_sum_over_terms_d"] - 1.0) < 1e-9)
            timed(args.limit, "foldin_set() %s" % tag, lambda: m.foldin_set([]))
        timed(args.limit, "query_scores_set() Q=%d" % Q, lambda: m.query_scores_set(np.zeros(0, dtype=np.int64)))
    write_out()
    timed(args.limit, "close", m.close)


if __name__ == "__main__":
    main()
