"""Cost of the edge queries (include/bisbm.h, "Edge queries") at BASELINE configs[2] -- N = 10^6 (5e5 + 5e5), E = 10^7, 32 + 32
blocks, 1024 chains -- for Q = 1, 16 and 256 type-a queries (5e5 candidates each).  Writes profiles/edge_queries_bench.json and
prints it.  In ONE process, host clock around calls that return after their kernels have finished:
  * ms of one edge_queries_accumulate per Q, and of one edge_queries_topk(k = 100) with the neighbours left out;
  * ms of one query_scores_accumulate on the same queries (the plug-in score on the same layout);
  * for Q = 16 the LISTED route of the same build on the same Q x 5e5 enumerated ADD pairs: ms of edge_probs_set (upload, host
    sort, multiplicities) and of one edge_probs_accumulate, alternated with the dense call, at least 5 repeats; medians and
    ranges, both routes per (query x candidate x chain) term -- and a check on the way that the two hold the same bits;
  * ms of one sweep of the same handle, for scale.
Every timed step runs under a time limit of its own (--limit seconds, a watchdog thread: the library's calls release the
interpreter): a step that runs into it ends the process there with status 3, after writing what it has -- nothing more is
started on the device after a step that hung.

    python tools/edge_queries_bench.py [--quick] [--chains 1024] [--queries 1 16 256] [--reps 5] [--limit 120]"""
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


def spread(ms):
    return {"all": ms, "median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a 10^5-node graph instead of configs[2] (a first look)")
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--listed", type=int, nargs="+", default=[16], help="the Q for which the listed route is timed as well")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--limit", type=int, default=120, help="seconds every timed step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_queries_bench.json"))
    args = ap.parse_args()
    OUT_PATH[0] = args.out
    na = nb = 50_000 if args.quick else 500_000
    E, k, C = 20 * na, 32, args.chains
    a, b = syn.planted_edges(na, nb, E, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), na + nb)
    m = B.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k, 1.0, (rp, cl), n_chains=C, seed=1)
    m.shuffle_bisbm()
    m.run_sweeps(2)  # (warm-up: first launches, the pass-depth policy's first look)
    out = OUT
    out.update({"n": na + nb, "edges": E, "blocks": "%d+%d" % (k, k), "chains": C, "candidates": nb, "k": args.k, "reps": args.reps,
                "max_degree": int(m.max_degree), "query_tile": B.EDGE_QUERY_TILE, "by_Q": {}})
    out["sweep_ms"] = float(np.median([timed(args.limit, "sweep", lambda: m.run_sweeps(1)) for _ in range(args.reps)]))
    rs = np.random.default_rng(5)
    for Q in args.queries:
        r = out["by_Q"][str(Q)] = {"terms_per_sample": Q * nb * C, "sum_bytes": 8 * Q * nb}
        terms = r["terms_per_sample"]
        queries = np.sort(rs.choice(na, Q, replace=False))
        r["set_ms"] = timed(args.limit, "edge_queries_set Q=%d" % Q, lambda: m.edge_queries_set(queries))
        m.query_scores_set(queries)
        listed = Q in args.listed
        if listed:
            # the listed route on the same terms: all Q x nb ADD pairs, enumerated
            pairs = np.stack([np.repeat(queries, nb), np.tile(na + np.arange(nb), Q)], axis=1)
            r["listed_set_ms"] = timed(args.limit, "edge_probs_set Q=%d" % Q, lambda: m.edge_probs_set(pairs))
            del pairs
        dense, lst, plug = [], [], []
        for rep in range(args.reps + 1):  # (the routes alternated; the first round warms up and is dropped)
            dense.append(timed(args.limit, "edge_queries_accumulate Q=%d" % Q, m.edge_queries_accumulate))
            if listed:
                lst.append(timed(args.limit, "edge_probs_accumulate Q=%d" % Q, m.edge_probs_accumulate))
            plug.append(timed(args.limit, "query_scores_accumulate Q=%d" % Q, m.query_scores_accumulate))
        r["accumulate_ms"] = spread(dense[1:])
        r["ns_per_term"] = r["accumulate_ms"]["median"] * 1e6 / terms
        r["accumulate_over_sweep"] = r["accumulate_ms"]["median"] / out["sweep_ms"]
        r["query_scores_accumulate_ms"] = spread(plug[1:])
        r["query_scores_ns_per_term"] = r["query_scores_accumulate_ms"]["median"] * 1e6 / terms
        t = [timed(args.limit, "edge_queries_topk Q=%d" % Q, lambda: m.edge_queries_topk(args.k, True)) for _ in range(args.reps + 1)][1:]
        r["topk_ms"] = spread(t)
        if listed:
            r["listed_accumulate_ms"] = spread(lst[1:])
            r["listed_ns_per_term"] = r["listed_accumulate_ms"]["median"] * 1e6 / terms
            r["listed_over_dense"] = r["listed_accumulate_ms"]["median"] / r["accumulate_ms"]["median"]
            # (a check on the way: the two routes hold the same bits)
            e = m.edge_probs()
            row = m.edge_queries(Q - 1)
            r["terms"] = [int(e["terms"]), int(row["terms"])]
            r["last_row_bit_equal_to_the_listed_sums"] = bool((e["w_sum"][(Q - 1) * nb:].view(np.uint64) == row["w_sum"].view(np.uint64)).all())
            del e
            m.edge_probs_set(np.zeros((0, 2), dtype=np.int64))
        m.query_scores_set(np.zeros(0, dtype=np.int64))
        m.edge_queries_set(np.zeros(0, dtype=np.int64))
    write_out()
    m.close()


if __name__ == "__main__":
    main()
