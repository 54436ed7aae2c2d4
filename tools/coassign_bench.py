"""Cost of the co-assignment counts (include/bisbm.h, "Co-assignment") at BASELINE configs[2] -- N = 10^6 (5e5 + 5e5), E = 10^7,
32 + 32 blocks, 1024 chains -- for Q = 1, 16 and 256 type-a queries (5e5 candidates each).  Writes profiles/coassign_bench.json
and prints it.  In ONE process, host clock around calls that return after their kernels have finished:
  * ms of one coassign_accumulate per Q in the packed form (four byte labels compared as one word, byte-wide partials) and in
    the plain form (extract, compare and add every cell: BISBM_COASSIGN_FORM=plain, read at every call), alternated, and of one
    coassign_topk(k = 100);
  * for Q = 16 and 256 one query_scores_accumulate of the same build on the same queries, alternated with the two forms: the
    yardstick, which does strictly more per cell (two table lookups and an f64 divide).  All three are reported per
    (query x candidate x chain) cell;
  * a check on the way: the packed and the plain form give the same counts, and count[q][q] == terms;
  * ms of one sweep of the same handle, for scale.
Every timed step runs under a time limit of its own (--limit seconds, a watchdog thread: the library's calls release the
interpreter): a step that runs into it ends the process there with status 3, after writing what it has -- nothing more is
started on the device after a step that hung.

    python tools/coassign_bench.py [--quick] [--chains 1024] [--queries 1 16 256] [--reps 3] [--limit 120]"""
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
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--scores-from", type=int, default=16, help="the query scores are timed beside for Q >= this")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--limit", type=int, default=120, help="seconds every timed step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coassign_bench.json"))
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
    out.update({"n": na + nb, "edges": E, "blocks": "%d+%d" % (k, k), "chains": C, "candidates": na, "k": args.k, "reps": args.reps,
                "cand_tile": B.COASSIGN_CAND_TILE, "query_tile": B.COASSIGN_TILE, "by_Q": {}})
    out["sweep_ms"] = float(np.median([timed(args.limit, "sweep", lambda: m.run_sweeps(1)) for _ in range(args.reps)]))
    rs = np.random.default_rng(5)

    def accumulate(form):
        if form == "plain":
            os.environ["BISBM_COASSIGN_FORM"] = "plain"
        else:
            os.environ.pop("BISBM_COASSIGN_FORM", None)
        m.coassign_accumulate()

    for Q in args.queries:
        r = out["by_Q"][str(Q)] = {"cells_per_sample": Q * na * C}
        queries = np.sort(rs.choice(na, Q, replace=False))
        r["set_ms"] = timed(args.limit, "coassign_set Q=%d" % Q, lambda: m.coassign_set(queries))
        scores = Q >= args.scores_from
        if scores:
            r["query_scores_set_ms"] = timed(args.limit, "query_scores_set Q=%d" % Q, lambda: m.query_scores_set(queries))
        t = {"packed": [], "plain": [], "query_scores": []}
        for rep in range(args.reps + 1):  # (the routes alternated; the first round warms up and is dropped)
            t["packed"].append(timed(args.limit, "coassign_accumulate packed Q=%d" % Q, lambda: accumulate("packed")))
            t["plain"].append(timed(args.limit, "coassign_accumulate plain Q=%d" % Q, lambda: accumulate("plain")))
            if scores:
                t["query_scores"].append(timed(args.limit, "query_scores_accumulate Q=%d" % Q, m.query_scores_accumulate))
        os.environ.pop("BISBM_COASSIGN_FORM", None)
        for name, ms in t.items():
            if ms:
                r[name + "_ms_all"], r[name + "_ms"] = ms[1:], float(np.median(ms[1:]))
                r[name + "_ps_per_cell"] = r[name + "_ms"] * 1e9 / r["cells_per_sample"]
        r["plain_over_packed"] = r["plain_ms"] / r["packed_ms"]
        r["packed_over_sweep"] = r["packed_ms"] / out["sweep_ms"]
        if scores:
            r["query_scores_over_packed"] = r["query_scores_ms"] / r["packed_ms"]
        tk = [timed(args.limit, "coassign_topk Q=%d" % Q, lambda: m.coassign_topk(args.k)) for _ in range(args.reps + 1)][1:]
        r["topk_ms_all"], r["topk_ms"] = tk, float(np.median(tk))
        r["count_bytes"] = 4 * Q * na
        # a check on the way: the samples stood still, so both forms counted the same labels (reps + 1) times each
        got = {}

        def one_sample_row(form):
            m.coassign_reset()
            accumulate(form)
            got[form] = m.coassignment(Q - 1)[0]
        timed(args.limit, "coassignment Q=%d" % Q, lambda: got.update(all=m.coassignment(Q - 1)))
        row, terms = got["all"]
        r["terms"] = int(terms)
        r["self_cell_is_terms"] = bool(row[queries[Q - 1]] == terms)
        timed(args.limit, "one packed sample Q=%d" % Q, lambda: one_sample_row("packed"))
        timed(args.limit, "one plain sample Q=%d" % Q, lambda: one_sample_row("plain"))
        os.environ.pop("BISBM_COASSIGN_FORM", None)
        r["forms_agree"] = bool((got["packed"] == got["plain"]).all() and (got["packed"] * (2 * (args.reps + 1)) == row).all())
        timed(args.limit, "coassign_set() Q=%d" % Q, lambda: m.coassign_set(np.zeros(0, dtype=np.int64)))
        if scores:
            timed(args.limit, "query_scores_set() Q=%d" % Q, lambda: m.query_scores_set(np.zeros(0, dtype=np.int64)))
    write_out()
    timed(args.limit, "close", m.close)


if __name__ == "__main__":
    main()
