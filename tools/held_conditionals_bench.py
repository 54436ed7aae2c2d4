"""Cost of the held conditionals and of the least-settled ranking (include/bisbm.h, "Held conditionals", "Least settled") at
tools/conditionals_bench.py's case (a) -- BASELINE configs[2], N = 10^6 (5e5 + 5e5), E = 10^7, 32 + 32 blocks, 4096 queries x
all chains of a 1024-chain handle -- in ONE process, host clock around calls that return after their kernels have finished,
medians of --reps after a warm-up call.  One conditional sample in four configurations:
  plain                       the switch off;
  on_nothing_held             the switch on, no clamp, no constraints, no fields: the plain kernel is launched;
  on_quarter_table            the switch on, every node held to a quarter of its type's blocks (tools/held_fast_bench.py's table);
  on_table_clamp_field        ... plus 10 % of the nodes clamped and a field of N(0, 1) nats in eight classes.
Then bisbm_least_settled_topk(100) over 10^6 queries (every node, a 16-chain handle, one sample) for both statistics, beside the
host's way: conditionals_stats() and a sort.  Writes profiles/held_conditionals_bench.json and prints it.
Every timed step runs under a time limit of its own (--limit seconds, a watchdog thread): a step that runs into it ends the
process there with status 3, after writing what it has -- nothing more is started on the device after a step that hung.

    python tools/held_conditionals_bench.py [--quick] [--chains 1024] [--few 16] [--queries 4096] [--reps 3] [--limit 120]"""
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
    ap.add_argument("--few", type=int, default=16, help="chains of the handle whose 10^6 queries are ranked")
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds every timed step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "held_conditionals_bench.json"))
    args = ap.parse_args()
    OUT_PATH[0] = args.out
    na = nb = 50_000 if args.quick else 500_000
    E, k = 20 * na, 32
    a, b = syn.planted_edges(na, nb, E, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), na + nb)
    n = na + nb
    OUT.update({"n": n, "edges": E, "blocks": "%d+%d" % (k, k), "reps": args.reps, "sample": {}, "least_settled": {}})

    def handle(C):
        made = []
        timed(args.limit, "create %d" % C, lambda: made.append(B.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k,
                                                                           1.0, (rp, cl), n_chains=C, seed=1)))
        m = made[0]
        timed(args.limit, "shuffle", m.shuffle_bisbm)
        timed(args.limit, "warm-up sweeps", lambda: m.run_sweeps(2))
        return m

    def sample(tag, m, C, Q):
        ms = [timed(args.limit, "conditionals_accumulate " + tag, m.conditionals_accumulate) for _ in range(args.reps + 1)][1:]
        got = {}
        timed(args.limit, "stats " + tag, lambda: got.update(st=m.conditionals_stats()))
        st = got["st"]
        r = OUT["sample"][tag] = {"chains": C, "queries": Q, "ms_all": ms, "ms": float(np.median(ms)), "held": bool(m.conditionals_is_held()),
                                  "ns_per_chain_query": float(np.median(ms)) * 1e6 / (C * Q), "terms": int(st["terms"]),
                                  "mean_stay": float(st["stay"].sum() / (st["terms"] * Q)), "mean_entropy": float(st["entropy"].sum() / (st["terms"] * Q)),
                                  "open_share": float(st["free"].sum() / (st["terms"] * Q))}
        if tag != "plain":
            r["over_plain"] = r["ms"] / OUT["sample"]["plain"]["ms"]
        write_out()

    rs = np.random.default_rng(5)
    Q = min(args.queries, n)
    queries = np.sort(rs.choice(n, Q, replace=False)).astype(np.uint32)
    m = handle(args.chains)
    lab = m.get_memberships(0).astype(np.int64)  # (the table must admit every chain: all of them to chain 0's labels)
    timed(args.limit, "every chain to chain 0's labels", lambda: (m.set_memberships(lab.astype(np.uint32)), m.init_bisbm()))
    timed(args.limit, "conditionals_set", lambda: m.conditionals_set(queries))
    sample("plain", m, args.chains, Q)
    timed(args.limit, "conditionals_held", lambda: m.conditionals_held(True))
    sample("on_nothing_held", m, args.chains, Q)
    quarter = np.where(lab < k, lab // (k // 4), 4 + (lab - k) // (k // 4))  # classes 0 .. 3 of type a, 4 .. 7 of type b
    allowed = np.zeros((8, 2 * k), dtype=bool)
    for q in range(4):
        allowed[q, q * (k // 4):(q + 1) * (k // 4)] = True
        allowed[q, k:] = True
        allowed[4 + q, k + q * (k // 4):k + (q + 1) * (k // 4)] = True
        allowed[4 + q, :k] = True
    timed(args.limit, "constrain", lambda: m.constrain(quarter, allowed))
    timed(args.limit, "conditionals_reset", m.conditionals_reset)
    sample("on_quarter_table", m, args.chains, Q)
    timed(args.limit, "clamp 0.1", lambda: m.clamp(rs.random(n) < 0.1))
    timed(args.limit, "set_fields", lambda: m.set_fields(rs.integers(0, 8, n), rs.normal(size=(8, 2 * k))))
    timed(args.limit, "conditionals_reset", m.conditionals_reset)
    sample("on_table_clamp_field", m, args.chains, Q)
    timed(args.limit, "conditionals_set()", lambda: m.conditionals_set([]))
    timed(args.limit, "close", m.close)

    # the ranking over every node
    m = handle(args.few)
    timed(args.limit, "conditionals_set all", lambda: m.conditionals_set(None))
    OUT["least_settled"]["sample_ms"] = timed(args.limit, "conditionals_accumulate all", m.conditionals_accumulate)
    for by in ("entropy", "stay"):
        got = {}
        dev = [timed(args.limit, "least_settled " + by, lambda: got.update(dev=m.least_settled(100, by))) for _ in range(args.reps + 1)][1:]

        def host():
            st = m.conditionals_stats()
            v = st[by]
            order = np.lexsort((np.arange(len(v)), v if by == "stay" else -v))[:100]
            got.update(host=(order, v[order]))
        hst = [timed(args.limit, "stats and sort " + by, host) for _ in range(args.reps + 1)][1:]
        same = bool((got["dev"][0] == got["host"][0]).all() and got["dev"][2].tobytes() == got["host"][1].tobytes())
        OUT["least_settled"][by] = {"queries": n, "k": 100, "device_ms_all": dev, "device_ms": float(np.median(dev)), "host_ms_all": hst,
                                    "host_ms": float(np.median(hst)), "host_over_device": float(np.median(hst) / np.median(dev)), "same_result": same}
    timed(args.limit, "close", m.close)
    write_out()


if __name__ == "__main__":
    main()
