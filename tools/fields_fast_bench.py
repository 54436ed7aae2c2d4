"""What a fielded MH sweep costs on the production kernel's fielded instances and on the generic kernel at
BASELINE configs[2] -- N = 10^6 (5e5 + 5e5), E = 10^7, 32 + 32 blocks, 1024 chains -- in ONE process, after the short anneal of
tools/clamp_bench.py and tools/held_fast_bench.py (--burn sweeps at T = 1, an exponential cooling of --cool sweeps down to
T = 1e-4, --settle sweeps at T = 1).  The field is tools/fields_bench.py's: every node prefers a quarter of its type's 32 blocks by
1 nat (eight classes: the quarter a node's id falls in, per type).  One MH sweep at T = 1 (bisbm_last_sweep_timing: the kernel's
time), a warm-up and --reps timed sweeps per figure, the routes in alternation, --rounds times over:
  * the fielded sweep on the production kernel (nothing forced; last_route() must say so),
  * the same handle under BISBM_FIELD_FAST=0: the generic kernel,
and, with the field cleared,
  * the unfielded production sweep under BISBM_SINGLE_STEPS=1: one step per pass, the like-for-like for the price of the add and of
    the hand word,
  * the unfielded production sweep as the policy runs it: what the cap of one step per pass costs.
Then the same four with 10 % of the nodes clamped on top (BISBM_HELD_FAST=1 throughout: the held instances for the unfielded two).
Writes profiles/fields_fast_bench.json and prints it.  Every step runs under a time limit of its own (--limit seconds;
tools/heatbath_bench.py's watchdog): a step that runs into it ends the process there with status 3, after writing what it has --
nothing more is started on the device after a step that hung.

    python tools/fields_fast_bench.py [--quick] [--chains 1024] [--reps 2] [--rounds 2] [--limit 600]"""
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
cb = importlib.import_module("clamp_bench")
OUT, write_out, spread = hb.OUT, hb.write_out, cb.spread

ENV = ("BISBM_FORCE_GENERIC", "BISBM_HELD_FAST", "BISBM_FIELD_FAST", "BISBM_SINGLE_STEPS", "BISBM_PASS_DEPTH", "BISBM_KEEP_SUM")


def timed(limit, what, fn):
    ms, res = hb.timed(limit, what, fn)
    print("%-70s %10.1f ms" % (what, ms), flush=True)
    return ms, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a 10^5-node graph instead of configs[2] (a first look)")
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2, help="how often the routes alternate")
    ap.add_argument("--burn", type=int, default=10)
    ap.add_argument("--cool", type=int, default=20)
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--limit", type=int, default=600, help="seconds every step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields_fast_bench.json"))
    args = ap.parse_args()
    hb.OUT_PATH[0] = args.out
    for key in ENV:
        os.environ.pop(key, None)
    na = nb = 50_000 if args.quick else 500_000
    E, k, C = 20 * na, 32, args.chains
    n = na + nb
    _, (a, b) = timed(args.limit, "graph: edges", lambda: syn.planted_edges(na, nb, E, k, k, seed=1))
    _, (rp, cl) = timed(args.limit, "graph: CSR", lambda: B.edge_to_adj((a, b), n))
    OUT.update({"n": n, "edges": E, "blocks": "%d+%d" % (k, k), "chains": C, "reps": args.reps, "rounds": args.rounds})
    _, m = timed(args.limit, "create", lambda: B.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k, 1.0, (rp, cl),
                                                            n_chains=C, seed=1))
    timed(args.limit, "shuffle", m.shuffle_bisbm)
    mh = B.MetropolisHasting()
    timed(args.limit, "burn-in", lambda: mh.anneal(m, B.constant_schedule, [1.0], args.burn * n, 1 << 60))
    rate = 1e-4 ** (1.0 / (args.cool * n))
    timed(args.limit, "cooling", lambda: mh.anneal(m, B.exponential_schedule, [1.0, rate], args.cool * n, 1 << 60))
    timed(args.limit, "MH sweeps at T = 1", lambda: m.run_sweeps(args.settle))

    ids = np.arange(n)
    quarter = np.where(ids < na, (ids * 4) // na, 4 + ((ids - na) * 4) // nb)  # classes 0 .. 3 of type a, 4 .. 7 of type b
    field = np.zeros((8, 2 * k))
    for q in range(4):
        field[q, q * (k // 4):(q + 1) * (k // 4)] = -1.0
        field[4 + q, k + q * (k // 4):k + (q + 1) * (k // 4)] = -1.0

    def sweeps(what, env, ms):
        """a warm-up and --reps timed sweeps under `env`, appended to ms: (route, steps per pass) of the launches"""
        os.environ.update(env)
        for rep in range(args.reps + 1):
            timed(args.limit, "MH sweep, " + what, lambda: m.run_sweeps(1))
            if rep:
                ms.append(m.last_sweep_timing()[0])
        seen = (m.last_route(), m.last_pass_steps())
        for key in env:
            del os.environ[key]
        return seen

    def four(tag, base):
        """the four figures, the routes alternating --rounds times; base: the environment of all of them"""
        ms = {"fielded_production": [], "fielded_generic": [], "unfielded_single_steps": [], "unfielded_policy": []}
        seen = {}
        held = B.ROUTE_HELD if base else 0
        for rnd in range(args.rounds):
            timed(args.limit, "set_fields", lambda: m.set_fields(quarter, field))
            seen["fielded_production"] = sweeps(tag + "fielded, production kernel", dict(base), ms["fielded_production"])
            seen["fielded_generic"] = sweeps(tag + "fielded, generic kernel", dict(base, BISBM_FIELD_FAST="0"), ms["fielded_generic"])
            timed(args.limit, "clear_fields", m.clear_fields)
            seen["unfielded_single_steps"] = sweeps(tag + "unfielded, one step per pass", dict(base, BISBM_SINGLE_STEPS="1"), ms["unfielded_single_steps"])
            seen["unfielded_policy"] = sweeps(tag + "unfielded, as the policy runs it", dict(base), ms["unfielded_policy"])
        assert seen["fielded_production"] == (B.ROUTE_PRODUCTION | B.ROUTE_FIELDS | held, 1), seen
        assert seen["fielded_generic"] == (B.ROUTE_FIELDS | held, 1), seen
        assert seen["unfielded_single_steps"] == (B.ROUTE_PRODUCTION | held, 1), seen
        assert seen["unfielded_policy"][0] == B.ROUTE_PRODUCTION | held and seen["unfielded_policy"][1] > 1, seen
        r = {key: dict(spread(v), steps_per_pass=seen[key][1], route=seen[key][0]) for key, v in ms.items()}
        med = lambda key: r[key]["median_ms"]
        r["generic_over_fielded_production"] = med("fielded_generic") / med("fielded_production")
        r["fielded_production_over_unfielded_single_steps"] = med("fielded_production") / med("unfielded_single_steps")
        r["fielded_production_over_unfielded_policy"] = med("fielded_production") / med("unfielded_policy")
        return r

    OUT["field"] = four("", {})
    write_out()
    mask = np.random.default_rng(1).random(n) < 0.1
    timed(args.limit, "clamp 0.1", lambda: m.clamp(mask))
    OUT["field_and_10_percent_clamped"] = four("10 % clamped, ", {"BISBM_HELD_FAST": "1"})
    OUT["field_and_10_percent_clamped"]["clamped_nodes"] = int(mask.sum())
    timed(args.limit, "unclamp", m.unclamp)
    timed(args.limit, "close", m.close)
    write_out()


if __name__ == "__main__":
    main()
