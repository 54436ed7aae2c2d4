"""What block fields cost (include/bisbm.h, "Block fields"), and what their code costs a handle without them, at BASELINE
configs[2] -- N = 10^6 (5e5 + 5e5), E = 10^7, 32 + 32 blocks, 1024 chains -- in ONE process, after the short anneal of
tools/clamp_bench.py (--burn sweeps at T = 1, an exponential cooling of --cool sweeps down to T = 1e-4, --settle sweeps at T = 1).
  (a) under a field: every node prefers a quarter of its type's 32 blocks by 1 nat (eight classes: the quarter a node's id falls
      in, per type).  One MH sweep (the generic kernel's field instance: bisbm_last_sweep_timing) beside the unfielded generic
      sweep of the same build (BISBM_FORCE_GENERIC=1) and the production kernel's; one heat-bath sweep at beta = 1 and two
      reshuffles of 3 scans (host clock around the call) beside the same calls without a field;
  (b) with --parent LIB (the library built from the parent commit): the calls of a handle WITHOUT fields whose kernels this
      feature touched, against the parent's -- the heat-bath sweep, the heat-bath sweep under a clamp of half the nodes and under
      the constraints of tools/constraints_bench.py, two reshuffles of 3 scans, and the generic MH
      sweep (BISBM_FORCE_GENERIC=1) -- one handle each from the same start, the calls alternating, --reps alternations with this
      build first and --reps with the parent's first; the two must leave the same chains.
Writes profiles/fields_bench.json and prints it.  Every step runs under a time limit of its own (--limit seconds;
tools/heatbath_bench.py's watchdog): a step that runs into it ends the process there with status 3, after writing what it has --
nothing more is started on the device after a step that hung.

    python tools/fields_bench.py [--quick] [--chains 1024] [--reps 2] [--parent ab/parent/libbisbm_hip.so] [--parts ab] [--calls LIST] [--limit 600]"""
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
cb = importlib.import_module("clamp_bench")     # (the package bound to the parent's library)
cnb = importlib.import_module("constraints_bench")
OUT, write_out, spread = hb.OUT, hb.write_out, cb.spread


def timed(limit, what, fn):
    """heatbath_bench.timed, with a line per finished step (a run of many short steps shows that it is alive)"""
    ms, res = hb.timed(limit, what, fn)
    print("%-50s %10.1f ms" % (what, ms), flush=True)
    return ms, res


NEW_SYMBOLS = cnb.NEW_SYMBOLS + ("bisbm_fields_set", "bisbm_fields_get", "bisbm_fields_energy", "bisbm_io_read_fields")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a 10^5-node graph instead of configs[2] (a first look)")
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--burn", type=int, default=10)
    ap.add_argument("--cool", type=int, default=20)
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--parent", default=None, help="libbisbm_hip.so built from the parent commit: part (b)")
    ap.add_argument("--parts", default="ab", help="which of the parts (a), (b) run")
    ap.add_argument("--calls", default=None, help="part (b): a comma-separated subset of heatbath_sweep, reshuffle_2_moves_3_scans, "
                                                   "generic_mh_sweep, heatbath_sweep_half_clamped, heatbath_sweep_constrained (default: all five)")
    ap.add_argument("--limit", type=int, default=600, help="seconds every step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields_bench.json"))
    args = ap.parse_args()
    hb.OUT_PATH[0] = args.out
    na = nb = 50_000 if args.quick else 500_000
    E, k, C = 20 * na, 32, args.chains
    n = na + nb
    _, (a, b) = timed(args.limit, "graph: edges", lambda: syn.planted_edges(na, nb, E, k, k, seed=1))
    _, (rp, cl) = timed(args.limit, "graph: CSR", lambda: B.edge_to_adj((a, b), n))
    OUT.update({"n": n, "edges": E, "blocks": "%d+%d" % (k, k), "chains": C, "reps": args.reps})
    half = np.random.default_rng(1).random(n) < 0.5

    def annealed(pkg, what):
        _, m = timed(args.limit, what + ": create", lambda: pkg.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k, 1.0,
                                                                           (rp, cl), n_chains=C, seed=1))
        timed(args.limit, what + ": shuffle", m.shuffle_bisbm)
        mh = pkg.MetropolisHasting()
        timed(args.limit, what + ": burn-in", lambda: mh.anneal(m, pkg.constant_schedule, [1.0], args.burn * n, 1 << 60))
        rate = 1e-4 ** (1.0 / (args.cool * n))
        timed(args.limit, what + ": cooling", lambda: mh.anneal(m, pkg.exponential_schedule, [1.0, rate], args.cool * n, 1 << 60))
        timed(args.limit, what + ": MH sweeps at T = 1", lambda: m.run_sweeps(args.settle))
        return m, None

    m, lab = annealed(B, "this build")

    def mh_ms(g):
        g.run_sweeps(1)
        return g.last_sweep_timing()[0]

    # (b) first, while both handles still hold the same chains: the calls of a handle without fields, this build and the parent's
    if args.parent and "b" in args.parts:
        P = cb.parent_package(args.parent, drop=NEW_SYMBOLS)
        p, _ = annealed(P, "parent")
        for g in (m, p):
            timed(args.limit, "first reshuffle call", lambda: g.reshuffle(1, 0, 1.0))  # (the scratch is allocated here)
            timed(args.limit, "warm-up heat-bath sweep", lambda: g.heatbath_sweeps(1, 1.0))
        calls = {
            "heatbath_sweep": lambda g: timed(args.limit, "heat-bath sweep", lambda: g.heatbath_sweeps(1, 1.0))[0],
            "reshuffle_2_moves_3_scans": lambda g: timed(args.limit, "reshuffles", lambda: g.reshuffle(2, 3, 1.0))[0],
            "generic_mh_sweep": lambda g: timed(args.limit, "generic MH sweep", lambda: mh_ms(g))[1],
            "heatbath_sweep_half_clamped": lambda g: timed(args.limit, "heat-bath sweep under a clamp", lambda: g.heatbath_sweeps(1, 1.0))[0],
            "heatbath_sweep_constrained": lambda g: timed(args.limit, "heat-bath sweep under constraints", lambda: g.heatbath_sweeps(1, 1.0))[0],
        }
        # the constraints of tools/constraints_bench.py: four classes per type, each allowing a disjoint quarter of the type's
        # blocks, a node's class the quarter its block is in (every chain is set to chain 0's labels first, so one table admits all)
        allowed = np.zeros((8, 2 * k), dtype=bool)
        for q in range(4):
            allowed[q, q * (k // 4):(q + 1) * (k // 4)] = True
            allowed[q, k:] = True
            allowed[4 + q, k + q * (k // 4):k + (q + 1) * (k // 4)] = True
            allowed[4 + q, :k] = True
        if args.calls:
            calls = {call: fn for call, fn in calls.items() if call in args.calls.split(",")}
        res = OUT["unfielded_calls_vs_parent"] = {}
        t = {first: {call: {"this": [], "parent": []} for call in calls} for first in ("this", "parent")}
        for call, fn in calls.items():  # (one kind of call at a time, both orders, so that a clamp is set and cleared once)
            if call == "generic_mh_sweep":
                os.environ["BISBM_FORCE_GENERIC"] = "1"
                for g in (m, p):
                    timed(args.limit, "warm-up generic MH sweep", lambda: g.run_sweeps(1))
            if call == "heatbath_sweep_half_clamped":
                for g in (m, p):
                    timed(args.limit, "clamp", lambda: g.clamp(half))
                    timed(args.limit, "warm-up heat-bath sweep under a clamp", lambda: g.heatbath_sweeps(1, 1.0))
            if call == "heatbath_sweep_constrained":
                for g in (m, p):
                    timed(args.limit, "unclamp", g.unclamp)
                    lab = g.get_memberships(0)
                    timed(args.limit, "every chain to chain 0's labels", lambda: (g.set_memberships(lab), g.init_bisbm()))
                    lab = lab.astype(np.int64)
                    timed(args.limit, "constrain", lambda: g.constrain(np.where(lab < k, lab // (k // 4), 4 + (lab - k) // (k // 4)), allowed))
                    timed(args.limit, "warm-up heat-bath sweep under constraints", lambda: g.heatbath_sweeps(1, 1.0))
            for first in ("this", "parent"):
                order = (("this", m), ("parent", p)) if first == "this" else (("parent", p), ("this", m))
                for _ in range(args.reps):
                    for who, g in order:
                        t[first][call][who].append(fn(g))
            os.environ.pop("BISBM_FORCE_GENERIC", None)
        for g in (m, p):
            timed(args.limit, "unclamp", g.unclamp)
            timed(args.limit, "unconstrain", g.unconstrain)
        for first in ("this", "parent"):
            r = res[first + "_first"] = {call: {who: spread(xs) for who, xs in d.items()} for call, d in t[first].items()}
            for call, d in r.items():
                d["this_minus_parent_median_ms"] = d["this"]["median_ms"] - d["parent"]["median_ms"]
                d["this_minus_parent_per_pair_ms"] = [x - y for x, y in zip(d["this"]["runs_ms"], d["parent"]["runs_ms"])]
                d["this_over_parent_median"] = d["this"]["median_ms"] / d["parent"]["median_ms"]
        same = m.get_entropy().tobytes() == p.get_entropy().tobytes() and all(np.array_equal(m.get_memberships(c), p.get_memberships(c)) for c in range(C))
        res["same_chains_as_parent"] = bool(same and repr(m.reshuffle_last()) == repr(p.reshuffle_last()))
        timed(args.limit, "parent: close", p.close)
        write_out()

    # (a) the fielded calls beside the unfielded ones of the same handle
    if "a" in args.parts:
        r = OUT["fielded_sweep"] = {"classes": 8, "preferred_blocks_per_node": k // 4, "preference_nats": 1.0}

        def measure(tag, generic=False):
            ms = {"mh_sweep": [], "heatbath_sweep": [], "reshuffle_2_moves_3_scans": []}
            if generic:
                os.environ["BISBM_FORCE_GENERIC"] = "1"
            for rep in range(args.reps + 1):  # (the first one is a warm-up)
                ms["mh_sweep"].append(timed(args.limit, "MH sweep, " + tag, lambda: mh_ms(m))[1])
                if not generic:
                    ms["heatbath_sweep"].append(timed(args.limit, "heat-bath sweep, " + tag, lambda: m.heatbath_sweeps(1, 1.0))[0])
                    ms["reshuffle_2_moves_3_scans"].append(timed(args.limit, "reshuffles, " + tag, lambda: m.reshuffle(2, 3, 1.0))[0])
            os.environ.pop("BISBM_FORCE_GENERIC", None)
            r[tag] = {call: spread(xs[1:]) for call, xs in ms.items() if len(xs) > 1}
            r[tag]["mh_steps_per_pass"] = m.last_pass_steps()
        measure("unfielded")
        measure("unfielded_generic", generic=True)
        ids = np.arange(n)
        quarter = np.where(ids < na, (ids * 4) // na, 4 + ((ids - na) * 4) // nb)  # classes 0 .. 3 of type a, 4 .. 7 of type b
        field = np.zeros((8, 2 * k))
        for q in range(4):
            field[q, q * (k // 4):(q + 1) * (k // 4)] = -1.0
            field[4 + q, k + q * (k // 4):k + (q + 1) * (k // 4)] = -1.0
        timed(args.limit, "set_fields", lambda: m.set_fields(quarter, field))
        measure("fielded")
        timed(args.limit, "field_energy", m.field_energy)
        timed(args.limit, "clear_fields", m.clear_fields)
        for call in ("mh_sweep", "heatbath_sweep", "reshuffle_2_moves_3_scans"):
            r["fielded"][call]["over_unfielded"] = r["fielded"][call]["median_ms"] / r["unfielded"][call]["median_ms"]
        r["fielded"]["mh_sweep"]["over_unfielded_generic"] = r["fielded"]["mh_sweep"]["median_ms"] / r["unfielded_generic"]["mh_sweep"]["median_ms"]
        write_out()
    timed(args.limit, "close", m.close)
    write_out()
    import json
    print(json.dumps(OUT))


if __name__ == "__main__":
    main()
