"""Cost of the rounds of mixed moves under replica exchange (include/bisbm.h, "Heat-bath sweeps and pair reshuffles inside replica
exchange") at BASELINE configs[2] -- N = 10^6 (5e5 + 5e5), E = 10^7, 32 + 32 blocks, --chains chains as ensembles of 8 rungs -- in
ONE process, after the short anneal of tools/heatbath_bench.py (--burn sweeps at T = 1, then an exponential cooling of --cool
sweeps from T = 1 down to T = 1e-4) and --settle MH sweeps at T = 1:
  (a) ms per round (host clock around tempering_rounds, medians of --reps) of the recipes {1, 0, 0}, {1, 1, 0} and {1, 0, 2 scans
      3}, and the per-rung table after each: reshuffle acceptance and heat-bath move share by rung;
  (b) with --parent LIB (the library built from the parent commit): the plain heatbath_sweeps and reshuffle calls of this build
      against the parent's, one handle each from the same start, the calls alternating, --reps of each -- the per-chain beta must
      not cost the existing calls more than the spread of the repeats;
  (c) with --parent LIB: tempering_rounds(R, mh=k) of this build against the parent's tempering_run(R k, k).
Writes profiles/tempered_moves_bench.json and prints it.  Every step runs under a time limit of its own, as in
tools/heatbath_bench.py: a step that runs into it ends the process with status 3 after writing what it has.  What the rounds do
to the mode hopping of equilibrated chains is NOT measured here.

    python tools/tempered_moves_bench.py [--quick] [--chains 1024] [--reps 3] [--parent ab/libbisbm_hip_parent.so] [--parts abc]
                                         [--parent-first] [--limit 600]"""
import argparse
import importlib
import importlib.util
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

LADDER = [1.0, 1.04, 1.08, 1.13, 1.18, 1.24, 1.31, 1.4]  # (8 rungs, steps of 4 to 7 %: chosen by hand, not tuned)
NEW_SYMBOLS = ("bisbm_tempering_run_rounds", "bisbm_tempering_rung_stats", "bisbm_rounds_population_run")


def parent_package(lib_path):
    """The Python package a second time, bound to the parent commit's library (which lacks this feature's symbols)."""
    pkg = os.path.join(ROOT, "bipartitesbm-mcmc_amd")
    spec = importlib.util.spec_from_file_location("bisbm_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["bisbm_parent"] = mod
    spec.loader.exec_module(mod)
    mod.LIB_PATH = os.path.abspath(lib_path)
    for name in NEW_SYMBOLS:
        mod.ABI.pop(name, None)
    mod.lib()
    return mod


def spread(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(min(xs)), "max_ms": float(max(xs)), "runs_ms": [float(x) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a 10^5-node graph instead of configs[2] (a first look)")
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--burn", type=int, default=10)
    ap.add_argument("--cool", type=int, default=20)
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--parent", default=None, help="libbisbm_hip.so built from the parent commit: parts (b) and (c)")
    ap.add_argument("--parts", default="abc", help="which of the parts (a), (b), (c) run")
    ap.add_argument("--parent-first", action="store_true", help="(b), (c): the parent's call goes first in every alternation")
    ap.add_argument("--limit", type=int, default=600, help="seconds every step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tempered_moves_bench.json"))
    args = ap.parse_args()
    hb.OUT_PATH[0] = args.out
    na = nb = 50_000 if args.quick else 500_000
    E, k, C = 20 * na, 32, args.chains
    n = na + nb
    a, b = syn.planted_edges(na, nb, E, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), n)
    OUT.update({"n": n, "edges": E, "blocks": "%d+%d" % (k, k), "chains": C, "ladder": LADDER, "ensembles": C // len(LADDER), "reps": args.reps})

    def annealed(pkg, what):
        _, m = timed(args.limit, what + ": create", lambda: pkg.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k, 1.0,
                                                                           (rp, cl), n_chains=C, seed=1))
        timed(args.limit, what + ": shuffle", m.shuffle_bisbm)
        mh = pkg.MetropolisHasting()
        timed(args.limit, what + ": burn-in", lambda: mh.anneal(m, pkg.constant_schedule, [1.0], args.burn * n, 1 << 60))
        rate = 1e-4 ** (1.0 / (args.cool * n))
        timed(args.limit, what + ": cooling", lambda: mh.anneal(m, pkg.exponential_schedule, [1.0, rate], args.cool * n, 1 << 60))
        timed(args.limit, what + ": MH sweeps at T = 1", lambda: m.run_sweeps(args.settle))
        return m

    m = annealed(B, "this build")
    P = parent_package(args.parent) if args.parent else None
    p = annealed(P, "parent") if P else None

    # (b) the existing calls, this build and the parent's alternating (before tempering is set: they are refused under it)
    order = (("parent", p), ("this", m)) if args.parent_first else (("this", m), ("parent", p))
    OUT["first_in_every_alternation"] = order[0][0]
    if P and "b" in args.parts:
        for g in (m, p):
            timed(args.limit, "first reshuffle call", lambda: g.reshuffle(1, 0, 1.0))  # (the scratch is allocated here)
            timed(args.limit, "warm-up heat-bath sweep", lambda: g.heatbath_sweeps(1, 1.0))
        t = {"heatbath_sweep": {"this": [], "parent": []}, "reshuffle_2_moves_3_scans": {"this": [], "parent": []}}
        for _ in range(args.reps):
            for who, g in order:
                t["heatbath_sweep"][who].append(timed(args.limit, "heat-bath sweep (%s)" % who, lambda: g.heatbath_sweeps(1, 1.0))[0])
            for who, g in order:
                t["reshuffle_2_moves_3_scans"][who].append(timed(args.limit, "reshuffles (%s)" % who, lambda: g.reshuffle(2, 3, 1.0))[0])
        OUT["existing_calls_vs_parent"] = {call: {who: spread(xs) for who, xs in d.items()} for call, d in t.items()}
        # one start, the same calls: every chain's labels, cum_dS bit for bit, and what the last call of each kind left behind
        same = m.get_entropy().tobytes() == p.get_entropy().tobytes() and all(np.array_equal(m.get_memberships(c), p.get_memberships(c)) for c in range(C))
        equal = {"heatbath_sweep": same and all(np.array_equal(x, y) for x, y in zip(m.last_counts(), p.last_counts())),
                 "reshuffle_2_moves_3_scans": same and repr(m.reshuffle_last()) == repr(p.reshuffle_last())}
        for call, d in OUT["existing_calls_vs_parent"].items():
            d["this_over_parent_median"] = d["this"]["median_ms"] / d["parent"]["median_ms"]
            d["equal_to_parent"] = bool(equal[call])
        write_out()

    # (c) MH-only rounds against the parent's tempering_run
    R, kk = 4, 2
    m.set_tempering(LADDER)
    if P and "c" in args.parts:
        p.set_tempering(LADDER)
        timed(args.limit, "warm-up rounds", lambda: m.tempering_rounds(1, mh=kk))
        timed(args.limit, "warm-up tempering_run", lambda: p.tempering_run(kk, kk))
        t = {"this": [], "parent": []}
        calls = {"this": lambda: m.tempering_rounds(R, mh=kk), "parent": lambda: p.tempering_run(R * kk, kk)}
        for _ in range(args.reps):
            for who, _g in order:
                t[who].append(timed(args.limit, "%s: %d rounds of %d MH sweeps" % (who, R, kk), calls[who])[0])
        OUT["mh_rounds_vs_parent_tempering_run"] = {"rounds": R, "sweeps_per_round": kk, "this": spread(t["this"]), "parent": spread(t["parent"]),
                                                    "this_over_parent_median": float(np.median(t["this"]) / np.median(t["parent"]))}
        write_out()
    if P:
        p.close()

    # (a) ms per round of three recipes and the per-rung table after each (the statistics start afresh with each recipe)
    OUT["recipes"] = {}
    for name, kw in () if "a" not in args.parts else (("mh1", dict(mh=1)), ("mh1_hb1", dict(mh=1, heatbath=1)), ("mh1_rs2_scans3", dict(mh=1, reshuffles=2, scans=3))):
        m.set_tempering(LADDER)
        timed(args.limit, name + ": warm-up round", lambda: m.tempering_rounds(1, **kw))
        ms = [timed(args.limit, name + ": round", lambda: m.tempering_rounds(1, **kw))[0] for _ in range(args.reps)]
        st = m.tempering_rung_stats()
        att, acc, rounds = m.tempering_stats()
        with np.errstate(invalid="ignore", divide="ignore"):
            OUT["recipes"][name] = {"round": spread(ms), "rounds_in_table": int(rounds),
                                    "mh_acceptance_by_rung": np.nan_to_num(st["mh_accepted"] / st["mh_steps"]).tolist(),
                                    "heatbath_move_share_by_rung": np.nan_to_num(st["heatbath_moves"] / st["heatbath_steps"]).tolist(),
                                    "reshuffles_by_rung": st["reshuffles"].tolist(), "reshuffles_accepted_by_rung": st["reshuffles_accepted"].tolist(),
                                    "reshuffle_acceptance_by_rung": np.nan_to_num(st["reshuffles_accepted"] / st["reshuffles"]).tolist(),
                                    "swaps_attempted": att.tolist(), "swaps_accepted": acc.tolist()}
        write_out()
    OUT["mode_hopping_of_equilibrated_chains"] = "not measured"
    write_out()
    m.close()


if __name__ == "__main__":
    main()
