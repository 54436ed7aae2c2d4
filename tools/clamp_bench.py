"""What a clamp costs and saves (include/bisbm.h, "Clamped nodes") at BASELINE configs[2] -- N = 10^6 (5e5 + 5e5), E = 10^7,
32 + 32 blocks, 1024 chains -- in ONE process, after the short anneal the neighbouring tools use (--burn sweeps at T = 1, an
exponential cooling of --cool sweeps down to T = 1e-4, --settle sweeps at T = 1):
  (a) one MH sweep at T = 1: unclamped on the production kernel, unclamped on the generic kernel (BISBM_FORCE_GENERIC=1, read by
      every bisbm_anneal call), and with 10 % and 99 % of the nodes clamped (the generic kernel: the one that reads the mask) --
      what the generic-kernel route costs and what a skipped position saves (bisbm_last_sweep_timing: the kernel's time);
  (b) one heat-bath sweep at beta = 1 with 0 / 50 / 99 % of the nodes clamped (host clock around the call, which returns after
      its kernel has finished), and the time per open node;
  (c) with --parent LIB (the library built from the parent commit): the UNCLAMPED heatbath_sweeps and reshuffle calls of this
      build against the parent's, one handle each from the same start, the calls alternating, --reps alternations with this
      build first and --reps with the parent's first; the two must leave the same chains.
The masks are seeded random draws per node.  Writes profiles/clamp_bench.json and prints it.  Every step runs under a time limit
of its own (--limit seconds; tools/heatbath_bench.py's watchdog): a step that runs into it ends the process there with status 3,
after writing what it has -- nothing more is started on the device after a step that hung.

    python tools/clamp_bench.py [--quick] [--chains 1024] [--reps 3] [--parent ab/parent/libbisbm_hip.so] [--parts abc] [--limit 600]"""
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

NEW_SYMBOLS = ("bisbm_clamp_set", "bisbm_clamp_get", "bisbm_io_read_clamp")


def parent_package(lib_path, drop=NEW_SYMBOLS):
    """The Python package a second time, bound to the parent commit's library (which lacks this feature's symbols, `drop`)."""
    pkg = os.path.join(ROOT, "bipartitesbm-mcmc_amd")
    spec = importlib.util.spec_from_file_location("bisbm_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["bisbm_parent"] = mod
    spec.loader.exec_module(mod)
    mod.LIB_PATH = os.path.abspath(lib_path)
    for name in drop:
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
    ap.add_argument("--parent", default=None, help="libbisbm_hip.so built from the parent commit: part (c)")
    ap.add_argument("--parts", default="abc", help="which of the parts (a), (b), (c) run")
    ap.add_argument("--limit", type=int, default=600, help="seconds every step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clamp_bench.json"))
    args = ap.parse_args()
    hb.OUT_PATH[0] = args.out
    na = nb = 50_000 if args.quick else 500_000
    E, k, C = 20 * na, 32, args.chains
    n = na + nb
    a, b = syn.planted_edges(na, nb, E, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), n)
    OUT.update({"n": n, "edges": E, "blocks": "%d+%d" % (k, k), "chains": C, "reps": args.reps})
    rng = np.random.default_rng(1)
    draw = rng.random(n)
    masks = {share: draw < share for share in (0.1, 0.5, 0.99)}

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

    # (c) first, while both handles still hold the same chains: the unclamped calls, this build and the parent's alternating
    if args.parent and "c" in args.parts:
        P = parent_package(args.parent)
        p = annealed(P, "parent")
        for g in (m, p):
            timed(args.limit, "first reshuffle call", lambda: g.reshuffle(1, 0, 1.0))  # (the scratch is allocated here)
            timed(args.limit, "warm-up heat-bath sweep", lambda: g.heatbath_sweeps(1, 1.0))
        res = OUT["unclamped_calls_vs_parent"] = {}
        for first in ("this", "parent"):
            order = (("this", m), ("parent", p)) if first == "this" else (("parent", p), ("this", m))
            t = {"heatbath_sweep": {"this": [], "parent": []}, "reshuffle_2_moves_3_scans": {"this": [], "parent": []}}
            for _ in range(args.reps):
                for who, g in order:
                    t["heatbath_sweep"][who].append(timed(args.limit, "heat-bath sweep (%s)" % who, lambda: g.heatbath_sweeps(1, 1.0))[0])
                for who, g in order:
                    t["reshuffle_2_moves_3_scans"][who].append(timed(args.limit, "reshuffles (%s)" % who, lambda: g.reshuffle(2, 3, 1.0))[0])
            r = res[first + "_first"] = {call: {who: spread(xs) for who, xs in d.items()} for call, d in t.items()}
            for call, d in r.items():
                d["this_minus_parent_median_ms"] = d["this"]["median_ms"] - d["parent"]["median_ms"]
                d["this_minus_parent_per_pair_ms"] = [x - y for x, y in zip(d["this"]["runs_ms"], d["parent"]["runs_ms"])]
                d["this_over_parent_median"] = d["this"]["median_ms"] / d["parent"]["median_ms"]
        same = m.get_entropy().tobytes() == p.get_entropy().tobytes() and all(np.array_equal(m.get_memberships(c), p.get_memberships(c)) for c in range(C))
        res["same_chains_as_parent"] = bool(same and repr(m.reshuffle_last()) == repr(p.reshuffle_last()))
        timed(args.limit, "parent: close", p.close)
        write_out()

    # (a) MH sweeps at T = 1
    if "a" in args.parts:
        def mh_sweeps(what):
            ms = []
            for rep in range(args.reps + 1):  # (the first one is a warm-up)
                timed(args.limit, "MH sweep, " + what, lambda: m.run_sweeps(1))
                ms.append(m.last_sweep_timing()[0])
            return spread(ms[1:]), m.last_pass_steps()
        r = OUT["mh_sweep"] = {}
        r["unclamped_production"], r["production_steps_per_pass"] = mh_sweeps("unclamped, production kernel")
        os.environ["BISBM_FORCE_GENERIC"] = "1"
        r["unclamped_generic"], _ = mh_sweeps("unclamped, generic kernel")
        del os.environ["BISBM_FORCE_GENERIC"]
        for share in (0.1, 0.99):
            timed(args.limit, "clamp", lambda: m.clamp(masks[share]))
            r["clamped_%g" % share], _ = mh_sweeps("%g of the nodes clamped" % share)
            r["clamped_%g" % share]["clamped_nodes"] = int(masks[share].sum())
        timed(args.limit, "unclamp", m.unclamp)
        r["unclamped_production_again"], _ = mh_sweeps("unclamped again, production kernel")
        for key in ("unclamped_generic", "clamped_0.1", "clamped_0.99"):
            r[key]["over_production"] = r[key]["median_ms"] / r["unclamped_production"]["median_ms"]
            r[key]["over_generic"] = r[key]["median_ms"] / r["unclamped_generic"]["median_ms"]
        write_out()

    # (b) heat-bath sweeps at beta = 1
    if "b" in args.parts:
        r = OUT["heatbath_sweep"] = {}
        for share in (0.0, 0.5, 0.99):
            if share:
                timed(args.limit, "clamp", lambda: m.clamp(masks[share]))
            ms = [timed(args.limit, "heat-bath sweep, %g of the nodes clamped" % share, lambda: m.heatbath_sweeps(1, 1.0))[0] for _ in range(args.reps + 1)]
            d = r["clamped_%g" % share] = spread(ms[1:])
            d["open_nodes"] = int(n - (masks[share].sum() if share else 0))
            d["ns_per_chain_open_node"] = d["median_ms"] * 1e6 / (C * d["open_nodes"])
        timed(args.limit, "unclamp", m.unclamp)
        for key in ("clamped_0.5", "clamped_0.99"):
            r[key]["over_unclamped"] = r[key]["median_ms"] / r["clamped_0"]["median_ms"]
        write_out()
    timed(args.limit, "close", m.close)
    write_out()


if __name__ == "__main__":
    main()
