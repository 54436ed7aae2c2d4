"""What a held MH sweep costs on the production kernel and on the generic kernel at BASELINE configs[2]
-- N = 10^6 (5e5 + 5e5), E = 10^7, 32 + 32 blocks, 1024 chains -- in ONE process, after the short anneal of tools/clamp_bench.py
and tools/constraints_bench.py (--burn sweeps at T = 1, an exponential cooling of --cool sweeps down to T = 1e-4, --settle sweeps
at T = 1).  The clamped shares are measured on these chains as they are (the state of tools/clamp_bench.py); for the table every
chain is then set to chain 0's labels, so that one table admits all of them (the streams stay the chains' own; the state of
tools/constraints_bench.py, in which a sweep takes about half the time), and the unheld sweep is measured again there.
One MH sweep at T = 1 (bisbm_last_sweep_timing: the kernel's time), a warm-up and --reps timed sweeps each, of
  * the unheld handle on the production kernel and on the generic kernel (BISBM_FORCE_GENERIC=1),
  * the handle with 0 / 5 / 10 / 50 / 90 / 97 / 99 % of its nodes clamped (seeded random draws per node; 0 %: a clamp of one node),
  * every node held to a quarter of its type's blocks (tools/constraints_bench.py's table),
  * 5 % clamped plus the quarter table,
each held case on the production kernel's held instances (BISBM_HELD_FAST=1) and on the generic kernel (BISBM_HELD_FAST=0), the
two alternating.  The crossing of the two kernels over the clamped share is what kHeldFastMaxClampShare (csrc/bisbm_kernels.hpp)
is set by.  Writes profiles/held_fast_bench.json and prints it.  Every step runs under a time limit of its own (--limit seconds;
tools/heatbath_bench.py's watchdog): a step that runs into it ends the process there with status 3, after writing what it has --
nothing more is started on the device after a step that hung.

    python tools/held_fast_bench.py [--quick] [--chains 1024] [--reps 2] [--limit 600]"""
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

SHARES = (0.0, 0.05, 0.1, 0.5, 0.9, 0.97, 0.99)


def timed(limit, what, fn):
    ms, res = hb.timed(limit, what, fn)
    print("%-60s %10.1f ms" % (what, ms), flush=True)
    return ms, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a 10^5-node graph instead of configs[2] (a first look)")
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--burn", type=int, default=10)
    ap.add_argument("--cool", type=int, default=20)
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--limit", type=int, default=600, help="seconds every step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "held_fast_bench.json"))
    args = ap.parse_args()
    hb.OUT_PATH[0] = args.out
    for key in ("BISBM_FORCE_GENERIC", "BISBM_HELD_FAST"):
        os.environ.pop(key, None)
    na = nb = 50_000 if args.quick else 500_000
    E, k, C = 20 * na, 32, args.chains
    n = na + nb
    _, (a, b) = timed(args.limit, "graph: edges", lambda: syn.planted_edges(na, nb, E, k, k, seed=1))
    _, (rp, cl) = timed(args.limit, "graph: CSR", lambda: B.edge_to_adj((a, b), n))
    OUT.update({"n": n, "edges": E, "blocks": "%d+%d" % (k, k), "chains": C, "reps": args.reps})
    _, m = timed(args.limit, "create", lambda: B.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k, 1.0, (rp, cl),
                                                            n_chains=C, seed=1))
    timed(args.limit, "shuffle", m.shuffle_bisbm)
    mh = B.MetropolisHasting()
    timed(args.limit, "burn-in", lambda: mh.anneal(m, B.constant_schedule, [1.0], args.burn * n, 1 << 60))
    rate = 1e-4 ** (1.0 / (args.cool * n))
    timed(args.limit, "cooling", lambda: mh.anneal(m, B.exponential_schedule, [1.0, rate], args.cool * n, 1 << 60))
    timed(args.limit, "MH sweeps at T = 1", lambda: m.run_sweeps(args.settle))

    def sweeps(what, env):
        """a warm-up and --reps timed sweeps under `env`: (spread of the kernel's ms, steps per pass)"""
        os.environ.update(env)
        ms = []
        for rep in range(args.reps + 1):
            timed(args.limit, "MH sweep, " + what, lambda: m.run_sweeps(1))
            ms.append(m.last_sweep_timing()[0])
        steps = m.last_pass_steps()
        for key in env:
            del os.environ[key]
        d = spread(ms[1:])
        d["steps_per_pass"] = steps
        return d

    def both_kernels(tag):
        r = {"production_held": sweeps(tag + ", production kernel", {"BISBM_HELD_FAST": "1"}),
             "generic": sweeps(tag + ", generic kernel", {"BISBM_HELD_FAST": "0"})}
        assert r["production_held"]["steps_per_pass"] == 2 and r["generic"]["steps_per_pass"] == 1, r
        r["generic_over_production_held"] = r["generic"]["median_ms"] / r["production_held"]["median_ms"]
        return r

    unheld = OUT["unheld"] = {"production": sweeps("unheld, production kernel", {}), "generic": sweeps("unheld, generic kernel", {"BISBM_FORCE_GENERIC": "1"})}
    write_out()

    draw = np.random.default_rng(1).random(n)
    res = OUT["clamped"] = {}
    for share in SHARES:
        mask = draw < share
        if not mask.any():
            mask[0] = True  # (an empty mask is no clamp)
        timed(args.limit, "clamp %g" % share, lambda: m.clamp(mask))
        r = res["%g" % share] = both_kernels("%g of the nodes clamped" % share)
        r["clamped_nodes"] = int(mask.sum())
        r["production_held_over_unheld"] = r["production_held"]["median_ms"] / unheld["production"]["median_ms"]
        write_out()
    timed(args.limit, "unclamp", m.unclamp)
    # where the two kernels cross: between the last share at which the production kernel wins and the first at which it loses
    wins = [s for s in SHARES if res["%g" % s]["generic_over_production_held"] > 1.0]
    loses = [s for s in SHARES if res["%g" % s]["generic_over_production_held"] <= 1.0]
    OUT["crossing_between_shares"] = [max(wins) if wins else None, min(loses) if loses else None]

    lab = m.get_memberships(0).astype(np.int64)  # (the table must admit every chain: all of them to chain 0's labels once more)
    timed(args.limit, "every chain to chain 0's labels", lambda: (m.set_memberships(lab.astype(np.uint32)), m.init_bisbm()))
    OUT["unheld_before_the_table"] = sweeps("unheld, production kernel, one start for all chains", {})
    lab = m.get_memberships(0).astype(np.int64)
    timed(args.limit, "every chain to chain 0's labels", lambda: (m.set_memberships(lab.astype(np.uint32)), m.init_bisbm()))
    quarter = np.where(lab < k, lab // (k // 4), 4 + (lab - k) // (k // 4))  # classes 0 .. 3 of type a, 4 .. 7 of type b
    allowed = np.zeros((8, 2 * k), dtype=bool)
    for q in range(4):
        allowed[q, q * (k // 4):(q + 1) * (k // 4)] = True
        allowed[q, k:] = True
        allowed[4 + q, k + q * (k // 4):k + (q + 1) * (k // 4)] = True
        allowed[4 + q, :k] = True
    timed(args.limit, "constrain", lambda: m.constrain(quarter, allowed))
    OUT["quarter_table"] = both_kernels("a quarter of the blocks each")
    write_out()
    timed(args.limit, "clamp 0.05", lambda: m.clamp(draw < 0.05))
    OUT["quarter_table_and_5_percent_clamped"] = both_kernels("a quarter of the blocks each, 5 % clamped")
    timed(args.limit, "unclamp", m.unclamp)
    timed(args.limit, "unconstrain", m.unconstrain)
    OUT["unheld_again"] = sweeps("unheld again, production kernel", {})
    for key in ("quarter_table", "quarter_table_and_5_percent_clamped"):
        OUT[key]["production_held_over_unheld"] = OUT[key]["production_held"]["median_ms"] / OUT["unheld_again"]["median_ms"]
    timed(args.limit, "close", m.close)
    write_out()


if __name__ == "__main__":
    main()
