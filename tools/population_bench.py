"""Cost and effect of population annealing (include/bisbm.h, "Population annealing") at BASELINE configs[2] -- N = 10^6 (5e5 +
5e5), E = 10^7, 32 + 32 blocks, 1024 chains -- over the schedule T = 2 -> 0.5 in 16 geometric steps with one sweep per
temperature.  Writes profiles/population_bench.json and prints it:
  * every resampling step at the death fraction the schedule itself produces: host ms of the step (description lengths down,
    parent map, state copies), the slots copied, the bytes moved (read + written) and bytes over time, beside the ms of the sweep
    that follows on the same handle;
  * the lowest and the median description length after the same sweep budget through 1024 independent exponential anneals and
    through the population run, and the distinct-ancestor trace.
The two runs are stages of their own: each is a child process under its own time limit, and the second starts only if the first
ended well.

    python tools/population_bench.py [--quick] [--chains 1024] [--limit 300]"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS, T_HOT, T_COLD, SWEEPS_PER_STEP, BURN_IN = 16, 2.0, 0.5, 1, 2


def model(args):
    B = importlib.import_module("bipartitesbm-mcmc_amd")
    syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")
    na = nb = 50_000 if args.quick else 500_000
    E, k = 20 * na, 32
    a, b = syn.planted_edges(na, nb, E, k, k, seed=1)
    rp, cl = B.edge_to_adj((a, b), na + nb)
    m = B.BlockModel(syn.contiguous_labels(na, nb, k, k), syn.types_vector(na, nb), 2 * k, k, k, 1.0, (rp, cl), n_chains=args.chains, seed=1)
    m.shuffle_bisbm()
    return B, m, {"n": na + nb, "edges": E, "blocks": "%d+%d" % (k, k), "chains": args.chains}


def stage_population(args):
    B, m, out = model(args)
    temps = B.validate_population_temps(np.geomspace(T_HOT, T_COLD, STEPS + 1))
    m.run_sweeps(BURN_IN, float(temps[0]))
    stride = (m.n + 255) // 256 * 256
    state_bytes = stride + 4 * (m.KA * m.KB + 2 * m.K + m.K * (m.max_degree + 1)) + 8
    steps = []
    for k in range(1, len(temps)):
        t0 = time.perf_counter()
        parent, lr = m.population_resample(1.0 / float(temps[k - 1]), 1.0 / float(temps[k]))
        step_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        m.run_sweeps(SWEEPS_PER_STEP, float(temps[k]))
        sweep_ms = (time.perf_counter() - t0) * 1e3 / SWEEPS_PER_STEP
        dead = int((parent != np.arange(len(parent))).sum())
        moved = 2 * dead * state_bytes
        steps.append({"T": float(temps[k]), "log_ratio": lr, "dead": dead, "dead_fraction": dead / len(parent), "step_host_ms": step_ms,
                      "bytes_moved": moved, "GB_per_s_over_the_whole_step": moved / step_ms / 1e6, "sweep_host_ms": sweep_ms,
                      "sweep_kernel_ms": m.last_sweep_timing()[0] / SWEEPS_PER_STEP, "step_fraction_of_sweep": step_ms / sweep_ms,
                      "distinct": int(len(np.unique(m.population_state()["ancestor"])))})
    S = m.entropy()
    out.update({"temps": [float(t) for t in temps], "sweeps_per_step": SWEEPS_PER_STEP, "burn_in_sweeps": BURN_IN, "state_bytes_per_chain": state_bytes,
                "steps": steps, "distinct": [s["distinct"] for s in steps], "log_ratio_total": m.population_state()["log_ratio_total"],
                "population_lowest": float(S.min()), "population_median": float(np.median(S))})
    m.close()
    return out


def stage_independent(args):
    B, m, out = model(args)
    budget = BURN_IN + STEPS * SWEEPS_PER_STEP
    alpha = (T_COLD / T_HOT) ** (1.0 / (budget * m.n))
    t0 = time.perf_counter()
    B.MetropolisHasting().anneal(m, B.exponential_schedule, [T_HOT, alpha], budget * m.n, 1 << 60)
    S = m.entropy()
    out = {"independent_sweeps": budget, "independent_alpha": alpha, "independent_host_ms_per_sweep": (time.perf_counter() - t0) * 1e3 / budget,
           "independent_lowest": float(S.min()), "independent_median": float(np.median(S))}
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a 10^5-node graph instead of configs[2] (a first look)")
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--limit", type=int, default=300, help="seconds a stage may take")
    ap.add_argument("--stage", choices=["population", "independent"], help="(internal) run one stage in this process and print its JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "population_bench.json"))
    args = ap.parse_args()
    if args.stage:
        print(json.dumps({"population": stage_population, "independent": stage_independent}[args.stage](args)), flush=True)
        return 0
    out = {}
    for stage in ("population", "independent"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--stage", stage, "--chains", str(args.chains)]
        r = subprocess.run(cmd + (["--quick"] if args.quick else []), capture_output=True, text=True)
        if r.returncode != 0:  # (nothing more is started on the device after a stage that did not end well)
            sys.stderr.write("stage %s ended with status %d\n%s" % (stage, r.returncode, r.stderr))
            return 1
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
