"""Population annealing (include/bisbm.h, "Population annealing") without a device: bisbm_population_offspring -- the weights,
the systematic resampling and the parent map of one step -- against the numpy restatement the GPU tests hold a step of a handle
to, its refusals, the symbols, and the CLI's refusals and --help."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
PHX_RESAMPLE = 8
JUST_BELOW_1 = 1.0 - 2.0 ** -53


# ---------------------------------------------------------------------------------------------------- numpy restatement
def model_step(S, delta, u):
    """Steps 2-5 of the definition -> (offspring, parent, log_ratio, margin).  margin: the least distance of an a_k - u with
    k < C - 1 from an integer -- np.exp and the library's exp may differ in the last bit, so the integers of the two are the
    same only when no ceil() sits on an edge; a_{C-1} = C is exact in both."""
    S = np.asarray(S, dtype=np.float64)
    C = len(S)
    s_min = S.min()
    w = np.exp(-delta * (S - s_min))
    c = np.cumsum(w)  # (sequential, ascending)
    W = c[-1]
    log_ratio = -delta * s_min + np.log(W / C)
    a = np.minimum(C * c / W, C)  # (the min: fl(fl(C * W) / W) can be C + 1 ulp where the trailing weights vanish)
    a[-1] = C
    x = a - u
    margin = float(np.abs(x[:-1] - np.round(x[:-1])).min()) if C > 1 else 1.0
    ceil = (np.floor(a) + (a - np.floor(a) > u)).astype(np.int64)  # ceil(a - u), exactly (a - u itself rounds)
    n = np.diff(np.concatenate([[0], ceil]))
    parent = np.arange(C)
    parent[n == 0] = np.repeat(np.arange(C), np.maximum(n - 1, 0))
    return n.astype(np.uint32), parent.astype(np.uint32), float(log_ratio), margin


def draw_S(C, seed=0):
    return 1000.0 + 3.0 * np.random.default_rng(1234 + seed).standard_normal(C)


def check_invariants(n, parent):
    C = len(n)
    assert int(n.sum()) == C
    assert ((parent == np.arange(C)) == (n >= 1)).all()
    assert (np.bincount(parent, minlength=C) == n).all()


@pytest.mark.parametrize("C", [1, 2, 7, 300, 1024])
def test_offspring_delta_zero_is_the_identity(C):
    for u in (0.0, 0.37, JUST_BELOW_1):
        n, parent, lr = B.population_offspring(draw_S(C), 0.0, u)
        assert (n == 1).all() and (parent == np.arange(C)).all() and lr == 0.0


@pytest.mark.parametrize("C", [1, 2, 7, 300, 1024])
@pytest.mark.parametrize("u", [0.0, 0.37, JUST_BELOW_1])
def test_offspring_against_the_numpy_model(C, u):
    S = draw_S(C)
    mn, mparent, mlr, margin = model_step(S, 0.7, u)
    assert margin >= 1e-9, margin  # (a condition on the inputs, not a tolerance)
    n, parent, lr = B.population_offspring(S, 0.7, u)
    assert (n == mn).all() and (parent == mparent).all()
    assert abs(lr - mlr) <= 1e-12 * abs(mlr)
    check_invariants(n, parent)
    if C == 300 and u == 0.37:
        print("C = 300, delta = 0.7, u = 0.37: margin %.3g, %d dead slots, largest family %d" % (margin, int((n == 0).sum()), int(n.max())))
        assert (n == 0).sum() > C // 2 and n.max() > 10  # (a step that really resamples)


@pytest.mark.parametrize("C", [1, 2, 7, 300, 1024])
def test_offspring_large_delta_one_chain_takes_every_slot(C):
    # (a draw whose lowest value leads by 0.8: the runner-up's weight is exp(-40), C of them are still nothing beside u)
    S = next(s for s in (draw_S(C, seed) for seed in range(100)) if C == 1 or np.partition(s, 1)[1] - s.min() >= 0.8)
    mn, mparent, mlr, margin = model_step(S, 50.0, 0.37)
    assert margin >= 1e-9, margin
    n, parent, lr = B.population_offspring(S, 50.0, 0.37)
    assert (parent == np.argmin(S)).all() and n[np.argmin(S)] == C
    assert (n == mn).all() and (parent == mparent).all() and abs(lr - mlr) <= 1e-12 * abs(mlr)
    check_invariants(n, parent)


@pytest.mark.parametrize("C", [2, 7, 300, 1024])
def test_offspring_two_equal_minima_share(C):
    S = draw_S(C)
    i, j = sorted(np.random.default_rng(C).choice(C, 2, replace=False))
    S[i] = S[j] = S.min() - 1.0
    mn, mparent, mlr, margin = model_step(S, 50.0, 0.37)
    assert margin >= 1e-9, margin
    n, parent, lr = B.population_offspring(S, 50.0, 0.37)
    assert (n == mn).all() and (parent == mparent).all() and abs(lr - mlr) <= 1e-12 * abs(mlr)
    assert n[i] == (C + 1) // 2 and n[j] == C // 2 and n[i] + n[j] == C  # (u = 0.37 < 1/2: the odd one goes to the first)
    check_invariants(n, parent)


@pytest.mark.parametrize("C", [7, 300, 1023])
def test_offspring_vanishing_trailing_weights_at_u_zero(C):
    """delta = 50 and trailing chains 2 above the minimum: their weights vanish beside W, c_k == W before the last slot, and the
    rounded (C * W) / W exceeds C for about one W in ten.  Without the min in a_k, u = 0 then gives ceil = C + 1 and the last
    count -1.  No model comparison here: a_k sits ON an integer, so only what holds whatever the last bit of exp is asserted."""
    over = 0
    for x in np.linspace(0.001, 0.03, 200):
        S = np.full(C, 1002.0)
        S[0], S[1] = 1000.0, 1000.0 + x
        W = np.cumsum(np.exp(-50.0 * (S - 1000.0)))[-1]
        over += (C * W) / W > C
        for u in (0.0, 2.0 ** -53, 0.37, JUST_BELOW_1):
            n, parent, lr = B.population_offspring(S, 50.0, u)
            check_invariants(n, parent)
            if u <= 0.37:  # (a rounded (C * W) / W one ulp BELOW C rightly leaves the last slot its own at u = 1 - 2^-53)
                assert n[0] + n[1] == C and (parent <= 1).all()
            mn, mparent, _, _ = model_step(S, 50.0, u)
            check_invariants(mn.astype(np.int64), mparent)
    assert over >= 5, over  # (the inputs do reach the case)
    # the draw of the report
    n, parent, _ = B.population_offspring([1000, 1000.015, 1002, 1002, 1002, 1002, 1002], 50.0, 0.0)
    assert n.tolist() == [5, 2, 0, 0, 0, 0, 0] and parent.tolist() == [0, 1, 0, 0, 0, 0, 1]


def test_offspring_parent_map_by_hand():
    """S chosen so that the weights are 1, 1/4, 1, 1/16 ... exactly: delta = ln 4, S in units of 1."""
    # w = [1, 4^-1, 1, 4^-2, 1], W = 3.3125, a = 5 c / W = [1.509, 1.887, 3.396, 3.491, 5]; u = 0.45: ceil(a - u) = [2, 2, 3, 4, 5]
    n, parent, lr = B.population_offspring([10.0, 11.0, 10.0, 12.0, 10.0], np.log(4.0), 0.45)
    assert n.tolist() == [2, 0, 1, 1, 1] and parent.tolist() == [0, 0, 2, 3, 4]
    assert abs(lr - (-np.log(4.0) * 10.0 + np.log(3.3125 / 5))) < 1e-12 * 14


def test_offspring_refusals():
    S = draw_S(5)
    for bad in (lambda: B.population_offspring([], 0.5, 0.5),
                lambda: B.population_offspring([1.0, np.nan], 0.5, 0.5),
                lambda: B.population_offspring([1.0, np.inf], 0.5, 0.5),
                lambda: B.population_offspring(S, -1e-9, 0.5),
                lambda: B.population_offspring(S, np.nan, 0.5),
                lambda: B.population_offspring(S, np.inf, 0.5),
                lambda: B.population_offspring(S, 0.5, 1.0),
                lambda: B.population_offspring(S, 0.5, -1e-9),
                lambda: B.population_offspring(S, 0.5, np.nan)):
        with pytest.raises(B.BisbmError) as e:
            bad()
        assert e.value.code == B.BISBM_ERR_INVALID_ARG and len(str(e.value)) > 20
    # outputs are optional, S is not
    L = B.lib()
    s = np.ascontiguousarray(S)
    assert L.bisbm_population_offspring(5, s.ctypes.data_as(B._f64p), 0.5, 0.5, None, None, None) == B.BISBM_OK
    assert L.bisbm_population_offspring(5, None, 0.5, 0.5, None, None, None) == B.BISBM_ERR_INVALID_ARG


def test_validate_population_temps():
    assert B.validate_population_temps([4, 2.5, 2.5, 1]).dtype == np.float32
    for bad in ([], [1.0], [1.0, 2.0], [2.0, 0.0], [2.0, -1.0], [np.inf, 1.0], [2.0, np.nan], "ab", [1e39, 1.0]):
        with pytest.raises(ValueError):
            B.validate_population_temps(bad)


def test_declared_population_symbols_are_bound():
    header = open(os.path.join(ROOT, "include", "bisbm.h")).read()
    names = ("bisbm_population_offspring", "bisbm_population_resample", "bisbm_population_run", "bisbm_population_get", "bisbm_population_reset")
    for name in names:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in B.ABI
    assert set(re.findall(r"\b(bisbm_population_\w+)\(", header)) == set(names)
    assert "#define BISBM_ABI_VERSION 3" in header and B.lib().bisbm_abi_version() == 3
    L = B.lib()
    # refused without a handle, before anything else
    assert L.bisbm_population_resample(None, 0.5, 1.0, None, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_population_run(None, 0, None, 1, None, None, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_population_get(None, None, None, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_population_reset(None) == B.BISBM_ERR_INVALID_ARG
    kernels = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "csrc", "bisbm_kernels.hpp")).read()
    assert re.search(r"constexpr uint32_t PHX_RESAMPLE = %d;" % PHX_RESAMPLE, kernels)


# ---------------------------------------------------------------------------------------------------- CLI
def _cli():
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    if not os.path.exists(cli):
        B.build(force=True)
    return cli


GRAPH = ["-e", os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist"), "-y", "18", "14", "-z", "2", "2", "-n", "9", "9", "7", "7"]
INVALID = "Invalid --population. At least 2 finite temperatures > 0 that do not rise, e.g. --population 4 2.5 1.5 1.\n"
PHILOX_ONLY = "--population runs in Philox mode only (mt19937-compat is the reference's verification path): add --rng philox.\n"


@pytest.mark.parametrize("args, message", [
    (["--population", "2"], INVALID),
    (["--population", "1", "2"], INVALID),
    (["--population", "2", "1", "1.5"], INVALID),
    (["--population", "2", "0"], INVALID),
    (["--population", "inf", "1"], INVALID),
    (["--population", "2", "x1"], INVALID),
    (["--population", "2", "1", "--chains", "4", "-d", "3"], PHILOX_ONLY),
    (["--population", "2", "1", "--chains", "4", "--rng", "mt19937-compat"], PHILOX_ONLY),
    (["--population", "2", "1", "--marginalize"],
     "--population anneals the chains and prints the best one: it cannot be combined with --marginalize. For marginals of an annealed "
     "population use the Python interface: population_anneal, then marginalize with no burn-in.\n"),
    (["--population_sweeps", "2"], "--population_sweeps sets the sweeps per temperature of a population run: it needs --population.\n"),
    (["--population", "2", "1", "--population_sweeps", "two"], "Invalid --population_sweeps. Sweeps per temperature: an integer >= 0.\n"),
    (["--population", "2", "1", "--merge"], "--population replaces the cooling schedule of the annealing run: it cannot be combined with --merge.\n"),
])
def test_cli_population_refusals(args, message):
    """Refused with one line before the device is touched (these runs never reach bisbm_create)."""
    r = subprocess.run([_cli()] + GRAPH + args, capture_output=True, text=True)
    assert (r.returncode, r.stdout) == (1, "")
    assert r.stderr.endswith(message), r.stderr


def test_cli_population_refuses_an_initial_partition_of_other_block_counts():
    """-n gives 2 + 2 blocks, -z asks for 3 + 2: without --population the driver merges or splits down to -z first; a population
    run replaces that schedule, so it is refused -- once the partition has been read, still before the device is touched."""
    graph = [a if (i, a) != (GRAPH.index("-z") + 1, "2") else "3" for i, a in enumerate(GRAPH)]
    r = subprocess.run([_cli()] + graph + ["--rng", "philox", "--chains", "4", "--population", "2", "1"], capture_output=True, text=True)
    assert (r.returncode, r.stdout) == (1, "")
    assert r.stderr.endswith("--population replaces the cooling schedule of the annealing run: the initial partition must have the -z block counts.\n"), r.stderr


def test_cli_help_names_population():
    r = subprocess.run([_cli(), "--help"], capture_output=True, text=True)
    assert "--population arg" in r.stderr and "--population_sweeps arg (=1)" in r.stderr
    head = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "host", "mcmc_main.cpp")).read().split("#include")[0]
    assert "--population," in head and "--population_sweeps" in head


def test_cli_population_reaches_the_device():
    """A valid request gets as far as the device (without one: bisbm_create's error; with one: n labels and the step report)."""
    r = subprocess.run([_cli()] + GRAPH + ["--rng", "philox", "-d", "5", "-r", "--chains", "8", "--population", "3", "2", "1", "--population_sweeps", "2"],
                       capture_output=True, text=True)
    if r.returncode == 0:
        assert len(r.stdout.split()) == 32 and "population step 2: T 2 -> 1, log ratio" in r.stderr and "population: 2 steps, log ratio total" in r.stderr
    else:
        assert r.returncode == 3 and "no hip device" in r.stderr.lower(), r.stderr
