"""Heat-bath sweeps and greedy polishing (include/bisbm.h, "Heat-bath sweeps and greedy polishing") without a device: the host
model of the choice (distributed.numpy_heatbath_choice, which the GPU tests hold the kernel to) against a literal loop on
hand-made rows, the binding, and the refusals that need no device."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
INF = float("inf")


def _literal(dS, P, r, free, u, greedy):
    """steps 3 and 4 of the definition, written out"""
    if not free:
        return r
    if greedy:
        lowest = min(dS)
        for s in range(len(dS)):
            if dS[s] == lowest:
                return s if dS[s] < 0.0 else r
    C_s = 0.0
    for s in range(len(P)):
        C_s = P[s] if s == 0 else C_s + P[s]
        if u < C_s:
            return s
    return max(s for s in range(len(P)) if P[s] > 0.0)


QUARTERS = [0.25, 0.25, 0.25, 0.25]
# P = 0.1, 0.2, 0.3: the running sums are 0.1, 0.1 + 0.2 = 0.30000000000000004, and + 0.3 = 0.6000000000000001
TENTHS = [0.1, 0.2, 0.3, 0.4]
C1 = 0.1 + 0.2
# every P a little short, so that C of the last block rounds below 1
SHORT = [0.5 - 2.0 ** -30, 0.25, 0.25 - 2.0 ** -30, 0.0]
HEAT = [
    # name, dS, P, r, free, u, expected
    ("first_block", [0.0, 1.0, 2.0, 3.0], QUARTERS, 2, True, 0.0, 0),
    ("first_block_just_below", [0.0] * 4, QUARTERS, 2, True, np.nextafter(0.25, 0.0), 0),
    ("at_the_boundary_goes_on", [0.0] * 4, QUARTERS, 2, True, 0.25, 1),
    ("last_block", [0.0] * 4, QUARTERS, 0, True, np.nextafter(1.0, 0.0), 3),
    ("rounded_boundary_below", [0.0] * 4, TENTHS, 0, True, np.nextafter(C1, 0.0), 1),
    ("rounded_boundary_at", [0.0] * 4, TENTHS, 0, True, C1, 2),
    ("exact_tenth_is_below_the_rounded_sum", [0.0] * 4, TENTHS, 0, True, 0.3, 1),
    ("fallback_largest_positive", [0.0] * 4, SHORT, 0, True, np.nextafter(1.0, 0.0), 2),
    ("zeros_are_skipped", [0.0, 900.0, 0.0, 900.0], [0.5, 0.0, 0.5, 0.0], 0, True, 0.5, 2),
    ("zeros_first", [900.0, 900.0, 0.0, 0.5], [0.0, 0.0, 0.6, 0.4], 2, True, 0.0, 2),
    ("zero_at_the_end_never_chosen", [0.0, 0.0, 900.0], [0.5, 0.5 - 2.0 ** -40, 0.0], 0, True, np.nextafter(1.0, 0.0), 1),
    ("not_free_stays", [0.0, -5.0, -9.0], [0.0, 1.0, 0.0], 0, False, 0.9, 0),
    ("one_block", [0.0], [1.0], 0, False, 0.3, 0),
]
GREEDY = [
    ("downhill", [0.0, -1.0, -3.0, 2.0], 0, True, 2),
    ("tie_lowest_wins", [1.0, -2.0, 0.0, -2.0], 2, True, 1),
    ("tie_below_r", [-2.0, 5.0, 0.0, -2.0], 2, True, 0),
    ("minimum_is_the_zero_at_r", [3.0, 0.0, 2.0], 1, True, 1),
    ("tie_with_the_zero_at_r_does_not_move", [0.0, 4.0, 0.0], 2, True, 2),
    ("negative_zero_is_not_downhill", [-0.0, 1.0, 0.0], 2, True, 2),
    ("not_free_stays", [-4.0, 0.0, -9.0], 1, False, 1),
]


@pytest.mark.parametrize("name,dS,P,r,free,u,want", HEAT, ids=[c[0] for c in HEAT])
def test_heat_bath_choice_is_the_literal_loop(name, dS, P, r, free, u, want):
    got = D.numpy_heatbath_choice(np.array(dS), np.array(P), r, free, u, False)
    assert got == _literal(dS, P, r, free, float(u), False) == want


@pytest.mark.parametrize("name,dS,r,free,want", GREEDY, ids=[c[0] for c in GREEDY])
def test_greedy_choice_is_the_literal_loop(name, dS, r, free, want):
    P = [1.0 if s == r else 0.0 for s in range(len(dS))]  # (not looked at)
    got = D.numpy_heatbath_choice(np.array(dS), np.array(P), r, free, 0.999, True)
    assert got == _literal(dS, P, r, free, 0.999, True) == want


def test_the_hand_made_rows_are_what_they_claim():
    assert C1 > 0.3 and sum(SHORT) < 1.0
    acc = 0.0
    for y in SHORT:
        acc = acc + y
    assert acc < np.nextafter(1.0, 0.0)  # (the fallback case's u is not below C of the last block)


def test_random_rows_against_the_literal_loop():
    rng = np.random.default_rng(3)
    for _ in range(300):
        k = int(rng.integers(1, 9))
        r = int(rng.integers(0, k))
        dS = rng.normal(0, 3, k).round(1)
        dS[r] = 0.0
        w = np.exp(-(dS - dS.min())) * (rng.random(k) > 0.2)
        w[r] = max(w[r], 1e-3)
        P = w / w.sum()
        u = float(rng.random())
        for greedy in (False, True):
            assert D.numpy_heatbath_choice(dS, P, r, k > 1, u, greedy) == _literal(list(dS), list(P), r, k > 1, u, greedy)


def test_the_call_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "bisbm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+bisbm_heatbath_run\s*\(\s*bisbm_handle\s+h\s*,\s*uint64_t\s+sweeps\s*,\s*double\s+beta\s*,\s*int\s+stop_when_settled", code)
    assert re.search(r"#define\s+BISBM_ABI_VERSION\s+3\b", code)
    assert "bisbm_heatbath_run" in B.ABI
    assert B.ABI["bisbm_heatbath_run"][1][1:4] == [C.c_uint64, C.c_double, C.c_int]
    if not os.path.exists(B.LIB_PATH):
        B.build()
    assert hasattr(C.CDLL(B.LIB_PATH), "bisbm_heatbath_run")
    assert B.PHILOX_PURPOSE_HEATBATH == 9
    kernels = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "csrc", "bisbm_kernels.hpp")).read()
    assert re.search(r"PHX_RESAMPLE\s*=\s*8\b", kernels) and re.search(r"PHX_HEATBATH\s*=\s*9\b", kernels)
    for method in ("heatbath_sweeps", "polish"):
        assert callable(getattr(B.BlockModel, method))
    assert B.numpy_heatbath_choice is D.numpy_heatbath_choice
    assert "bisbm_heatbath_run" in open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "host", "bisbm.hpp")).read()
    assert "bisbm_heatbath.hip" in open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "build.py")).read()


def test_a_null_handle_is_an_invalid_argument():
    assert B.lib().bisbm_heatbath_run(None, 1, 1.0, 0, None, None) == B.BISBM_ERR_INVALID_ARG


class _NoSweeps:
    """a model that must not be asked to run anything"""
    n, shard = 10, None

    def __getattr__(self, name):
        raise AssertionError("the model was touched: " + name)


def test_marginalize_refuses_an_unknown_sampler_and_heatbath_with_a_ladder():
    for fn, args in ((B.marginalize, (_NoSweeps(), 1, 1, 1)), (B.marginalize_modes, (_NoSweeps(), 1, 1, 1, 0.1))):
        with pytest.raises(ValueError, match="sampler"):
            fn(*args, sampler="gibbs")
    with pytest.raises(ValueError, match="tempering"):
        B.marginalize(_NoSweeps(), 1, 1, 1, sampler="heatbath", tempering=[1.0, 2.0])
    with pytest.raises(ValueError, match="tempering"):
        B.marginalize_modes(_NoSweeps(), 1, 1, 1, 0.1, reassign=True, sampler="heatbath", tempering=[1.0, 2.0])


CLI = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
EL = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
BASE = ["-e", EL, "-y", "500", "500", "-z", "3", "3", "-n", "167", "167", "166", "167", "167", "166"]
CLI_REFUSALS = [
    (["--heatbath"], "--heatbath", "--marginalize"),
    (["--marginalize", "--heatbath", "--tempering", "1", "2", "--chains", "2", "--rng", "philox"], "--heatbath", "--tempering"),
    (["--marginalize", "--heatbath", "--rng", "mt19937-compat"], "--heatbath", "Philox"),
    (["--marginalize", "--polish", "5"], "--polish", "--marginalize"),
    (["--polish", "0", "--rng", "philox"], "Invalid --polish", ">= 1"),
    (["--polish", "-3", "--rng", "philox"], "Invalid --polish", ">= 1"),
    (["--polish", "many", "--rng", "philox"], "Invalid --polish", ">= 1"),
    (["--polish", "5", "-d", "1"], "--polish", "Philox"),
]


@pytest.mark.parametrize("extra,flag,word", CLI_REFUSALS, ids=[" ".join(c[0]) for c in CLI_REFUSALS])
def test_the_command_line_refuses_before_anything_runs(extra, flag, word):
    if not os.path.exists(CLI):
        B.build()
    r = subprocess.run([CLI] + BASE + extra, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stdout == "", (r.returncode, r.stdout, r.stderr)
    assert flag in r.stderr and word in r.stderr, r.stderr


def test_help_lists_the_flags():
    if not os.path.exists(CLI):
        B.build()
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=120)
    assert "--polish N" in r.stdout + r.stderr and "--heatbath" in r.stdout + r.stderr
