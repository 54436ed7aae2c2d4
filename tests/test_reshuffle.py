"""Pair reshuffles (include/bisbm.h, "Pair reshuffles") without a device: the host model (distributed.numpy_reshuffle_*, which
the GPU tests hold the kernel to) against literal loops on hand-made inputs, the binding, and the refusals that need no device."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
R, S = 3, 5  # the pair of the hand-made cases (global labels)


# --------------------------------------------------------------------------------------------------------------- the pair
def _literal_pairs(ka, kb):
    """the enumeration of step 2, written out: type a first, each type lexicographically"""
    return [(t, r, s) for t, k in ((0, ka), (1, kb)) for r in range(k) for s in range(r + 1, k)]


@pytest.mark.parametrize("ka,kb", [(3, 2), (1, 4), (4, 1), (2, 2), (70, 3), (1, 2)])
def test_the_pair_is_the_literal_enumeration(ka, kb):
    pairs = _literal_pairs(ka, kb)
    N = len(pairs)
    assert N == ka * (ka - 1) // 2 + kb * (kb - 1) // 2
    for x in list(range(0, 2 ** 32, 2 ** 32 // 997)) + [2 ** 32 - 1]:
        assert D.numpy_reshuffle_pair(x, ka, kb) == pairs[(x * N) // 2 ** 32]
    # every pair comes up, the first at x = 0 and the last at the largest word
    assert D.numpy_reshuffle_pair(0, ka, kb) == pairs[0] and D.numpy_reshuffle_pair(2 ** 32 - 1, ka, kb) == pairs[-1]
    assert {D.numpy_reshuffle_pair((i * 2 ** 32 + 2 ** 31) // N, ka, kb) for i in range(N)} == set(pairs)


def test_a_shape_without_a_pair_has_none():
    assert D.numpy_reshuffle_pair(12345, 1, 1) is None


# ------------------------------------------------------------------------------------------------------------- the launch
def _literal_launch(bits, r, s):
    lab = []
    for b in bits:
        lab.append(s if b else r)
    if all(x != r for x in lab):
        lab[0] = r
    if all(x != s for x in lab):
        lab[len(lab) - 1] = s
    return lab


def test_launch_fix_ups():
    assert D.numpy_reshuffle_launch([0, 0, 0, 0], R, S) == [R, R, R, S]  # all bits 0: the last member gets s
    assert D.numpy_reshuffle_launch([1, 1, 1, 1], R, S) == [R, S, S, S]  # all bits 1: member 0 gets r
    assert D.numpy_reshuffle_launch([0, 0], R, S) == [R, S] and D.numpy_reshuffle_launch([1, 1], R, S) == [R, S]
    assert D.numpy_reshuffle_launch([1, 0, 1], R, S) == [S, R, S]
    rng = np.random.default_rng(5)
    for _ in range(200):
        bits = (rng.random(int(rng.integers(2, 12))) < rng.random()).astype(int).tolist()
        got = D.numpy_reshuffle_launch(bits, R, S)
        assert got == _literal_launch(bits, R, S) and R in got and S in got


# --------------------------------------------------------------------------------------------------------------- the step
def _literal_step(dS_o, c_is_r, free, beta, u=None, forced_to_r=None):
    """step 5 (free scan: u) and one member of steps 6 and 7 (forced: forced_to_r), written out"""
    if not free:
        if forced_to_r is not None and forced_to_r != c_is_r:
            return forced_to_r, 0.0, True  # the forced move of a member that is not free
        return c_is_r, 1.0, False
    dS = {"c": 0.0, "o": dS_o}
    dS_min = min(dS["c"], dS["o"])
    w = {}
    for key in ("c", "o"):
        x = beta * (dS[key] - dS_min)
        w[key] = 0.0 if x > 700.0 else float(np.exp(-x))  # (numpy's exponential, as the model's default)
    w_r, w_s = (w["c"], w["o"]) if c_is_r else (w["o"], w["c"])
    Z = w_r + w_s
    P_r, P_s = w_r / Z, w_s / Z
    to_r = (u < P_r) if forced_to_r is None else forced_to_r
    f = P_r if to_r else P_s
    return to_r, f, f == 0.0


def test_a_member_that_is_not_free_stays():
    for c_is_r in (True, False):
        assert D.numpy_reshuffle_step(-50.0, c_is_r, False, 1.0, u=0.99) == (c_is_r, 1.0, False)
        assert D.numpy_reshuffle_step(None, c_is_r, False, 1.0, forced_to_r=c_is_r) == (c_is_r, 1.0, False)


def test_a_forced_move_of_a_member_that_is_not_free_kills_the_pass_and_the_move_is_rejected():
    for c_is_r in (True, False):
        to_r, f, dead = D.numpy_reshuffle_step(None, c_is_r, False, 1.0, forced_to_r=not c_is_r)
        assert (to_r, f, dead) == (not c_is_r, 0.0, True) == _literal_step(None, c_is_r, False, 1.0, forced_to_r=not c_is_r)
    for u_acc in (0.0, 0.5):
        assert D.numpy_reshuffle_accept(-1e9, 1e9, (0.5, 1), (0.0, 0), 1.0, u_acc) == (0.0, False)


def test_a_zero_factor_kills_the_pass():
    # beta * dS_o > 700: the weight of o is an exact 0.0, and a member forced there has the factor 0.0
    assert D.numpy_reshuffle_step(701.0, True, True, 1.0, forced_to_r=False) == (False, 0.0, True)
    assert D.numpy_reshuffle_step(350.6, False, True, 2.0, forced_to_r=True) == (True, 0.0, True)
    assert D.numpy_reshuffle_step(701.0, True, True, 1.0, forced_to_r=True) == (True, 1.0, False)
    # ... and 700 itself is not cut
    to_r, f, dead = D.numpy_reshuffle_step(700.0, True, True, 1.0, forced_to_r=False)
    assert f == float(np.exp(-700.0)) / (1.0 + float(np.exp(-700.0))) and f > 0.0 and not dead
    # a free scan never draws a block of weight 0.0
    for u in (0.0, np.nextafter(1.0, 0.0)):
        assert D.numpy_reshuffle_step(701.0, True, True, 1.0, u=u) == (True, 1.0, False)
        assert D.numpy_reshuffle_step(-701.0, True, True, 1.0, u=u) == (False, 1.0, False)


def test_u_exactly_at_P_r_goes_to_s():
    for dS_o, c_is_r in ((0.0, True), (1.25, True), (-0.5, False), (2.0, False)):
        P_r = _literal_step(dS_o, c_is_r, True, 1.0, forced_to_r=True)[1]
        assert 0.0 < P_r < 1.0
        assert D.numpy_reshuffle_step(dS_o, c_is_r, True, 1.0, u=P_r)[0] is False
        assert D.numpy_reshuffle_step(dS_o, c_is_r, True, 1.0, u=np.nextafter(P_r, 0.0))[0] is True
    assert D.numpy_reshuffle_step(0.0, True, True, 1.0, u=0.5) == (False, 0.5, False)  # (dS_o = 0: P_r = 0.5 exactly)


def test_random_steps_against_the_literal_loop():
    rng = np.random.default_rng(7)
    for _ in range(500):
        dS_o = round(float(rng.normal(0, 4)), 2) * (300.0 if rng.random() < 0.1 else 1.0)
        c_is_r, free, beta, u = bool(rng.random() < 0.5), bool(rng.random() < 0.9), float(rng.choice([0.5, 1.0, 5.0 / 3.0])), float(rng.random())
        assert D.numpy_reshuffle_step(dS_o, c_is_r, free, beta, u=u) == _literal_step(dS_o, c_is_r, free, beta, u=u)
        forced = bool(rng.random() < 0.5)
        assert D.numpy_reshuffle_step(dS_o, c_is_r, free, beta, forced_to_r=forced) == _literal_step(dS_o, c_is_r, free, beta, forced_to_r=forced)


# ------------------------------------------------------------------------------------------------ Q and the acceptance
def test_the_mantissa_and_exponent_carry_5000_small_factors():
    m, e = D.numpy_reshuffle_q([1e-3] * 5000)
    assert 1e-3 ** 5000 == 0.0  # (a plain product underflows)
    assert 0.5 <= m < 1.0
    # log2 of the product is 5000 log2(1e-3), to the rounding of 5000 multiplies
    assert abs((math.log2(m) + e) - 5000 * math.log2(1e-3)) < 1e-8
    assert D.numpy_reshuffle_q([]) == (0.5, 1) and D.numpy_reshuffle_q([1.0, 1.0]) == (0.5, 1)
    assert D.numpy_reshuffle_q([0.25, 0.0, 0.5]) == (0.0, 0)
    # the literal loop
    mm, ee = math.frexp(1.0)
    for f in (0.3, 0.7, 1e-200, 1e-200, 0.9):
        mm, e2 = math.frexp(mm * f)
        ee += e2
    assert D.numpy_reshuffle_q([0.3, 0.7, 1e-200, 1e-200, 0.9]) == (mm, ee)
    # ... and two Q of thousands of members still give a finite ratio
    A, acc = D.numpy_reshuffle_accept(0.0, 0.0, D.numpy_reshuffle_q([1e-3] * 5000), D.numpy_reshuffle_q([1e-3] * 4999 + [2e-3]), 1.0, 0.9)
    assert abs(A - 2.0) < 1e-9 and acc


def _literal_accept(dS_fwd, dS_rev, q_fwd, q_rev, beta, u_acc):
    if q_rev[0] == 0.0:
        return 0.0, False
    dS = dS_fwd - dS_rev
    lnA = (0.0 - beta * dS) + (math.log(q_rev[0] / q_fwd[0]) + float(q_rev[1] - q_fwd[1]) * 0.6931471805599453)
    try:
        A = math.exp(lnA)
    except OverflowError:
        A = math.inf
    return A, u_acc < A


def test_the_acceptance_is_the_literal_combination():
    # A >= 1: accepted whatever u_acc is
    for u_acc in (0.0, np.nextafter(1.0, 0.0)):
        A, acc = D.numpy_reshuffle_accept(-3.0, 1.0, (0.75, -4), (0.75, -4), 1.0, u_acc)
        assert A == math.exp(4.0) and acc
    assert D.numpy_reshuffle_accept(-2000.0, 0.0, (0.5, 1), (0.5, 1), 1.0, 0.999) == (math.inf, True)
    # A = 1 exactly (nothing changed, equal Q): u_acc < 1 always
    assert D.numpy_reshuffle_accept(0.5, 0.5, (0.625, -7), (0.625, -7), 2.0, np.nextafter(1.0, 0.0)) == (1.0, True)
    # uphill with equal Q: the plain Metropolis rule
    A, acc = D.numpy_reshuffle_accept(2.0, 0.0, (0.5, 1), (0.5, 1), 1.0, 0.2)
    assert abs(A - math.exp(-2.0)) < 1e-15 and not acc
    assert D.numpy_reshuffle_accept(2.0, 0.0, (0.5, 1), (0.5, 1), 1.0, 0.1)[1]
    # Q_rev / Q_fwd enters as it stands: a proposal four times as likely forwards as backwards is accepted a quarter as often
    A = D.numpy_reshuffle_accept(0.0, 0.0, (0.5, 3), (0.5, 1), 1.0, 0.0)[0]
    assert abs(A - 0.25) < 1e-15
    rng = np.random.default_rng(11)
    for _ in range(300):
        args = (float(rng.normal(0, 30)), float(rng.normal(0, 30)), (float(rng.uniform(0.5, 1)), int(rng.integers(-9000, 2))),
                (float(rng.uniform(0.5, 1)), int(rng.integers(-9000, 2))), float(rng.choice([1.0, 5.0 / 3.0])), float(rng.random()))
        got, want = D.numpy_reshuffle_accept(*args), _literal_accept(*args)
        assert got[1] == want[1] and (got[0] == want[0] or abs(got[0] - want[0]) <= 1e-12 * want[0])


# ------------------------------------------------------------------------------------------------------------ the binding
def test_the_calls_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "bisbm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+bisbm_reshuffle_run\s*\(\s*bisbm_handle\s+h\s*,\s*uint64_t\s+moves\s*,\s*uint32_t\s+scans\s*,\s*double\s+beta\s*,\s*uint64_t\s*\*\s*accepted_out", code)
    assert re.search(r"\bint\s+bisbm_reshuffle_get_last\s*\(\s*bisbm_handle\s+h\s*,\s*bisbm_reshuffle_record\s*\*\s*out", code)
    assert re.search(r"#define\s+BISBM_ABI_VERSION\s+3\b", code)
    assert B.ABI["bisbm_reshuffle_run"][1][1:4] == [C.c_uint64, C.c_uint32, C.c_double]
    if not os.path.exists(B.LIB_PATH):
        B.build()
    raw = C.CDLL(B.LIB_PATH)
    assert hasattr(raw, "bisbm_reshuffle_run") and hasattr(raw, "bisbm_reshuffle_get_last")
    assert B.PHILOX_PURPOSE_RESHUFFLE == 10
    kernels = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "csrc", "bisbm_kernels.hpp")).read()
    assert re.search(r"PHX_HEATBATH\s*=\s*9\b", kernels) and re.search(r"PHX_RESHUFFLE\s*=\s*10\b", kernels)
    # the record as Python reads it is the header's struct, field for field
    body = re.search(r"typedef struct bisbm_reshuffle_record \{(.*?)\}", code, flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().split(" ", 1)[-1]) if decl.strip()]
    assert names == [f[0] for f in B.ReshuffleRecord._fields_], names
    assert C.sizeof(B.ReshuffleRecord) == 80
    for method in ("reshuffle", "reshuffle_last"):
        assert callable(getattr(B.BlockModel, method))
    for fn in ("numpy_reshuffle_launch", "numpy_reshuffle_step", "numpy_reshuffle_accept"):
        assert getattr(B, fn) is getattr(D, fn)
    hpp = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "host", "bisbm.hpp")).read()
    assert "bisbm_reshuffle_run" in hpp and "bisbm_reshuffle_get_last" in hpp
    assert "bisbm_reshuffle.hip" in open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "build.py")).read()


def test_a_null_handle_is_an_invalid_argument():
    L = B.lib()
    assert L.bisbm_reshuffle_run(None, 1, 3, 1.0, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_reshuffle_get_last(None, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_reshuffle_get_total(None, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_debug_exp(None, None, 0, None) == B.BISBM_ERR_INVALID_ARG


def test_without_a_device_there_is_no_handle_to_reshuffle():
    """the new calls need a handle, and without a HIP device there is none: create fails loudly, as for every other call"""
    import torch
    if torch.cuda.is_available():
        return  # (tests/test_gpu_reshuffle.py runs the calls)
    rowptr = np.array([0, 1, 2], dtype=np.uint64)
    col = np.array([1, 0], dtype=np.uint32)
    with pytest.raises(B.BisbmError) as e:
        B.BlockModel([0, 1], [0, 1], 2, 1, 1, 1.0, (rowptr, col)).reshuffle(1)
    assert e.value.code == B.BISBM_ERR_NO_DEVICE


class _NoSweeps:
    """a model that must not be asked to run anything"""
    n, shard = 10, None

    def __getattr__(self, name):
        raise AssertionError("the model was touched: " + name)


def test_marginalize_refuses_reshuffles_with_a_ladder_and_negative_counts():
    with pytest.raises(ValueError, match="tempering"):
        B.marginalize(_NoSweeps(), 1, 1, 1, tempering=[1.0, 2.0], reshuffles=2)
    with pytest.raises(ValueError, match="negative"):
        B.marginalize(_NoSweeps(), 1, 1, 1, reshuffles=-1)
    with pytest.raises(ValueError, match="negative"):
        B.marginalize(_NoSweeps(), 1, 1, 1, reshuffles=1, reshuffle_scans=-1)


CLI = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
EL = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
BASE = ["-e", EL, "-y", "500", "500", "-z", "3", "3", "-n", "167", "167", "166", "167", "167", "166"]
CLI_REFUSALS = [
    (["--reshuffle", "2", "--rng", "philox"], "--reshuffle", "--marginalize"),
    (["--marginalize", "--reshuffle_scans", "2", "--rng", "philox"], "--reshuffle_scans", "--reshuffle"),
    (["--marginalize", "--reshuffle", "2", "--tempering", "1", "2", "--chains", "2", "--rng", "philox"], "--reshuffle", "--tempering"),
    (["--marginalize", "--reshuffle", "2", "--rng", "mt19937-compat"], "--reshuffle", "Philox"),
    (["--marginalize", "--reshuffle", "0", "--rng", "philox"], "Invalid --reshuffle", ">= 1"),
    (["--marginalize", "--reshuffle", "some", "--rng", "philox"], "Invalid --reshuffle", ">= 1"),
    (["--marginalize", "--reshuffle", "2", "--reshuffle_scans", "-1", "--rng", "philox"], "Invalid --reshuffle_scans", ">= 0"),
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
    assert "--reshuffle M" in r.stdout + r.stderr and "--reshuffle_scans" in r.stdout + r.stderr
