"""CPU tests of the chain-trace summary (include/bisbm.h, "Chain traces": bisbm_trace_summary).  It is a pure host function whose
definition fixes the order of every sum, so the model below -- plain Python loops over Python floats, one term at a time --
must reproduce it bit for bit."""
import ctypes as C
import importlib
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")


# ---- the definition as sequential Python -------------------------------------------------------------------------------------
def numpy_trace_summary(x, window=5.0):
    """(tau [C], window [C], rhat) of x [T, C]: the header's definition with every sum added one term at a time."""
    x = np.asarray(x, dtype=np.float64)
    T, Cn = x.shape
    half = T // 2
    tau, win = [], []
    for c in range(Cn):
        col = [float(v) for v in x[:, c]]
        s = 0.0
        for v in col:
            s += v
        mu = s / float(T)
        d = [v - mu for v in col]

        def gamma(k):
            g = 0.0
            for t in range(T - k):
                g += d[t] * d[t + k]
            return g / float(T)
        g0 = gamma(0)
        if g0 == 0.0:
            tau.append(math.inf), win.append(0)
            continue
        acc, M = 1.0, 0
        for k in range(1, half + 1):
            acc = acc + 2.0 * (gamma(k) / g0)
            M = k
            if float(k) >= window * acc:
                break
        tau.append(acc), win.append(M)
    means, var = [], []
    for j in range(2 * Cn):
        c, t0 = j % Cn, (0 if j < Cn else T - half)
        seq = [float(v) for v in x[t0:t0 + half, c]]
        s = 0.0
        for v in seq:
            s += v
        m = s / float(half)
        q = 0.0
        for v in seq:
            e = v - m
            q += e * e
        means.append(m), var.append(q / float(half - 1))
    sv = 0.0
    for v in var:
        sv += v
    sm = 0.0
    for v in means:
        sm += v
    W, mbar = sv / float(2 * Cn), sm / float(2 * Cn)
    sb = 0.0
    for v in means:
        e = v - mbar
        sb += e * e
    Bn = sb / (float(2 * Cn) - 1.0)
    rhat = math.nan if W == 0.0 else math.sqrt(((float(half - 1) / float(half)) * W + Bn) / W)
    return np.array(tau, dtype=np.float64), np.array(win, dtype=np.uint32), rhat


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want):
    assert (_bits(got[0]) == _bits(want[0])).all(), (got[0], want[0])
    assert got[1].dtype == np.uint32 and (got[1] == want[1]).all(), (got[1], want[1])
    assert _bits([got[2]])[0] == _bits([want[2]])[0], (got[2], want[2])


def _ar1(phi, seed, T, Cn, discard=200):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((discard + T, Cn))
    x = np.zeros_like(e)
    for t in range(1, discard + T):
        x[t] = phi * x[t - 1] + e[t]
    return x[discard:]


# ---- 1. bit equality with the model --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,Cn,seed", [(4, 1, 0), (5, 3, 1), (37, 2, 2), (200, 5, 3), (301, 1, 4)])
def test_random_series_are_bit_equal_to_the_model(T, Cn, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, Cn)) * 3.0 + rng.standard_normal(Cn) * 10.0
    for window in (5.0, 1.0, 0.3, 40.0):
        _same(B.trace_summary(x, window), numpy_trace_summary(x, window))
    y = _ar1(0.9, seed, T, Cn, discard=10)  # correlated: the window runs further
    _same(B.trace_summary(y), numpy_trace_summary(y))


def test_a_constant_chain_never_moved():
    x = np.random.default_rng(0).standard_normal((50, 3))
    x[:, 1] = 7.25
    got = B.trace_summary(x)
    _same(got, numpy_trace_summary(x))
    assert got[0][1] == math.inf and got[1][1] == 0
    assert np.isfinite(got[0][[0, 2]]).all() and (got[1][[0, 2]] >= 1).all()
    tau, win, rhat = B.trace_summary(np.full((10, 2), 3.0))  # every chain constant: W == 0
    assert (tau == math.inf).all() and (win == 0).all() and math.isnan(rhat)
    _same((tau, win, rhat), numpy_trace_summary(np.full((10, 2), 3.0)))


def test_the_alternating_series():
    """x_t = (-1)^t, T = 100: mu = 0, gamma(0) = 1, gamma(1) = -99 / 100, so acc = 1 + 2 (-0.99) = -0.98 and 1 >= 5 (-0.98) stops
    at the first lag."""
    x = np.array([1.0 if t % 2 == 0 else -1.0 for t in range(100)])
    tau, win, rhat = B.trace_summary(x)  # (a 1-d series is one chain)
    assert tau.shape == (1,) and tau[0] == 1.0 + 2.0 * (-0.99) == -0.98 and win[0] == 1
    _same((tau, win, rhat), numpy_trace_summary(x[:, None]))


def test_two_chains_offset_by_three_do_not_agree():
    x = np.random.default_rng(5).standard_normal((400, 2))
    x[:, 1] += 3.0
    got = B.trace_summary(x)
    _same(got, numpy_trace_summary(x))
    assert got[2] > 1.9
    assert B.trace_summary(x[:, :1])[2] < 1.05  # one of them alone is fine


# ---- 2. AR(1): tau near (1 + phi) / (1 - phi) --------------------------------------------------------------------------------
def test_ar1_tau_is_within_a_factor_two_of_the_analytic_value():
    """phi = 0.8: tau = (1 + phi) / (1 - phi) = 9.  With numpy alone, seeds 0 - 2 gave tau in 6.7 ... 14.0 and windows 34 ... 70
    for this T; the bound asserted is the factor 2."""
    x = _ar1(0.8, 0, 4000, 4)
    assert x.shape == (4000, 4)
    tau, win, rhat = B.trace_summary(x)
    print("tau", tau, "window", win, "rhat", rhat)
    assert (tau > 4.5).all() and (tau < 18.0).all()
    assert (win < 2000).all() and (win >= 5.0 * tau).all()
    assert rhat < 1.01
    _same((tau, win, rhat), numpy_trace_summary(x))


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    x = np.random.default_rng(1).standard_normal((20, 2))
    for bad in (lambda: B.trace_summary(x[:3]),                      # T = 3
                lambda: B.trace_summary(np.zeros((8, 0))),           # C = 0
                lambda: B.trace_summary(x, 0.0), lambda: B.trace_summary(x, -1.0),
                lambda: B.trace_summary(x, math.inf), lambda: B.trace_summary(x, math.nan)):
        with pytest.raises(B.BisbmError) as e:
            bad()
        assert e.value.code == B.BISBM_ERR_INVALID_ARG
    for poison in (math.nan, math.inf, -math.inf):
        y = x.copy()
        y[7, 1] = poison
        with pytest.raises(B.BisbmError) as e:
            B.trace_summary(y)
        assert e.value.code == B.BISBM_ERR_INVALID_ARG and "x[7][1]" in str(e.value)
    with pytest.raises(ValueError):
        B.trace_summary(np.zeros((4, 2, 2)))
    # any output may be NULL
    L = B.lib()
    v = np.ascontiguousarray(x)
    rhat = C.c_double()
    assert L.bisbm_trace_summary(20, 2, B._p(v, B._f64p), 5.0, None, None, C.byref(rhat)) == B.BISBM_OK
    assert rhat.value == B.trace_summary(x)[2]
    assert L.bisbm_trace_summary(20, 2, B._p(v, B._f64p), 5.0, None, None, None) == B.BISBM_OK
    assert L.bisbm_trace_summary(20, 2, None, 5.0, None, None, None) == B.BISBM_ERR_INVALID_ARG


def test_cli_refuses_a_bad_trace_before_touching_a_device(tmp_path):
    import subprocess
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    if not os.path.exists(cli):
        B.build(force=True)
    el = os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist")
    out = str(tmp_path / "trace.txt")

    def run(*args):
        r = subprocess.run([cli, "-e", el, "-y", "18", "14", *args], capture_output=True, text=True)
        return r.returncode, r.stdout, r.stderr
    rc, so, err = run("--trace", out, "4")
    assert rc == 1 and so == "" and "it needs --marginalize" in err
    for bad in (["--trace", out], ["--trace", out, "4", "5"]):
        rc, so, err = run("--marginalize", *bad)
        assert rc == 1 and so == "" and err.startswith("Invalid --trace. Two arguments")
    for depth in ("0", "1025", "x", "3.5", "-2"):
        rc, so, err = run("--marginalize", "--trace", out, depth)
        assert rc == 1 and so == "" and (err.startswith("Invalid --trace.") or "unrecognised option" in err), depth
    assert not os.path.exists(out)
    assert "--trace OUT DEPTH" in run("--help")[2]


def test_the_six_symbols_are_bound_and_the_drivers_take_a_trace():
    import inspect
    mz = importlib.import_module("bipartitesbm-mcmc_amd.marginalize")
    for name in ("bisbm_trace_set", "bisbm_trace_record", "bisbm_trace_reset", "bisbm_trace_get_lags", "bisbm_trace_get_series",
                 "bisbm_trace_summary"):
        assert name in B.ABI and hasattr(B.lib(), name), name
    assert B.lib().bisbm_abi_version() == 3
    for fn in (mz.marginalize, mz.marginalize_modes):
        assert inspect.signature(fn).parameters["trace"].default is None
    with pytest.raises(ValueError):
        mz._trace_start(None, -1)
