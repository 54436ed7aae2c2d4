"""Replica exchange (include/bisbm.h, "Replica exchange") without a device: the Python-side ladder check, the numpy restatement of
an exchange round that the GPU tests hold the exchange kernel to, and the CLI's refusals and --help."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
PHX_EXCHANGE = 7


# ---------------------------------------------------------------------------------------------------- numpy restatement
def philox(seed, chain, purpose, idx):
    """Philox4x32-10 of the oracle with the engine's key and counter layout (seed; idx_lo, idx_hi, chain, purpose)."""
    import ctypes as C
    u32p = C.POINTER(C.c_uint32)
    c = np.array([idx & 0xFFFFFFFF, idx >> 32, chain, purpose], dtype=np.uint32)
    k = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    o = np.zeros(4, dtype=np.uint32)
    O.lib().orc_philox4x32_10(c.ctypes.data_as(u32p), k.ctypes.data_as(u32p), o.ctypes.data_as(u32p))
    return [int(x) for x in o]


def u53(hi, lo):
    return float(((hi << 32) | lo) >> 11) * 2.0 ** -53


def exchange_round(rung, S, ladder, seed, first_gid, r, attempted, accepted):
    """One exchange round r over the chains of one handle (first global id first_gid): rung[c] is updated in place, the per-pair
    counters too.  S: every chain's description length (f64), ladder: the temperatures as given (the library runs them as
    float32, B.validate_ladder)."""
    L = len(ladder)
    T = [float(t) for t in B.validate_ladder(ladder)]
    for g in range(len(rung) // L):
        at = {int(rung[g * L + j]): g * L + j for j in range(L)}
        for i in range(r % 2, L - 1, 2):
            a, b = at[i], at[i + 1]
            delta = (1.0 / T[i] - 1.0 / T[i + 1]) * (float(S[a]) - float(S[b]))
            U = philox(seed, first_gid + g * L, PHX_EXCHANGE, r * L + i)
            attempted[i] += 1
            if delta >= 0 or u53(U[0], U[1]) < np.exp(delta):
                accepted[i] += 1
                rung[a], rung[b] = i + 1, i
                at[i], at[i + 1] = b, a


def test_exchange_round_restatement():
    """The restatement the GPU tests hold the exchange kernel to, on the ladder as the library runs it (validate_ladder): pairs
    of the round's parity only, a swap whenever the colder chain has the larger description length, and u against exp(delta)
    otherwise with the ensemble's own stream."""
    L, seed = 4, 11
    ladder = [1.0, 1.5, 2.0, 3.0]
    rung = np.array([0, 1, 2, 3, 0, 1, 2, 3], dtype=np.uint32)
    att, acc = np.zeros(L - 1, dtype=np.uint64), np.zeros(L - 1, dtype=np.uint64)
    S_up = np.array([50.0, 40.0, 30.0, 20.0, 50.0, 40.0, 30.0, 20.0])  # colder rungs hold the longer descriptions: every swap taken
    exchange_round(rung, S_up, ladder, seed, 0, 0, att, acc)
    assert list(att) == [2, 0, 2] and list(acc) == [2, 0, 2]
    assert list(rung) == [1, 0, 3, 2, 1, 0, 3, 2]
    exchange_round(rung, S_up, ladder, seed, 0, 1, att, acc)  # odd round: pair (1, 2) -- chains 0 (rung 1) and 3 (rung 2)
    assert list(att) == [2, 2, 2] and list(acc) == [2, 2, 2] and list(rung) == [2, 0, 3, 1, 2, 0, 3, 1]
    # an uphill proposal: accepted exactly when u < exp(delta), u from (seed, ensemble's first gid, purpose 7, r L + i)
    rung = np.array([0, 1], dtype=np.uint32)
    att, acc = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    S = np.array([10.0, 10.7])
    U = philox(3, 8, PHX_EXCHANGE, 4 * 2 + 0)
    want = u53(U[0], U[1]) < np.exp((1.0 - 0.5) * (10.0 - 10.7))
    exchange_round(rung, S, [1.0, 2.0], 3, 8, 4, att, acc)
    assert int(acc[0]) == int(want) and list(rung) == ([1, 0] if want else [0, 1])


# ---------------------------------------------------------------------------------------------------- ladder check
def test_validate_ladder():
    lad = B.validate_ladder([1, 1.3, 2, 3.5])
    assert lad.dtype == np.float32 and list(lad) == [np.float32(x) for x in (1, 1.3, 2, 3.5)]
    assert list(B.validate_ladder([1.0, 1.0])) == [1.0, 1.0]  # equal temperatures are a ladder (every swap accepted)
    for bad, what in (([1.0], "at least 2"), ([], "at least 2"), ([1.0, 0.5], "non-decreasing"), ([0.0, 1.0], "> 0"),
                      ([-1.0, 1.0], "> 0"), ([1.0, float("inf")], "finite"), ([1.0, float("nan")], "finite"),
                      ([1e-50, 1.0], "> 0"), ([1.0, 1e39], "finite"), (["a", "b"], "numbers"), (None, "numbers")):
        with pytest.raises(ValueError) as e:
            B.validate_ladder(bad)
        assert what in str(e.value), (bad, str(e.value))


def test_declared_tempering_symbols_are_bound():
    for name in ("bisbm_tempering_set", "bisbm_tempering_run", "bisbm_tempering_get", "bisbm_tempering_stats"):
        assert name in B.ABI
    L = B.lib()
    # refused without a handle, before anything else
    assert L.bisbm_tempering_set(None, 0, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_tempering_run(None, 1, 1, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_tempering_get(None, None, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_tempering_stats(None, None, None, None) == B.BISBM_ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------------- CLI
def _cli():
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    if not os.path.exists(cli):
        B.build(force=True)
    return cli


GRAPH = ["-e", os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist"), "-y", "18", "14", "-z", "2", "2", "-n", "9", "9", "7", "7"]


@pytest.mark.parametrize("args, message", [
    (["--tempering", "1", "2"], "--tempering runs replica exchange for the marginals of the coldest chains: it needs --marginalize.\n"),
    (["--exchange_every", "2"], "--tempering runs replica exchange for the marginals of the coldest chains: it needs --marginalize.\n"),
    (["--marginalize", "--exchange_every", "2"], "--exchange_every sets the period of the exchange rounds: it needs --tempering.\n"),
    (["--marginalize", "--tempering", "1"],
     "Invalid --tempering. A non-decreasing ladder of at least 2 finite temperatures > 0, e.g. --tempering 1 1.5 2.5 4.\n"),
    (["--marginalize", "--tempering", "2", "1"],
     "Invalid --tempering. A non-decreasing ladder of at least 2 finite temperatures > 0, e.g. --tempering 1 1.5 2.5 4.\n"),
    (["--marginalize", "--tempering", "0", "1"],
     "Invalid --tempering. A non-decreasing ladder of at least 2 finite temperatures > 0, e.g. --tempering 1 1.5 2.5 4.\n"),
    (["--marginalize", "--tempering", "1", "inf"],
     "Invalid --tempering. A non-decreasing ladder of at least 2 finite temperatures > 0, e.g. --tempering 1 1.5 2.5 4.\n"),
    (["--marginalize", "--tempering", "1", "x2"],
     "Invalid --tempering. A non-decreasing ladder of at least 2 finite temperatures > 0, e.g. --tempering 1 1.5 2.5 4.\n"),
    (["--marginalize", "--tempering", "1", "2", "--exchange_every", "two"],
     "Invalid --exchange_every. Sweeps between exchange rounds: an integer >= 0 (0: no exchanges).\n"),
    (["--marginalize", "--tempering", "1", "2", "4", "--chains", "4", "--rng", "philox"],
     "--tempering with 3 temperatures needs --chains a multiple of 3 (got 4).\n"),
    (["--marginalize", "--tempering", "1", "2", "--chains", "6", "--devices", "0,0", "--rng", "philox"],
     "--tempering with 2 temperatures over 2 devices needs --chains a multiple of 4 (every device's share a multiple of 2; got 6).\n"),
    (["--marginalize", "--tempering", "1", "2", "--chains", "5", "--devices", "0,0", "--rng", "philox"],
     "--tempering with 2 temperatures needs --chains a multiple of 2 (got 5).\n"),
    (["--marginalize", "--tempering", "1", "2", "--chains", "4", "-d", "3"],
     "--tempering runs in Philox mode only (mt19937-compat is the reference's verification path): add --rng philox.\n"),
])
def test_cli_tempering_refusals(args, message):
    """Refused with one line before the device is touched (these runs never reach bisbm_create)."""
    r = subprocess.run([_cli()] + GRAPH + args, capture_output=True, text=True)
    assert (r.returncode, r.stdout) == (1, "")
    assert r.stderr.endswith(message), r.stderr


def test_cli_help_names_tempering():
    r = subprocess.run([_cli(), "--help"], capture_output=True, text=True)
    assert "--tempering" in r.stderr and "--exchange_every" in r.stderr


def test_cli_tempering_reaches_the_device():
    """A valid request gets as far as the device (without one: bisbm_create's error; with one: n labels and the swap report)."""
    r = subprocess.run([_cli()] + GRAPH + ["--rng", "philox", "-b", "64", "-t", "128", "-f", "32", "--chains", "8", "--marginalize",
                                           "--tempering", "1", "1.5", "2.5", "4", "--exchange_every", "2"], capture_output=True, text=True)
    if r.returncode == 0:
        assert len(r.stdout.split()) == 32 and "swap acceptance:" in r.stderr
    else:
        assert r.returncode == 3 and "no hip device" in r.stderr.lower(), r.stderr
