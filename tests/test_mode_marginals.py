"""CPU tests of the mode-resolved marginals (include/bisbm.h, "Mode-resolved marginals"): the exported symbols, the argument
checks of marginalize_modes and the CLI's refusals (all reached without a device), and the numpy model of a two-mode pool --
what the GPU tests compare the device with -- on the construction of the first GPU test."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_align import agreement, aligned_sample, relabelled_planted_starts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

TWO_MODES = dict(na=300, nb=200, ka=4, kb=4, chains=16, noise=0.1)


def two_mode_pool():
    """(P, Q, starts): P = contiguous labels, Q = P read na / (2 ka) resp. nb / (2 kb) nodes further on, cyclically, per type;
    16 chains next to P (the even ones, seed 100) and next to Q (the odd ones, seed 200), each in its own numbering."""
    t = TWO_MODES
    na, nb, ka, kb = t["na"], t["nb"], t["ka"], t["kb"]
    P = syn.contiguous_labels(na, nb, ka, kb)
    Q = np.concatenate([P[(np.arange(na) + na // (2 * ka)) % na], P[na + (np.arange(nb) + nb // (2 * kb)) % nb]]).astype(np.uint32)
    sp = relabelled_planted_starts(P, na, ka, kb, t["chains"] // 2, noise=t["noise"], seed=100)
    sq = relabelled_planted_starts(Q, na, ka, kb, t["chains"] // 2, noise=t["noise"], seed=200)
    return P, Q, np.array([(sq if c % 2 else sp)[c // 2] for c in range(t["chains"])])


def mode_sample(labels_by_chain, mode_of_chain, refs, na, ka, kb):
    """One mode-resolved sample: aligned_sample applied to each mode's chains with that mode's reference ->
    (counts [M, n, kmax], {chain: perm}, {chain: overlap total})."""
    labels_by_chain = np.asarray(labels_by_chain)
    moc = np.asarray(mode_of_chain, dtype=np.int64)
    counts = np.zeros((len(refs), labels_by_chain.shape[1], max(ka, kb)), dtype=np.int64)
    perms, totals = {}, {}
    for g, ref in enumerate(refs):
        members = np.flatnonzero(moc == g)
        counts[g], p, t = aligned_sample(labels_by_chain[members], ref, na, ka, kb)
        for i, c in enumerate(members):
            perms[int(c)], totals[int(c)] = p[i], int(t[i])
    return counts, perms, totals


def test_the_new_symbols_are_exported():
    for name in ("bisbm_marginals_set_modes", "bisbm_marginals_get_modes", "bisbm_marginals_set_mode_reference",
                 "bisbm_marginals_get_mode_reference", "bisbm_marginals_get_mode", "bisbm_marginals_map_mode"):
        assert name in B.ABI and hasattr(B.lib(), name)
    header = open(os.path.join(ROOT, "include", "bisbm.h")).read()
    assert "#define BISBM_MODE_NONE 0xffffffffu" in header and B.MODE_NONE == 0xFFFFFFFF
    assert B.lib().bisbm_abi_version() == 3
    assert callable(B.marginalize_modes) and callable(B.mode_assignment)
    for member in ("marginals_set_modes", "marginals_modes"):
        assert callable(getattr(B.BlockModel, member))
    hpp = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "host", "bisbm.hpp")).read()
    for member in ("marginals_set_modes", "marginals_modes", "marginals_set_mode_reference", "marginals_get_mode", "marginals_map_mode"):
        assert member + "(" in hpp
    # without a handle every call is refused before anything is touched
    assert B.lib().bisbm_marginals_set_modes(None, 0, None) == B.BISBM_ERR_INVALID_ARG
    assert B.lib().bisbm_marginals_map_mode(None, 0, None, None) == B.BISBM_ERR_INVALID_ARG


class _Untouched:
    """A model that marginalize_modes must refuse before it runs anything."""
    n_chains = 6
    shard = None  # (one rank)

    def __getattr__(self, name):
        raise AssertionError("the model was used (%s) before the arguments were checked" % name)


def test_marginalize_modes_checks_its_arguments():
    m = _Untouched()
    with pytest.raises(ValueError, match="exactly one"):
        B.marginalize_modes(m, 1, 2, 1, threshold=0.5, mode_of_chain=[0, 0, 1, 1, 0, 1])
    with pytest.raises(ValueError, match="exactly one"):
        B.marginalize_modes(m, 1, 2, 1)
    with pytest.raises(ValueError, match="6 chains"):
        B.marginalize_modes(m, 1, 2, 1, mode_of_chain=[0, 1, 0])

    class _Spread(_Untouched):
        class shard:
            world_size = 2
    with pytest.raises(ValueError, match="across ranks"):
        B.marginalize_modes(_Spread(), 1, 2, 1, threshold=0.5)


def test_mode_assignment_from_an_array_and_from_a_grouping():
    moc, M = B.mode_assignment([1, B.MODE_NONE, 0, 1], 4)
    assert M == 2 and moc.dtype == np.uint32 and moc.tolist() == [1, B.MODE_NONE, 0, 1]
    grouping = {"chains": np.array([4, 1, 2]), "mode": np.array([0, 1, 0]), "medoids": np.array([4, 1])}
    moc, M = B.mode_assignment(grouping, 6)
    assert M == 2 and moc.tolist() == [B.MODE_NONE, 1, 0, B.MODE_NONE, 0, B.MODE_NONE]
    with pytest.raises(ValueError):
        B.mode_assignment([B.MODE_NONE] * 3, 3)
    with pytest.raises(ValueError):
        B.mode_assignment([0, -1, 0], 3)
    with pytest.raises(ValueError):
        B.mode_assignment({"chains": [7], "mode": [0], "medoids": [7]}, 6)


def test_cli_refuses_mode_marginals_without_modes_or_with_tempering():
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    if not os.path.exists(cli):
        B.build(force=True)
    el = os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist")
    base = [cli, "-e", el, "-y", "18", "14", "-z", "2", "2", "-n", "9", "9", "7", "7", "--marginalize"]
    r = subprocess.run(base + ["--mode_marginals", "out"], capture_output=True, text=True)
    assert (r.returncode, r.stdout) == (1, "")
    assert r.stderr == "--mode_marginals counts one histogram per mode: it needs --modes (with --marginalize) for the grouping.\n"
    r = subprocess.run(base + ["--modes", "m.txt", "0.5", "--mode_marginals", "out", "--tempering", "1", "2", "--chains", "4", "--rng", "philox"],
                       capture_output=True, text=True)
    assert (r.returncode, r.stdout) == (1, "")
    assert r.stderr.startswith("--mode_marginals gives every chain a mode of its own: it cannot be combined with --tempering")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert "--mode_marginals PREFIX" in r.stderr


def test_model_of_a_two_mode_pool():
    """8 chains near P and 8 near Q: counted per mode each MAP is its partition exactly, without a tie; pooled onto one
    reference the MAP describes neither (0.76 of P, 0.744 of Q with the library's solver)."""
    t = TWO_MODES
    na, ka, kb = t["na"], t["ka"], t["kb"]
    P, Q, labs = two_mode_pool()
    base = np.where(np.arange(len(P)) >= na, ka, 0)
    moc = np.arange(t["chains"]) % 2
    counts, perms, totals = mode_sample(labs, moc, [labs[0], labs[1]], na, ka, kb)
    for g, truth in enumerate((P, Q)):
        assert (counts[g].sum(axis=1) == t["chains"] // 2).all()
        assert agreement(counts[g].argmax(axis=1) + base, truth, na, ka, kb) == 1.0
        top2 = np.sort(counts[g], axis=1)[:, -2:]
        assert (top2[:, 1] > top2[:, 0]).all()
    assert (perms[0] == np.arange(ka + kb)).all() and totals[0] == len(P)
    pooled = aligned_sample(labs, labs[0], na, ka, kb)[0].argmax(axis=1) + base
    assert agreement(pooled, P, na, ka, kb) <= 0.8 and agreement(pooled, Q, na, ka, kb) <= 0.8
