"""CPU tests of the block summaries (include/bisbm.h, "Block summaries"): the literal model numpy_block_sums against a triple loop
written out here, block_moments (exact zero variance, the split of the sum of squares past 2^32, mean and variance against
fractions.Fraction), the header's declarations, and the refusals that need no device."""
import importlib
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
NONE = B.MODE_NONE


def _random_pool(rs, chains, ka, kb, top=5000):
    K = ka + kb
    perms = np.array([np.concatenate([rs.permutation(ka), ka + rs.permutation(kb)]) for _ in range(chains)], dtype=np.uint32)
    quads = rs.integers(0, top, (chains, ka, kb)).astype(np.int32)
    n_rs = rs.integers(0, top, (chains, K)).astype(np.int32)
    m_rs = rs.integers(0, top, (chains, K)).astype(np.int32)
    return perms, quads, n_rs, m_rs


def test_numpy_block_sums_equal_a_loop_written_out():
    rs = np.random.default_rng(5)
    ka, kb, chains, M = 3, 5, 9, 4
    K = ka + kb
    perms, quads, n_rs, m_rs = _random_pool(rs, chains, ka, kb, top=100000)  # (squares past 2^32 among them)
    modes = np.array([0, 2, NONE, 0, 3, 3, NONE, 0, 2], dtype=np.uint32)  # mode 1 is empty, two chains are in no mode
    got = B.numpy_block_sums(perms, quads, n_rs, m_rs, modes, M, ka, kb)
    E = [[[[0, 0, 0] for _ in range(kb)] for _ in range(ka)] for _ in range(M)]
    N = [[[0, 0, 0] for _ in range(K)] for _ in range(M)]
    D = [[[0, 0, 0] for _ in range(K)] for _ in range(M)]
    terms = [0] * M

    def add(cell, x):
        x = int(x)
        cell[0] += x
        cell[1] += (x * x) & 0xFFFFFFFF
        cell[2] += (x * x) >> 32
    for c in range(chains):
        if modes[c] == NONE:
            continue
        g, pi = int(modes[c]), perms[c]
        for a in range(ka):
            for b in range(kb):
                add(E[g][int(pi[a])][int(pi[ka + b]) - ka], quads[c][a][b])
        for r in range(K):
            add(N[g][int(pi[r])], n_rs[c][r])
            add(D[g][int(pi[r])], m_rs[c][r])
        terms[g] += 1
    assert got["terms"].dtype == np.uint64 and got["terms"].tolist() == terms == [3, 0, 2, 2]
    assert got["e"].shape == (M, 3, ka, kb) and got["n"].shape == got["d"].shape == (M, 3, K)
    for g in range(M):
        for w in range(3):
            assert got["e"][g, w].tolist() == [[E[g][R][S][w] for S in range(kb)] for R in range(ka)], (g, w)
            assert got["n"][g, w].tolist() == [N[g][r][w] for r in range(K)], (g, w)
            assert got["d"][g, w].tolist() == [D[g][r][w] for r in range(K)], (g, w)
    assert not got["e"][1].any() and not got["n"][1].any() and not got["d"][1].any()
    assert got["e"][:, 2].any()  # (some square went past 2^32)
    # the sums of a mode do not depend on the numbering of the source: the totals are those of the members
    for g in (0, 2, 3):
        members = np.flatnonzero(modes == g)
        assert int(got["e"][g, 0].sum()) == int(quads[members].astype(np.int64).sum())
        assert int(got["n"][g, 0].sum()) == int(n_rs[members].astype(np.int64).sum())


def test_block_moments_of_identical_samples_have_variance_exactly_zero():
    x = np.array([[0, 1, 7], [70001, 123456789, 2**31 - 1]], dtype=np.uint64)
    for t in (1, 3, 1000, 77777):
        # (the words of t equal samples: each sample adds its own low and high half)
        lo = np.array([[(int(v) * int(v) & 0xFFFFFFFF) * t for v in row] for row in x.tolist()], dtype=np.uint64)
        hi = np.array([[(int(v) * int(v) >> 32) * t for v in row] for row in x.tolist()], dtype=np.uint64)
        mean, var = B.block_moments(x * np.uint64(t), lo, hi, t)
        assert mean.shape == var.shape == x.shape
        assert (var == 0.0).all() and (mean == x.astype(np.float64)).all(), t
    mean, var = B.block_moments(np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64), 0)
    assert np.isnan(mean).all() and np.isnan(var).all()


def test_block_moments_across_the_split_of_the_squares():
    xs = (70000, 70002)  # 70000^2 = 4.9e9 > 2^32
    assert all(x * x > 2**32 for x in xs)
    lo = sum((x * x) & 0xFFFFFFFF for x in xs)
    hi = sum((x * x) >> 32 for x in xs)
    assert hi == 2 and lo == (70000 * 70000 - 2**32) + (70002 * 70002 - 2**32)
    assert (hi << 32) + lo == sum(x * x for x in xs)
    got = B.numpy_block_sums(np.array([[0, 1], [0, 1]]), np.array([[[xs[0]]], [[xs[1]]]]), np.zeros((2, 2), dtype=np.int64),
                             np.array([[xs[0]] * 2, [xs[1]] * 2]), [0, 0], 1, 1, 1)
    assert got["e"][0, :, 0, 0].tolist() == [sum(xs), lo, hi] and got["d"][0, :, 1].tolist() == [sum(xs), lo, hi]
    mean, var = B.block_moments(got["e"][0, 0], got["e"][0, 1], got["e"][0, 2], 2)
    assert mean[0, 0] == 70001.0 and var[0, 0] == 1.0


def test_block_moments_equal_exact_fractions():
    rs = np.random.default_rng(11)
    for t, top in ((1, 10), (7, 1000), (100, 2**31 - 1), (4096, 2**31 - 1)):
        x = rs.integers(0, top, (t, 6), endpoint=True)
        s = np.array([sum(int(v) for v in col) for col in x.T], dtype=np.uint64)
        lo = np.array([sum((int(v) * int(v)) & 0xFFFFFFFF for v in col) for col in x.T], dtype=np.uint64)
        hi = np.array([sum((int(v) * int(v)) >> 32 for v in col) for col in x.T], dtype=np.uint64)
        mean, var = B.block_moments(s, lo, hi, t)
        for j in range(x.shape[1]):
            col = [int(v) for v in x[:, j]]
            mu = Fraction(sum(col), t)
            v2 = Fraction(sum(v * v for v in col), t) - mu * mu
            assert mean[j] == float(mu) and var[j] == float(v2) and var[j] >= 0.0, (t, j)


def test_the_header_declares_the_calls_and_the_version_stays():
    header = open(os.path.join(ROOT, "include", "bisbm.h")).read()
    assert "#define BISBM_ABI_VERSION 3\n" in header
    assert "#define BISBM_BLOCK_SUMS 1u" in header and "#define BISBM_BLOCK_KEEP_LAST 2u" in header
    for decl in ("int bisbm_block_sums_set(bisbm_handle h, uint32_t what);", "int bisbm_block_sums_get(bisbm_handle h, uint32_t mode, uint64_t *terms,",
                 "int bisbm_block_sums_get_last(bisbm_handle h, uint32_t chain, uint32_t *mode_out,"):
        assert decl in header, decl
    assert "2^32" in header[header.index("Block summaries"):header.index("#define BISBM_BLOCK_SUMS")]  # (the bound is stated)
    assert (B.BLOCK_SUMS, B.BLOCK_KEEP_LAST) == (1, 2)
    for name in ("bisbm_block_sums_set", "bisbm_block_sums_get", "bisbm_block_sums_get_last"):
        assert name in B.ABI and hasattr(B.lib(), name)
    assert B.lib().bisbm_abi_version() == 3
    for member in ("block_sums_set", "block_sums", "block_summary", "block_last"):
        assert callable(getattr(B.BlockModel, member))
    hpp = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "host", "bisbm.hpp")).read()
    for call in ("bisbm_block_sums_set(", "bisbm_block_sums_get(", "bisbm_block_sums_get_last("):
        assert call in hpp
    # without a handle every call is refused before anything is touched
    assert B.lib().bisbm_block_sums_set(None, 1) == B.BISBM_ERR_INVALID_ARG
    assert B.lib().bisbm_block_sums_get(None, 0, None, None, None, None) == B.BISBM_ERR_INVALID_ARG
    assert B.lib().bisbm_block_sums_get_last(None, 0, None, None, None, None) == B.BISBM_ERR_INVALID_ARG


class _Untouched:
    """A model that marginalize must refuse before it runs anything."""
    n_chains = 4
    shard = None

    def __getattr__(self, name):
        raise AssertionError("the model was used (%s) before the arguments were checked" % name)


def test_marginalize_blocks_needs_align_before_the_model_is_touched():
    with pytest.raises(ValueError, match="align=True"):
        B.marginalize(_Untouched(), 5, 2, 1, blocks=True)


def test_cli_refuses_block_summary_without_an_aligned_sample():
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    if not os.path.exists(cli):
        B.build(force=True)
    el = os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist")
    base = [cli, "-e", el, "-y", "18", "14", "-z", "2", "2", "-n", "9", "9", "7", "7"]
    for extra in (["--marginalize"], [], ["--marginalize", "--modes", "m.txt", "0.5"]):
        r = subprocess.run(base + extra + ["--block_summary", "out.txt"], capture_output=True, text=True)
        assert (r.returncode, r.stdout) == (1, ""), extra
        assert r.stderr.startswith("--block_summary sums the chains' block states in the numbering of aligned samples: it needs --marginalize with --align"), extra
    r = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert "--block_summary OUT" in r.stderr
