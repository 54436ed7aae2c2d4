"""CPU tests of the anchored modes and of the distances to reference partitions (include/bisbm.h, "Anchored modes",
"Distances to reference partitions"): the exported symbols, the argument checks of marginalize_modes and the CLI (all reached
without a device), the numpy model of the nearest-anchor rule, and the margins of the two-mode pool of
tests/test_mode_marginals.py that the GPU tests' expectations rest on."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_mode_marginals import TWO_MODES, _Untouched, two_mode_pool
from test_partition_distances import numpy_vi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
NONE = B.MODE_NONE


def nearest_anchor(vi, threshold):
    """The rule of a sample: per row of vi [chains, modes] the column of the least VI (ties -> the lowest mode) if that VI is
    <= threshold, MODE_NONE otherwise."""
    vi = np.asarray(vi, dtype=np.float64)
    best = vi.argmin(axis=1)  # (the first of equal minima)
    return np.where(vi[np.arange(len(vi)), best] <= threshold, best, NONE).astype(np.uint32)


def numpy_vi_to(labels_by_chain, refs, K, ref_K=None):
    """VI [chains, refs] of every chain's labels with every reference (numpy_vi of tests/test_partition_distances.py)."""
    ref_K = [K] * len(refs) if ref_K is None else ref_K
    return np.array([[max(numpy_vi(lab, ref, K, ref_K[g]), 0.0) for g, ref in enumerate(refs)] for lab in labels_by_chain])


def test_the_new_symbols_are_exported():
    for name in ("bisbm_partition_distances_to", "bisbm_marginals_set_mode_anchors", "bisbm_marginals_get_mode_assignment"):
        assert name in B.ABI and hasattr(B.lib(), name)
    assert B.lib().bisbm_abi_version() == 3
    for member in ("partition_distances_to", "marginals_set_mode_anchors", "marginals_mode_assignment"):
        assert callable(getattr(B.BlockModel, member))
    hpp = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "host", "bisbm.hpp")).read()
    for member in ("partition_distances_to", "marginals_set_mode_anchors", "marginals_mode_assignment"):
        assert member + "(" in hpp
    # without a handle every call is refused before anything is touched
    L = B.lib()
    assert L.bisbm_partition_distances_to(None, 0, None, 0, None, None, None, None, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_marginals_set_mode_anchors(None, 0, None, 1.0) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_marginals_get_mode_assignment(None, None, None, None, None) == B.BISBM_ERR_INVALID_ARG


def test_marginalize_modes_checks_the_new_arguments():
    m = _Untouched()
    with pytest.raises(ValueError, match="reassign"):
        B.marginalize_modes(m, 1, 2, 1, threshold=0.5, tempering=[1.0, 1.5])
    with pytest.raises(ValueError, match="grouping"):
        B.marginalize_modes(m, 1, 2, 1, mode_of_chain=[0, 0, 1, 1, 0, 1], reassign=True)
    with pytest.raises(ValueError, match="exactly one"):
        B.marginalize_modes(m, 1, 2, 1, reassign=True)


def test_cli_refuses_reassign_without_mode_marginals():
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    if not os.path.exists(cli):
        B.build(force=True)
    el = os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist")
    base = [cli, "-e", el, "-y", "18", "14", "-z", "2", "2", "-n", "9", "9", "7", "7", "--marginalize"]
    r = subprocess.run(base + ["--modes", "m.txt", "0.5", "--reassign"], capture_output=True, text=True)
    assert (r.returncode, r.stdout) == (1, "")
    assert r.stderr.startswith("--reassign counts every sample into the mode of its nearest anchor: it needs --mode_marginals")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert "--reassign" in r.stderr


def test_nearest_anchor_model():
    vi = [[0.2, 0.5, 0.9], [0.7, 0.3, 0.3], [0.4, 0.4, 0.1], [2.0, 1.5, 1.5], [0.6, 0.6, 0.6]]
    assert nearest_anchor(vi, 1.0).tolist() == [0, 1, 2, NONE, 0]
    assert nearest_anchor(vi, 0.3).tolist() == [0, 1, 2, NONE, NONE]  # (<=: a VI at the threshold is within it)
    assert nearest_anchor(vi, 0.0).tolist() == [NONE] * 5
    assert nearest_anchor(vi, float("inf")).tolist() == [0, 1, 2, 1, 0]
    assert nearest_anchor([[0.0, 0.0]], 0.0).tolist() == [0]


def test_margins_of_the_two_mode_pool():
    """What the GPU tests of the anchored modes expect of the TWO_MODES pool with anchors P and Q, from numpy alone: the gaps are
    far wider than any rounding of the device's sums (1e-10)."""
    t = TWO_MODES
    K = t["ka"] + t["kb"]
    P, Q, starts = two_mode_pool()
    vi = numpy_vi_to(starts, [P, Q], K)
    near_p, near_q = vi[0::2], vi[1::2]
    assert near_p[:, 0].max() <= 0.717 and near_p[:, 1].min() >= 1.691
    assert near_q[:, 1].max() <= 0.741 and near_q[:, 0].min() >= 1.662
    assert nearest_anchor(vi, 1.0).tolist() == [0, 1] * 8
    at = nearest_anchor(vi, 0.6)
    assert np.flatnonzero(at == 0).tolist() == [0, 12, 14] and np.flatnonzero(at == 1).tolist() == [3, 7]
    assert (at == NONE).sum() == 11
    best = np.sort(vi.min(axis=1))
    below, above = best[best <= 0.6].max(), best[best > 0.6].min()
    assert abs(below - 0.584) < 5e-4 and abs(above - 0.609) < 5e-4
