"""CPU checks of the partition distances (include/bisbm.h, "Partition distances and posterior modes"): the three symbols, the
grouping into modes on hand-made matrices, the numpy statement of the definition (the reference of the GPU tests in
tests/test_gpu_partition_distances.py) with its properties, and the refusals of `mcmc --modes` that need no device."""
import ctypes as C
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")


# ---- the definition in numpy: integer tables with np.add.at, exact sums with math.fsum ------------------------------------
def numpy_contingency(lc, ld, Kc, Kd):
    """n_rs [Kc, Kd] of two label vectors (global labels)."""
    t = np.zeros((Kc, Kd), dtype=np.int64)
    np.add.at(t, (np.asarray(lc, dtype=np.int64), np.asarray(ld, dtype=np.int64)), 1)
    return t


def xlnx_sum(counts):
    """sum of x ln x over the positive entries, every term rounded once (log, product), the sum exact (fsum)."""
    x = np.asarray(counts, dtype=np.float64).ravel()
    x = x[x > 0]
    return math.fsum((x * np.log(x)).tolist())


def numpy_vi(lc, ld, Kc, Kd):
    t = numpy_contingency(lc, ld, Kc, Kd)
    n = len(lc)
    return (xlnx_sum(t.sum(axis=1)) + xlnx_sum(t.sum(axis=0)) - 2.0 * xlnx_sum(t)) / n


def numpy_entropy(lc, Kc):
    n = len(lc)
    return math.log(n) - xlnx_sum(np.bincount(np.asarray(lc, dtype=np.int64), minlength=Kc)) / n


def numpy_conditional_entropy(lc, ld, Kc, Kd):
    """H(c | d) = - sum_rs (n_rs / n) ln (n_rs / b_s), straight from its definition."""
    t = numpy_contingency(lc, ld, Kc, Kd).astype(np.float64)
    n, b = len(lc), t.sum(axis=0)
    terms = [-(t[r, s] / n) * math.log(t[r, s] / b[s]) for r in range(Kc) for s in range(Kd) if t[r, s] > 0]
    return math.fsum(terms)


def vi_tolerance(n, kac, kbc, kad, kbd):
    """|VI_device - VI_exact| <= (2 cells + 2 (K_c + K_d) + 16) 2^-52 ln n: each of the three sums has non-negative terms, each
    term carries a log of at most 1 ulp and one product rounding, any order of adding T terms is within T 2^-53 relative of the
    exact sum, and each sum is at most n ln n."""
    cells = kac * kad + kbc * kbd
    return (2 * cells + 2 * (kac + kbc + kad + kbd) + 16) * 2.0 ** -52 * math.log(n)


def h_tolerance(n, ka, kb):
    """The same bound with H's share of the terms: one sum of K_c terms."""
    return (2 * (ka + kb) + 16) * 2.0 ** -52 * math.log(n)


def relabel(lab, na, ka, kb, rng):
    """The same partition in another numbering (a random permutation of the blocks within each type)."""
    perm = np.concatenate([rng.permutation(ka), ka + rng.permutation(kb)])
    return perm[np.asarray(lab, dtype=np.int64)].astype(np.uint32)


def move_nodes(lab, na, ka, kb, frac, rng):
    """`frac` of the nodes sent to a random block of their type."""
    lab = np.array(lab, dtype=np.uint32)
    n = len(lab)
    pick = rng.choice(n, size=int(frac * n), replace=False)
    lab[pick] = np.where(pick < na, rng.integers(0, ka, len(pick)), ka + rng.integers(0, kb, len(pick))).astype(np.uint32)
    return lab


def random_labels(na, nb, ka, kb, rng):
    return np.concatenate([rng.integers(0, ka, na), ka + rng.integers(0, kb, nb)]).astype(np.uint32)


# ---- 1. ABI ------------------------------------------------------------------------------------------------------------------
def test_the_three_symbols_are_exported_and_bound():
    if not os.path.exists(B.LIB_PATH):
        B.build()
    raw = C.CDLL(B.LIB_PATH)
    for name in ("bisbm_partition_distances", "bisbm_partition_contingency", "bisbm_partition_modes"):
        assert hasattr(raw, name), name
        assert name in B.ABI, name
    assert B.lib().bisbm_abi_version() == 3
    assert callable(B.BlockModel.partition_distances) and callable(B.BlockModel.partition_contingency)
    assert callable(B.BlockModel.partition_modes) and callable(B.partition_modes)


# ---- 2. modes on hand-made matrices ------------------------------------------------------------------------------------------
def _six():
    vi = np.full((6, 6), 1.0)
    np.fill_diagonal(vi, 0.0)

    def put(i, j, x):
        vi[i, j] = vi[j, i] = x
    put(0, 2, 0.1), put(2, 5, 0.1), put(0, 5, 0.3), put(1, 3, 0.12)
    return vi


def test_modes_join_through_linkage_and_pick_medoids():
    mode, med = B.partition_modes(_six(), 0.15)
    assert mode.dtype == np.uint32 and med.dtype == np.uint32
    assert mode.tolist() == [0, 1, 0, 1, 2, 0]
    assert med.tolist() == [2, 1, 4]  # 2 is nearest to {0, 5}; {1, 3} tie -> the lowest; 4 is alone


def test_modes_threshold_zero_and_above_the_maximum():
    vi = _six()
    vi[1, 3] = vi[3, 1] = 0.0
    mode, med = B.partition_modes(vi, 0.0)
    assert mode.tolist() == [0, 1, 2, 1, 3, 4] and med.tolist() == [0, 1, 2, 4, 5]
    mode, med = B.partition_modes(_six(), 5.0)
    assert mode.tolist() == [0] * 6 and len(med) == 1
    sums = _six().sum(axis=1)
    assert med[0] == int(np.argmin(sums))
    mode, med = B.partition_modes(np.zeros((1, 1)), 0.0)
    assert mode.tolist() == [0] and med.tolist() == [0]


def test_modes_refusals():
    L = B.lib()
    out = np.zeros(4, dtype=np.uint32)
    nm = C.c_uint32()
    one = np.zeros(1)
    assert L.bisbm_partition_modes(0, B._p(one, B._f64p), 0.1, B._p(out, B._u32p), None, C.byref(nm)) == B.BISBM_ERR_INVALID_ARG
    for bad in (-0.1, float("nan")):
        with pytest.raises(B.BisbmError) as e:
            B.partition_modes(_six(), bad)
        assert e.value.code == B.BISBM_ERR_INVALID_ARG and "threshold" in str(e.value)
    vi = _six()
    vi[0, 4] = float("nan")
    with pytest.raises(B.BisbmError) as e:
        B.partition_modes(vi, 0.1)
    assert e.value.code == B.BISBM_ERR_INVALID_ARG and "NaN" in str(e.value)
    vi = _six()
    vi[3, 4] = 0.5
    with pytest.raises(B.BisbmError) as e:
        B.partition_modes(vi, 0.1)
    assert e.value.code == B.BISBM_ERR_INVALID_ARG and "symmetric" in str(e.value) and "[3][4]" in str(e.value)
    with pytest.raises(ValueError):
        B.partition_modes(np.zeros((2, 3)), 0.1)


# ---- 3. the numpy statement and its properties ---------------------------------------------------------------------------------
CASES = [(400, 600, 4, 6), (12000, 8000, 8, 3), (50000, 50000, 32, 32), (50000, 50000, 64, 64)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d+%d_n%d" % (c[2], c[3], c[0] + c[1]))
def test_numpy_definition_properties(case):
    na, nb, ka, kb = case
    n, K = na + nb, ka + kb
    rng = np.random.default_rng(ka * 1000 + kb)
    truth = syn.contiguous_labels(na, nb, ka, kb)
    tol = vi_tolerance(n, ka, kb, ka, kb)
    same = relabel(truth, na, ka, kb, rng)
    moved = move_nodes(same, na, ka, kb, 0.05, rng)
    rand = random_labels(na, nb, ka, kb, rng)
    # a partition and a relabelling of itself
    assert abs(numpy_vi(truth, same, K, K)) <= tol
    assert (numpy_contingency(truth, same, K, K) > 0).sum() == K
    # no cell mixes the types
    t = numpy_contingency(moved, rand, K, K)
    assert t[:ka, ka:].sum() == 0 and t[ka:, :ka].sum() == 0 and t.sum() == n
    for x, y in ((truth, moved), (moved, rand), (truth, rand)):
        v, w = numpy_vi(x, y, K, K), numpy_vi(y, x, K, K)
        assert abs(v - w) <= tol                                                            # symmetry
        assert v >= -tol and v <= numpy_entropy(x, K) + numpy_entropy(y, K) + tol           # 0 <= VI <= H(c) + H(d)
        split = numpy_conditional_entropy(x, y, K, K) + numpy_conditional_entropy(y, x, K, K)
        assert abs(v - split) <= 2 * tol                                                    # VI = H(c|d) + H(d|c)
    assert 0 < numpy_vi(truth, moved, K, K) < numpy_vi(truth, rand, K, K)
    # chains of different shapes: the table is K_c x K_d
    merged = np.where(truth == ka - 1, ka - 2, truth) if ka > 1 else truth
    merged = np.where(merged >= ka, merged - 1, merged).astype(np.uint32)  # ka - 1 + kb blocks
    v = numpy_vi(merged, truth, K - 1, K)
    assert abs(v - (numpy_entropy(truth, K) - numpy_entropy(merged, K - 1))) <= tol  # a refinement: VI = H(fine) - H(coarse)


def test_order_of_the_adds_stays_far_inside_the_tolerance():
    """The bound leaves room for any order of adding the terms: numpy's own sum forwards, backwards and shuffled stays within a
    small part of it (the reference alone sits far inside)."""
    na, nb, ka, kb = 50000, 50000, 32, 32
    K, n = ka + kb, na + nb
    rng = np.random.default_rng(3)
    truth = syn.contiguous_labels(na, nb, ka, kb)
    other = move_nodes(relabel(truth, na, ka, kb, rng), na, ka, kb, 0.05, rng)
    t = numpy_contingency(truth, other, K, K)
    exact = numpy_vi(truth, other, K, K)

    def ordered(order):
        def s(c):
            x = np.asarray(c, dtype=np.float64).ravel()
            x = x[x > 0]
            terms = (x * np.log(x))[order(len(x))]
            acc = 0.0
            for v in terms.tolist():
                acc += v
            return acc
        return (s(t.sum(axis=1)) + s(t.sum(axis=0)) - 2.0 * s(t)) / n
    worst = max(abs(ordered(o) - exact) for o in (lambda k: np.arange(k), lambda k: np.arange(k)[::-1], lambda k: rng.permutation(k)))
    assert worst <= 0.05 * vi_tolerance(n, ka, kb, ka, kb)


# ---- 4. the CLI's refusals -----------------------------------------------------------------------------------------------------
def test_cli_refuses_bad_modes_before_touching_a_device(tmp_path):
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    if not os.path.exists(cli):
        B.build(force=True)
    el = os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist")
    out = tmp_path / "modes.txt"

    def run(*args):
        r = subprocess.run([cli, *args], capture_output=True, text=True)
        return r.returncode, r.stdout, r.stderr
    base = ("-e", el, "-y", "18", "14", "-n", "9", "9", "7", "7", "-z", "2", "2")
    rc, so, se = run(*base, "--modes", str(out), "0.1")
    assert rc == 1 and so == "" and "--marginalize" in se
    rc, so, se = run(*base, "--marginalize", "--modes", str(out))
    assert rc == 1 and so == "" and "Two arguments" in se
    rc, so, se = run(*base, "--marginalize", "--modes", str(out), "0.1", "0.2")
    assert rc == 1 and so == "" and "Two arguments" in se
    rc, so, se = run(*base, "--marginalize", "--modes")
    assert rc == 1 and so == "" and "--modes" in se  # (the parser's own: the required argument is missing)
    for bad in ("-0.5", "nan", "inf", "abc", "0.1x"):
        rc, so, se = run(*base, "--marginalize", "--modes", str(out), bad)
        assert rc == 1 and so == "" and "finite number >= 0" in se, (bad, se)
    assert not out.exists()
