"""CPU checks of the fold-in queries (include/bisbm.h, "Fold-in queries"): the host statement of the definition
(distributed.numpy_foldin_posterior / numpy_foldin_tables / numpy_foldin_rows, the reference of the GPU tests) against a literal
Python double loop, the invariants of the definition, the six symbols declared, exported and bound, the tile constants the Python
side states against the kernel header's, and the refusals of `mcmc --foldin` that need no device.

The row-sum invariants hold up to rounding: all terms are non-negative, so the bound is n_candidates 2^-52 relative (the
derivation of test_gpu_pair_scores.py's docstring)."""
import importlib
import math
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed

EPS = 2.0 ** -52
SYMBOLS = ["bisbm_foldin_set", "bisbm_foldin_accumulate", "bisbm_foldin_reset", "bisbm_foldin_get_posteriors", "bisbm_foldin_get_row",
           "bisbm_foldin_topk"]
NA, NB, KA, KB = 17, 13, 4, 4


def _case():
    """17 + 13 nodes, 4 + 4 blocks: type-a block 3 is empty (n_r = 0), type-a block 2 holds only the isolated node 16 (m_r = 0,
    n_r = 1), type-b block 3 holds only the isolated node 29"""
    rs = np.random.default_rng(11)
    labels = np.concatenate([rs.integers(0, 2, NA), KA + rs.integers(0, 3, NB)]).astype(np.uint32)
    labels[16], labels[29] = 2, KA + 3
    edges = [(int(u), NA + int(v)) for u, v in zip(rs.integers(0, 16, 60), rs.integers(0, 12, 60))]
    K = KA + KB
    m = np.zeros((K, K), dtype=np.int32)
    deg = np.zeros(NA + NB, dtype=np.int64)
    for u, v in edges:
        m[labels[u], labels[v]] += 1
        m[labels[v], labels[u]] += 1
        deg[u] += 1
        deg[v] += 1
    m_r = m.sum(axis=1).astype(np.int32)
    n_r = np.bincount(labels, minlength=K).astype(np.int32)
    assert n_r[3] == 0 and (n_r[2], m_r[2]) == (1, 0) and (n_r[KA + 3], m_r[KA + 3]) == (1, 0)
    return labels, m, m_r, n_r, deg


def _literal(labels, m, m_r, n_r, deg, qtype, nbrs, alpha):
    """the definition as written, one float at a time"""
    own0, oth0, k_own, k_oth = (KA, 0, KB, KA) if qtype else (0, KA, KA, KB)
    mant, ex = [0.0] * k_own, [None] * k_own
    for r in range(k_own):
        if n_r[own0 + r] <= 0:
            continue
        mant[r], ex[r] = math.frexp(float(n_r[own0 + r]))
        for w in nbrs:
            s = int(labels[w]) - oth0
            x = (float(m[own0 + r][oth0 + s]) + alpha) / (float(m_r[own0 + r]) + alpha * float(k_oth))
            mant[r] = mant[r] * x
            mant[r], e2 = math.frexp(mant[r])
            ex[r] += e2
    E = max(e for e in ex if e is not None)
    w = [0.0 if ex[r] is None or ex[r] - E < -1000 else math.ldexp(mant[r], ex[r] - E) for r in range(k_own)]
    Z = w[0]
    for x in w[1:]:
        Z = Z + x
    P = [x / Z for x in w]
    g = []
    for s in range(k_oth):
        acc = 0.0
        for r in range(k_own):
            if m_r[own0 + r] == 0 or P[r] == 0.0:
                continue
            acc = acc + (P[r] * float(m[own0 + r][oth0 + s])) / float(m_r[own0 + r])
        g.append(0.0 if m_r[oth0 + s] == 0 else acc / float(m_r[oth0 + s]))
    oth = range(0, NA) if qtype else range(NA, NA + NB)
    own = range(NA, NA + NB) if qtype else range(0, NA)
    rec = [0.0 if deg[v] == 0 else (float(len(nbrs)) * float(deg[v])) * g[int(labels[v]) - oth0] for v in oth]
    sim = [P[int(labels[v]) - own0] for v in own]
    return P, g, rec, sim


QUERIES = [(0, [NA + 1, NA + 4, NA + 4, NA + 7]),   # type a, a repeated neighbour
           (1, [0, 5, 9]),                          # type b
           (0, [NA + 3]),                           # d = 1
           (1, [2]),
           (0, [NA + 12, NA + 0, NA + 12]),         # an isolated neighbour (its block has m_r = 0)
           (1, [16, 3])]                            # likewise for type b


def test_numpy_model_is_the_double_loop():
    labels, m, m_r, n_r, deg = _case()
    for alpha in (1.0, 0.001):
        for qtype, nbrs in QUERIES:
            P, g = D.numpy_foldin_tables(labels, m, m_r, n_r, KA, qtype, nbrs, alpha)
            rec, sim = D.numpy_foldin_rows(labels, deg, NA, KA, qtype, len(nbrs), P, g)
            wP, wg, wrec, wsim = _literal(labels, m, m_r, n_r, deg, qtype, nbrs, alpha)
            for got, want in ((P, wP), (g, wg), (rec, wrec), (sim, wsim)):
                got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
                assert got.shape == want.shape and (got.view(np.uint64) == want.view(np.uint64)).all(), (qtype, nbrs)
            assert (D.numpy_foldin_posterior(labels, m, m_r, n_r, KA, qtype, nbrs, alpha) == P).all()
            if not qtype:
                assert P[3] == 0.0 and P[2] > 0.0  # the empty block; the block without edges keeps a weight through alpha
    assert D.numpy_foldin_tables is B.numpy_foldin_tables and D.numpy_foldin_rows is B.numpy_foldin_rows
    assert D.numpy_foldin_posterior is B.numpy_foldin_posterior


def test_posterior_is_normalised_and_the_rows_add_up():
    labels, m, m_r, n_r, deg = _case()
    for qtype, nbrs in QUERIES:
        P, g = D.numpy_foldin_tables(labels, m, m_r, n_r, KA, qtype, nbrs, 0.5)
        rec, sim = D.numpy_foldin_rows(labels, deg, NA, KA, qtype, len(nbrs), P, g)
        own = slice(KA, KA + KB) if qtype else slice(0, KA)
        assert abs(P.sum() - 1.0) <= 4 * EPS and (P >= 0).all()
        assert (rec >= 0).all() and (sim >= 0).all()
        want = len(nbrs) * float(P[m_r[own] > 0].sum())
        assert abs(rec.sum() - want) <= len(rec) * EPS * want, (rec.sum(), want)
        want = float((P * n_r[own]).sum())
        assert abs(sim.sum() - want) <= len(sim) * EPS * want, (sim.sum(), want)


def test_four_hundred_small_factors_stay_finite():
    """400 factors of about 1e-3 multiply to 1e-1200, far below the smallest double: the plain product is 0.0 for every block
    and the posterior 0 / 0; mantissa and exponent kept apart give a finite, normalised one"""
    ka, kb, na = 3, 2, 6
    K = ka + kb
    m = np.zeros((K, K), dtype=np.int32)
    m[:ka, ka:] = [[1, 999], [2, 998], [3, 2997]]
    m[ka:, :ka] = m[:ka, ka:].T
    m_r = m.sum(axis=1).astype(np.int32)
    n_r = np.array([2, 2, 2, 1, 1], dtype=np.int32)
    labels = np.array([0, 0, 1, 1, 2, 2, ka, ka + 1], dtype=np.uint32)
    nbrs = [na] * 400  # the node of type-b block 0: x = (m[r][0] + alpha) / (m_r[r] + 2 alpha) ~ 1e-3
    plain = np.prod([(m[:ka, ka] + 0.5) / (m_r[:ka] + 0.5 * kb)] * 400, axis=0)
    assert (plain == 0.0).all()
    P = D.numpy_foldin_posterior(labels, m, m_r, n_r, ka, 0, nbrs, 0.5)
    assert np.isfinite(P).all() and abs(P.sum() - 1.0) <= 4 * EPS and P.max() > 0.99
    # the block whose factor is largest wins: x_1 = 2.5 / 1001 against x_0 = 1.5 / 1001 and x_2 = 3.5 / 3001
    assert P.argmax() == 1


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "bisbm.h")).read()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(bisbm_handle h" % name, header, re.M), name
        assert name in B.ABI
    assert "#define BISBM_FOLDIN_RECOMMEND 1u" in header and "#define BISBM_FOLDIN_SIMILAR 2u" in header
    assert (B.FOLDIN_RECOMMEND, B.FOLDIN_SIMILAR) == (1, 2)
    lib = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "libbisbm_hip.so")
    if not os.path.exists(lib):
        B.build(force=True)
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert re.search(r" T %s$" % name, exported, re.M), name
    for method in ("foldin_set", "foldin_accumulate", "foldin_reset", "foldin_posteriors", "foldin_scores", "foldin_topk", "foldin_recommend",
                   "foldin_similar"):
        assert callable(getattr(B.BlockModel, method))
    assert "bisbm_abi_version" in B.ABI and "#define BISBM_ABI_VERSION 3" in header


def test_python_states_the_kernel_constants():
    text = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "csrc", "bisbm_kernels.hpp")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (kFoldin\w+) = (\d+);", text)}
    assert (const["kFoldinCandTile"], const["kFoldinTile"]) == (B.FOLDIN_CAND_TILE, B.FOLDIN_TILE)


def test_cli_refusals_that_need_no_device(tmp_path):
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    if not os.path.exists(cli):
        B.build(force=True)
    el = os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist")
    q, out = tmp_path / "nodes.txt", tmp_path / "out.txt"
    q.write_text("a 20 21 20\nb 3\n")

    def run(*args):
        r = subprocess.run([cli, "-e", el, "-y", "18", "14", *args], capture_output=True, text=True)
        return r.returncode, r.stdout, r.stderr
    assert run("--foldin", str(q), str(out), "3", "--foldin_alpha", "0.1") == (
        1, "", "--foldin folds nodes that are not in the graph into the samples of the chains: it needs --marginalize.\n")
    for k in ("0", "-2", "x3", "2.5"):
        rc, so, err = run("--marginalize", "--foldin", str(q), str(out), k, "--foldin_alpha", "0.1")
        assert (rc, so) == (1, "") and err.startswith("Invalid --foldin. K must be a positive integer"), (k, err)
    rc, so, err = run("--marginalize", "--foldin", str(q), str(out), str(B.QUERY_MAX_K + 1), "--foldin_alpha", "0.1")
    assert (rc, so) == (1, "") and err.startswith("Invalid --foldin. K is at most %d" % B.QUERY_MAX_K), err
    for args in ((str(q), str(out)), (str(q),), (str(q), str(out), "3", "4")):
        rc, so, err = run("--marginalize", "--foldin", *args, "--foldin_alpha", "0.1")
        assert (rc, so) == (1, "") and err.startswith("Invalid --foldin. Three arguments"), (args, err)
    rc, so, err = run("--marginalize", "--foldin", str(q), str(out), "3")  # no --foldin_alpha
    assert (rc, so) == (1, "") and err.startswith("--foldin needs --foldin_alpha"), err
    for a in ("0", "-1", "nan", "inf", "x", "1e"):
        rc, so, err = run("--marginalize", "--foldin", str(q), str(out), "3", "--foldin_alpha=" + a)
        assert (rc, so) == (1, "") and err.startswith("Invalid --foldin_alpha."), (a, err)
    rc, so, err = run("--marginalize", "--foldin_alpha", "0.1")
    assert (rc, so) == (1, "") and "it needs --foldin" in err
    ok = ("--marginalize", "--foldin", str(q), str(out), "3", "--foldin_alpha", "0.1")
    missing = str(tmp_path / "missing.txt")
    assert run("--marginalize", "--foldin", missing, str(out), "3", "--foldin_alpha", "0.1") == (1, "", "[error] --foldin: cannot read %s\n" % missing)
    for text, line, what in (("a 20\n\nc 3\n", 3, "must begin with the node's type"),      # a malformed line
                             ("a 20\nb\n", 2, "names no neighbour"),
                             ("a 20 2x\n", 1, "2x is not a node id"),
                             ("a 20 3\n", 1, "3 is not"),                                   # a type-a node among a type-a node's neighbours
                             ("b 3\nb 3 18\n", 2, "18 is not"),
                             ("a 32\n", 1, "32 is not")):
        q.write_text(text)
        rc, so, err = run(*ok)
        assert (rc, so) == (1, "") and err.startswith("[error] --foldin: line %d of %s" % (line, q)) and what in err, (text, err)
    assert not out.exists()
    help_text = subprocess.run([cli, "--help"], capture_output=True, text=True).stderr
    assert "--foldin QUERIES OUT K" in help_text and "--foldin_alpha A" in help_text
