"""CPU checks of the edge probabilities (include/bisbm.h, "Edge probabilities"): the host statement of one chain's dS
(distributed.numpy_edge_dS, the model of the GPU tests) against the description length of the checker library on the edited
graph, and the surface: header, ctypes table, marginalize(edge_probs=...), the refusals of `mcmc --edge_probs` that need no
device."""
import importlib
import math
import os
import re
import subprocess

import numpy as np

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed

NA, NB, KA, KB = 15, 12, 3, 2


def small_graph(seed=3):
    """(a, b, labels): 15 + 12 nodes, 3 + 2 blocks, 60 edges of which four repeat an earlier one.  Node 14 (type a) and node 26
    (type b) have no edge and sit alone in blocks 2 and 4: d = 0 and m_r = 0.  Every block is non-empty, the other labels are
    random."""
    rs = np.random.default_rng(seed)
    cells = rs.choice((NA - 1) * (NB - 1), 56, replace=False)
    a, b = cells // (NB - 1), NA + cells % (NB - 1)
    dup = rs.choice(56, 4, replace=False)
    a, b = np.concatenate([a, a[dup]]), np.concatenate([b, b[dup]])
    order = rs.permutation(60)
    la = rs.integers(0, 2, NA - 1)
    la[:2] = (0, 1)
    labels = np.concatenate([la, [2], np.full(NB - 1, 3), [4]]).astype(np.uint32)
    return a[order].astype(np.int64), b[order].astype(np.int64), labels


def all_edits(a, b):
    """(pairs [P, 2], kinds [P]): all 180 ADD pairs, then every distinct edge as REMOVE"""
    u, v = np.meshgrid(np.arange(NA), NA + np.arange(NB), indexing="ij")
    add = np.stack([u.ravel(), v.ravel()], axis=1)
    rem = np.unique(np.stack([a, b], axis=1), axis=0)
    return np.concatenate([add, rem]), np.concatenate([np.zeros(len(add), dtype=np.uint8), np.ones(len(rem), dtype=np.uint8)])


def edited(a, b, u, v, kind):
    """the edge list with one edge u - v more (kind 0) or less (kind 1)"""
    if kind == 0:
        return np.concatenate([a, [u]]), np.concatenate([b, [v]])
    i = int(np.flatnonzero((a == u) & (b == v))[0])
    return np.delete(a, i), np.delete(b, i)


def tolerance(n, ka, kb, max_degree, S0, S1):
    """The summand count of orc_entropy times half an ulp, for both entropies"""
    K = ka + kb
    return 2 * (n + ka * kb + K * (max_degree + 2) + 2 * K + 16) * 2.0 ** -53 * max(abs(S0), abs(S1))


def test_model_equals_the_oracles_entropy_difference():
    a, b, labels = small_graph()
    n = NA + NB
    rowptr, col = O.edge_to_csr(a, b, n)
    deg = np.diff(rowptr.astype(np.int64))
    assert len(a) == 60 and len(np.unique(np.stack([a, b], axis=1), axis=0)) == 56
    assert deg[14] == 0 and deg[26] == 0 and len(set(labels.tolist())) == KA + KB
    o = O.OracleModel(rowptr, col, NA, NB, KA, KB, 1.0, labels)
    o.init_bisbm()
    S0 = o.entropy()
    m, m_r, n_r, eta = o.m(), o.m_r(), o.n_r(), o.eta()
    assert m_r[2] == 0 and m_r[4] == 0
    pairs, kinds = all_edits(a, b)
    assert (kinds == 0).sum() == 180 and (kinds == 1).sum() == 56
    mult = D.numpy_edge_multiplicity(rowptr, col, pairs)
    assert sorted(set(mult.tolist())) == [0, 1, 2] and (mult[kinds == 1] >= 1).all()
    logq = O.lib().orc_log_q
    worst = 0.0
    for (u, v), kind, mu in zip(pairs.tolist(), kinds.tolist(), mult.tolist()):
        dS = D.numpy_edge_dS(m, m_r, n_r, eta, deg, labels, KA, KB, len(a), u, v, kind, mu, lambda i: math.lgamma(i) if i else math.inf, logq)
        a1, b1 = edited(a, b, u, v, kind)
        rp1, cl1 = O.edge_to_csr(a1, b1, n)
        o1 = O.OracleModel(rp1, cl1, NA, NB, KA, KB, 1.0, labels)
        o1.init_bisbm()
        S1 = o1.entropy()
        err = abs(dS - (S1 - S0))
        worst = max(worst, err)
        assert err <= tolerance(n, KA, KB, o.maxdeg, S0, S1), (u, v, kind, mu, dS, S1 - S0)
    print("worst |dS - (S1 - S0)| = %.3g at S0 = %.6g" % (worst, S0))


def test_header_and_ctypes_table_declare_the_calls():
    text = open(os.path.join(ROOT, "include", "bisbm.h")).read()
    assert re.search(r"#define\s+BISBM_ABI_VERSION\s+3\b", text)  # (additions only)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("set", "accumulate", "reset", "get", "get_last"):
        assert re.search(r"\bint\s+bisbm_edge_probs_%s\s*\(" % name, code), name
        assert "bisbm_edge_probs_" + name in B.ABI
    for name, value in (("BISBM_EDGE_ADD", 0), ("BISBM_EDGE_REMOVE", 1), ("BISBM_EDGE_KEEP_LAST", 1)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, value), code), name
    assert (B.EDGE_ADD, B.EDGE_REMOVE, B.EDGE_KEEP_LAST) == (0, 1, 1)
    assert len(B.ABI["bisbm_edge_probs_set"][1]) == 6 and len(B.ABI["bisbm_edge_probs_get"][1]) == 5
    engine = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "csrc", "bisbm_engine.hpp")).read()
    assert re.search(r"kEdgeProbsTile\s*=\s*%d\b" % B.EDGE_PROBS_TILE, engine)


class _StubModel:
    """What marginalize() asks of a model on one rank, every call written down"""
    n, na, KA, kmax = 6, 3, 2, 2

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args, **kw):
            self.calls.append((name,) + args)
            if name == "marginals_get":
                return np.zeros((self.n, self.kmax), dtype=np.uint32)
        return call


def test_marginalize_sets_resets_and_samples_the_edge_probs():
    pairs, kinds = np.array([[0, 3], [1, 4]]), [0, 1]
    m = _StubModel()
    B.marginalize(m, 5, 2, 3, edge_probs=(pairs, kinds), score_pairs=pairs)
    names = [c[0] for c in m.calls]
    assert names == ["run_sweeps", "pair_scores_set", "pair_scores_reset", "edge_probs_set", "edge_probs_reset", "marginals_reset",
                     "run_sweeps", "marginals_accumulate", "pair_scores_accumulate", "edge_probs_accumulate",
                     "run_sweeps", "marginals_accumulate", "pair_scores_accumulate", "edge_probs_accumulate", "marginals_get"], names
    call = m.calls[names.index("edge_probs_set")]
    assert call[1] is pairs and call[2] is kinds
    m = _StubModel()
    B.marginalize(m, 0, 1, 0, edge_probs=(pairs,))  # all ADD
    call = [c for c in m.calls if c[0] == "edge_probs_set"][0]
    assert call[1] is pairs and call[2] is None
    assert [c[0] for c in m.calls].count("edge_probs_accumulate") == 1
    m = _StubModel()
    B.marginalize(m, 0, 2, 0)
    assert not any(c[0].startswith("edge_probs") for c in m.calls)


def test_cli_refusals_need_no_device(tmp_path):
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    if not os.path.exists(cli):
        B.build(force=True)
    el = os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist")
    a, b = O.load_edge_list(el)
    u0, v0 = int(min(a[0], b[0])), int(max(a[0], b[0]))  # an edge of the graph
    edges = set(zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist()))
    non = next((u, v) for u in range(18) for v in range(18, 32) if (u, v) not in edges)
    good, out = tmp_path / "pairs.txt", tmp_path / "probs.txt"
    good.write_text("0 18\n%d %d -\n17 31 +\n" % (u0, v0))

    def run(*args):
        r = subprocess.run([cli, *args], capture_output=True, text=True)
        return r.returncode, r.stdout, r.stderr
    base = ("-e", el, "-y", "18", "14", "-n", "9", "9", "7", "7", "-z", "2", "2")
    rc, so, se = run(*base, "--edge_probs", str(good), str(out))
    assert rc == 1 and so == "" and "--marginalize" in se
    rc, so, se = run(*base, "--marginalize", "--edge_probs", str(good))
    assert rc == 1 and so == "" and "Two paths" in se
    rc, so, se = run(*base, "--marginalize", "--edge_probs", str(tmp_path / "missing"), str(out))
    assert rc == 1 and so == "" and "cannot read" in se
    bad = tmp_path / "bad.txt"
    for text, line in (("0 18\n3\n", 2), ("0 18 *\n", 1), ("0 18 + 4\n", 1), ("0 x\n", 1), ("0 18\n1 19\n-2 20\n", 3), ("0 18 -+\n", 1)):
        bad.write_text(text)
        rc, so, se = run(*base, "--marginalize", "--edge_probs", str(bad), str(out))
        assert rc == 1 and so == "" and ("line %d " % line) in se, (text, se)
    for text, index in (("0 18\n3 5\n", 1), ("18 19 -\n", 0), ("0 32\n", 0)):
        bad.write_text(text)
        rc, so, se = run(*base, "--marginalize", "--edge_probs", str(bad), str(out))
        assert rc == 1 and so == "" and ("pair %d " % index) in se and "type-a" in se, (text, se)
    bad.write_text("%d %d -\n%d %d -\n" % (u0, v0, non[0], non[1]))  # a `-` on a non-edge
    rc, so, se = run(*base, "--marginalize", "--edge_probs", str(bad), str(out))
    assert rc == 1 and so == "" and "pair 1 " in se and "does not hold" in se, se
    assert not out.exists()
