"""CPU checks of the edge queries (include/bisbm.h, "Edge queries"): the vectorised host statement of one chain's rows
(distributed.numpy_edge_query_rows, the model of the GPU tests on larger shapes) against a loop of numpy_edge_dS -- which
tests/test_edge_probs.py pins to the checker library's description length --, and the surface: header, ctypes table, tile
constants, marginalize(recommend_edges=...), the refusals of `mcmc --recommend_edges` that need no device."""
import importlib
import math
import os
import re
import subprocess

import numpy as np

import oracle_lib as O
from test_edge_probs import KA, KB, NA, NB, small_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed


def LG(i):
    return math.lgamma(i) if i else math.inf


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def test_rows_equal_a_loop_of_the_listed_model_bit_for_bit():
    a, b, labels = small_graph()
    n = NA + NB
    rowptr, col = O.edge_to_csr(a, b, n)
    deg = np.diff(rowptr.astype(np.int64))
    o = O.OracleModel(rowptr, col, NA, NB, KA, KB, 1.0, labels)
    o.init_bisbm()
    m, m_r, n_r, eta = o.m(), o.m_r(), o.n_r(), o.eta()
    logq = O.lib().orc_log_q
    queries = np.arange(n)
    mult = D.numpy_edge_query_mult(rowptr, col, NA, queries)
    rows = D.numpy_edge_query_rows(m, m_r, n_r, eta, deg, labels, NA, KA, KB, len(a), queries, mult, LG, logq)
    assert len(rows) == n
    seen = set()
    for q, row, mu_row in zip(queries.tolist(), rows, mult):
        cands = range(NA, n) if q < NA else range(NA)
        pairs = np.array([(q, c) if q < NA else (c, q) for c in cands])
        mu = D.numpy_edge_multiplicity(rowptr, col, pairs)
        assert mu_row.dtype == np.uint32 and (mu_row == mu).all()
        want = [D.numpy_edge_dS(m, m_r, n_r, eta, deg, labels, KA, KB, len(a), u, v, 0, k, LG, logq) for (u, v), k in zip(pairs.tolist(), mu.tolist())]
        assert row.dtype == np.float64 and (bits(row) == bits(want)).all(), (q, row, want)
        assert np.isfinite(row).all()
        seen |= set(mu.tolist())
    assert seen == {0, 1, 2}  # (absent edges, single edges, the four doubled ones)
    assert deg[14] == 0 and deg[26] == 0 and m_r[2] == 0 and m_r[4] == 0  # the isolated nodes, alone in their blocks
    assert int(deg.max()) + 1 == np.asarray(eta).shape[1]  # d + 1 of the largest degree lies beyond the eta table
    # a type-b query's row is the column of the type-a queries' rows: the same pairs
    for v in (NA, n - 1):
        assert (bits(rows[v]) == bits([rows[u][v - NA] for u in range(NA)])).all()


def test_the_multiplicity_term_of_an_absent_edge_is_plus_zero():
    """lg(1) = lg(2) = 0.0 exactly, so t_mult = lg(mu + 2) - lg(mu + 1) is +0.0 at mu = 0: a cell that is no present edge may
    skip the add.  The C library's lgamma, whose values the engine's table holds."""
    for lg in (O.lib().orc_lgamma_fast, math.lgamma):
        one, two = float(lg(1)), float(lg(2))
        assert one == 0.0 and two == 0.0
        assert bits(two - one) == bits(0.0)
        assert float(lg(3)) - two > 0.0


def test_header_ctypes_table_and_tile_constants_agree():
    text = open(os.path.join(ROOT, "include", "bisbm.h")).read()
    assert re.search(r"#define\s+BISBM_ABI_VERSION\s+3\b", text)  # (additions only)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    n_args = {"set": 3, "accumulate": 1, "reset": 1, "get_row": 5, "topk": 6}
    for name, count in n_args.items():
        decl = re.search(r"\bint\s+bisbm_edge_queries_%s\s*\(([^)]*)\)" % name, code)
        assert decl, name
        assert len(decl.group(1).split(",")) == count, name
        assert len(B.ABI["bisbm_edge_queries_" + name][1]) == count, name
    kernels = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "csrc", "bisbm_kernels.hpp")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (kEdgeQuery\w+) = (\d+);", kernels)}
    assert (const["kEdgeQueryCandTile"], const["kEdgeQueryTile"]) == (B.EDGE_QUERY_CAND_TILE, B.EDGE_QUERY_TILE)
    assert B.EDGE_QUERY_TILE * 4 <= 32  # one flag bit per cell of a lane
    build = importlib.import_module("bipartitesbm-mcmc_amd.build")
    assert "bisbm_edge_queries.hip" in build.SOURCES
    for method in ("edge_queries_set", "edge_queries_accumulate", "edge_queries_reset", "edge_queries", "edge_queries_topk", "recommend_edges"):
        assert callable(getattr(B.BlockModel, method)), method


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
            if name in ("recommend", "recommend_edges"):
                return name
        return call


def test_marginalize_sets_resets_samples_and_returns_the_edge_recommendations():
    queries = np.array([0, 4])
    m = _StubModel()
    out = B.marginalize(m, 5, 2, 3, recommend=(queries, 3), recommend_edges=(queries, 2, False))
    names = [c[0] for c in m.calls]
    assert names == ["run_sweeps", "query_scores_set", "query_scores_reset", "edge_queries_set", "edge_queries_reset", "marginals_reset",
                     "run_sweeps", "marginals_accumulate", "query_scores_accumulate", "edge_queries_accumulate",
                     "run_sweeps", "marginals_accumulate", "query_scores_accumulate", "edge_queries_accumulate", "marginals_get",
                     "recommend", "recommend_edges"], names
    assert m.calls[names.index("edge_queries_set")][1] is queries
    assert m.calls[-1] == ("recommend_edges", 2, False)
    assert len(out) == 4 and out[2:] == ("recommend", "recommend_edges")
    m = _StubModel()
    out = B.marginalize(m, 0, 1, 0, recommend_edges=(queries, 7))
    assert m.calls[-1] == ("recommend_edges", 7, True) and len(out) == 3 and out[2] == "recommend_edges"
    assert [c[0] for c in m.calls].count("edge_queries_accumulate") == 1
    m = _StubModel()
    B.marginalize(m, 0, 2, 0)
    assert not any(c[0].startswith("edge_queries") or c[0] == "recommend_edges" for c in m.calls)


def test_cli_refusals_need_no_device(tmp_path):
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    if not os.path.exists(cli):
        B.build(force=True)
    el = os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist")
    q, out = tmp_path / "queries.txt", tmp_path / "out.txt"
    q.write_text("3\n20\n")

    def run(*args):
        r = subprocess.run([cli, "-e", el, "-y", "18", "14", *args], capture_output=True, text=True)
        return r.returncode, r.stdout, r.stderr
    assert run("--recommend_edges", str(q), str(out), "3") == (
        1, "", "--recommend_edges ranks the candidates of nodes over the samples of the chains: it needs --marginalize.\n")
    for k in ("0", "-2", "x3", "2.5", ""):
        rc, so, err = run("--marginalize", "--recommend_edges", str(q), str(out), k)
        assert (rc, so) == (1, "") and err.startswith("Invalid --recommend_edges. K must be a positive integer"), (k, err)
    rc, so, err = run("--marginalize", "--recommend_edges", str(q), str(out))
    assert (rc, so) == (1, "") and err.startswith("Invalid --recommend_edges. Three arguments")
    missing = str(tmp_path / "missing.txt")
    assert run("--marginalize", "--recommend_edges", missing, str(out), "3") == (1, "", "[error] --recommend_edges: cannot read %s\n" % missing)
    q.write_text("3\n\n20\n32\n5\n")
    assert run("--marginalize", "--recommend_edges", str(q), str(out), "3") == (
        1, "", "[error] --recommend_edges: line 4 of %s (32) must name a node [0, 32)\n" % q)
    q.write_text("3\n7 9\n")
    rc, so, err = run("--marginalize", "--recommend_edges", str(q), str(out), "3")
    assert (rc, so) == (1, "") and "line 2 of" in err
    # --include_edges goes with either ranking; alone it is refused as before
    assert run("--marginalize", "--include_edges")[2] == "--include_edges keeps a query's neighbours among its candidates: it needs --recommend.\n"
    q.write_text("3\n32\n")
    rc, so, err = run("--marginalize", "--include_edges", "--recommend_edges", str(q), str(out), "3")
    assert (rc, so) == (1, "") and "line 2 of" in err  # (accepted next to --recommend_edges: the next check speaks)
    assert not out.exists()
    help_text = subprocess.run([cli, "--help"], capture_output=True, text=True).stderr
    assert "--recommend_edges QUERIES OUT K" in help_text and "log_prob" in help_text
