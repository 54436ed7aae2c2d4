"""CPU checks of the query scores (include/bisbm.h, "Query scores"): the host statement of the ranking
(distributed.numpy_query_topk, the reference of the GPU tests), the refusals of `mcmc --recommend` that need no device, and the
tile constants the Python side states against the kernel header's."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
NONE = 0xFFFFFFFF


def test_ranking_ties_go_to_the_lowest_index():
    row = np.array([1.0, 3.0, 3.0, 0.0, 2.0, 3.0, 0.0])
    idx, val = D.numpy_query_topk(row, 4)
    assert idx.dtype == np.uint32 and val.dtype == np.float64
    assert idx.tolist() == [1, 2, 5, 4] and val.tolist() == [3.0, 3.0, 3.0, 2.0]
    # the k-th and the (k + 1)-th are equal: the lower index is in, the higher is out
    idx, val = D.numpy_query_topk(row, 2)
    assert idx.tolist() == [1, 2] and val.tolist() == [3.0, 3.0]
    # candidates of sum 0.0 are eligible and rank last, by index
    idx, val = D.numpy_query_topk(row, 7)
    assert idx.tolist() == [1, 2, 5, 4, 0, 3, 6] and val.tolist() == [3.0, 3.0, 3.0, 2.0, 1.0, 0.0, 0.0]


def test_ranking_exclusion_and_fewer_eligible_than_k():
    row = np.array([1.0, 3.0, 3.0, 0.0, 2.0, 3.0, 0.0])
    idx, val = D.numpy_query_topk(row, 3, excluded=[2, 1, 1])  # (a neighbour by two edges is listed twice)
    assert idx.tolist() == [5, 4, 0] and val.tolist() == [3.0, 2.0, 1.0]
    idx, val = D.numpy_query_topk(row, 4, excluded=[0, 1, 2, 4, 5])
    assert idx.tolist() == [3, 6, NONE, NONE] and val.tolist() == [0.0, 0.0, 0.0, 0.0]
    idx, val = D.numpy_query_topk(row, 2, excluded=np.arange(7))
    assert idx.tolist() == [NONE, NONE] and (val == 0).all()
    idx, val = D.numpy_query_topk(np.zeros(0), 2)
    assert idx.tolist() == [NONE, NONE]
    assert B.QUERY_NONE == D.QUERY_NONE == NONE


def test_python_states_the_kernel_constants():
    text = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "csrc", "bisbm_kernels.hpp")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (kQuery\w+) = (\d+);", text)}
    assert (const["kQueryCandTile"], const["kQueryTile"], const["kQueryMaxK"]) == (B.QUERY_CAND_TILE, B.QUERY_TILE, B.QUERY_MAX_K)
    header = open(os.path.join(ROOT, "include", "bisbm.h")).read()
    assert "every k <= %d is served" % B.QUERY_MAX_K in header


def test_cli_refusals_that_need_no_device(tmp_path):
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    if not os.path.exists(cli):
        B.build(force=True)
    el = os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist")
    q, out = tmp_path / "queries.txt", tmp_path / "out.txt"
    q.write_text("3\n20\n")

    def run(*args):
        r = subprocess.run([cli, "-e", el, "-y", "18", "14", *args], capture_output=True, text=True)
        return r.returncode, r.stdout, r.stderr
    assert run("--recommend", str(q), str(out), "3") == (
        1, "", "--recommend ranks the candidates of nodes over the samples of the chains: it needs --marginalize.\n")
    for k in ("0", "-2", "x3", "2.5", ""):
        rc, so, err = run("--marginalize", "--recommend", str(q), str(out), k)
        assert (rc, so) == (1, "") and err.startswith("Invalid --recommend. K must be a positive integer"), (k, err)
    rc, so, err = run("--marginalize", "--recommend", str(q), str(out))
    assert (rc, so) == (1, "") and err.startswith("Invalid --recommend. Three arguments")
    missing = str(tmp_path / "missing.txt")
    assert run("--marginalize", "--recommend", missing, str(out), "3") == (1, "", "[error] --recommend: cannot read %s\n" % missing)
    q.write_text("3\n\n20\n32\n5\n")
    assert run("--marginalize", "--recommend", str(q), str(out), "3") == (
        1, "", "[error] --recommend: line 4 of %s (32) must name a node [0, 32)\n" % q)
    q.write_text("3\n7 9\n")
    rc, so, err = run("--marginalize", "--recommend", str(q), str(out), "3")
    assert (rc, so) == (1, "") and "line 2 of" in err
    assert run("--marginalize", "--include_edges")[2] == "--include_edges keeps a query's neighbours among its candidates: it needs --recommend.\n"
    assert not out.exists()
    help_text = subprocess.run([cli, "--help"], capture_output=True, text=True).stderr
    assert "--recommend QUERIES OUT K" in help_text and "--include_edges" in help_text
