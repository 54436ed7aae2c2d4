"""CPU checks of the co-assignment calls (include/bisbm.h, "Co-assignment"): the host statement of the counts
(distributed.numpy_coassign, the reference of the GPU tests) against a brute-force double loop, the five symbols declared,
exported and bound, the tile constants the Python side states against the kernel header's, and the refusals of
`mcmc --similar` that need no device."""
import importlib
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed

SYMBOLS = ["bisbm_coassign_set", "bisbm_coassign_accumulate", "bisbm_coassign_reset", "bisbm_coassign_get_row", "bisbm_coassign_topk"]


def test_numpy_model_is_the_double_loop():
    na, nb, vectors = 17, 13, 7
    rs = np.random.default_rng(3)
    labels = [np.concatenate([rs.integers(0, 3, na), 3 + rs.integers(0, 4, nb)]).astype(np.uint32) for _ in range(vectors)]
    queries = [0, na + 2, 16, na, 5, 29, 5]  # both types, a repeated one, the last node of each type
    rows = D.numpy_coassign(labels, queries, na)
    assert len(rows) == len(queries)
    for q, row in zip(queries, rows):
        first, n_own = (0, na) if q < na else (na, nb)
        want = [0] * n_own
        for lab in labels:
            for j in range(n_own):
                want[j] += int(lab[first + j] == lab[q])
        assert row.dtype == np.uint32 and row.tolist() == want
        assert row[q - first] == vectors
    assert (rows[4] == rows[6]).all()
    # symmetry between two queries of one type
    assert rows[0][16] == rows[2][0] and rows[0][5] == rows[4][0] and rows[1][0] == rows[3][2]
    # a row adds up to the sizes of the query's blocks
    for q, row in zip(queries, rows):
        assert int(row.sum()) == sum(int((lab == lab[q]).sum()) for lab in labels)
    assert D.numpy_coassign is B.numpy_coassign


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "bisbm.h")).read()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(bisbm_handle h" % name, header, re.M), name
        assert name in B.ABI
    lib = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "libbisbm_hip.so")
    if not os.path.exists(lib):
        B.build(force=True)
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert re.search(r" T %s$" % name, exported, re.M), name
    for method in ("coassign_set", "coassign_accumulate", "coassign_reset", "coassignment", "coassign_topk", "similar"):
        assert callable(getattr(B.BlockModel, method))
    assert "bisbm_abi_version" in B.ABI and "#define BISBM_ABI_VERSION 3" in header


def test_python_states_the_kernel_constants():
    text = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "csrc", "bisbm_kernels.hpp")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (kCoassign\w+) = (\d+);", text)}
    assert (const["kCoassignCandTile"], const["kCoassignTile"]) == (B.COASSIGN_CAND_TILE, B.COASSIGN_TILE)


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
    assert run("--similar", str(q), str(out), "3") == (
        1, "", "--similar counts the chains in which nodes share a block over the samples of the chains: it needs --marginalize.\n")
    for k in ("0", "-2", "x3", "2.5", ""):
        rc, so, err = run("--marginalize", "--similar", str(q), str(out), k)
        assert (rc, so) == (1, "") and err.startswith("Invalid --similar. K must be a positive integer"), (k, err)
    rc, so, err = run("--marginalize", "--similar", str(q), str(out), str(B.QUERY_MAX_K + 1))
    assert (rc, so) == (1, "") and err.startswith("Invalid --similar. K is at most %d" % B.QUERY_MAX_K), err
    for args in ((str(q), str(out)), (str(q),), (str(q), str(out), "3", "4")):
        rc, so, err = run("--marginalize", "--similar", *args)
        assert (rc, so) == (1, "") and err.startswith("Invalid --similar. Three arguments"), (args, err)
    missing = str(tmp_path / "missing.txt")
    assert run("--marginalize", "--similar", missing, str(out), "3") == (1, "", "[error] --similar: cannot read %s\n" % missing)
    q.write_text("3\n\n20\n32\n5\n")
    assert run("--marginalize", "--similar", str(q), str(out), "3") == (
        1, "", "[error] --similar: line 4 of %s (32) must name a node [0, 32)\n" % q)
    assert not out.exists()
    help_text = subprocess.run([cli, "--help"], capture_output=True, text=True).stderr
    assert "--similar QUERIES OUT K" in help_text and "--recommend QUERIES OUT K" in help_text
