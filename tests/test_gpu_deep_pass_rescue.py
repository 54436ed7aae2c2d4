"""The column test of the four- and eight-steps passes on the GPU (-m gpu).

step_quad32, step_quad and step_oct keep a later step whose inverse-CDF target lies strictly between an earlier mover's r and s
when (D - 1) k fits the target's margin (column_clash, csrc/bisbm_stand_rule.hpp; the rule itself is checked on the CPU by
test_stand_rule.py, and test_gpu_target_rescue.py pins every depth to the oracle on small column sums).  Here:
  * the diagnostic build (BISBM_PASS_COUNTS) shows that on those small-column-sum graphs the deep passes both keep and refuse
    column candidates, at the boundary (D - 1) k == margin and (D - 1) k == margin + 1 too;
  * the chains of a pinned deep pass equal those of two steps per pass and of one step per pass to the bit -- state, rates, counts
    and the running sum kept step by step -- on graphs where several movers precede a step of a pass: one 32 + 32 graph of
    48 000 nodes (step_quad32), one 16 + 13 (step_quad), one 8 + 7 (step_oct at depth 8, step_quad at depth 4)."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_gpu_target_rescue import _COUNTS_RUN, ENV, SHAPES

pytestmark = pytest.mark.gpu

B = importlib.import_module("bipartitesbm-mcmc_amd")
SYN = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 60

DEEP = [s for s in SHAPES if s[0] in ("quad32", "quad", "oct")]
BOUNDARY = ("quad32", "quad")  # (depth 8 asks for 7 k <= margin: a boundary case needs a column entry >= 8 at the target)


def test_diagnostic_build_sees_the_deep_passes_keep_and_refuse(tmp_path):
    """Over the pairs of a deep pass whose earlier step is a committed mover: shared blocks, column candidates kept and refused on
    every shape, both boundary cases at depth 4."""
    assert [s[0] for s in DEEP] == ["quad32", "quad", "oct"]
    build = importlib.util.spec_from_file_location("_bisbm_build", os.path.join(ROOT, "bipartitesbm-mcmc_amd", "build.py"))
    mod = importlib.util.module_from_spec(build)
    build.loader.exec_module(mod)
    lib = str(tmp_path / "libbisbm_counts.so")
    mod.compile_library(lib, ["-DBISBM_PASS_COUNTS=1"], jobs=8)
    env = {k: v for k, v in os.environ.items() if k not in ENV}
    for sid, na, nb, ne, ka, kb, depth, pass_steps, seed in DEEP:
        e = dict(env)
        e["BISBM_PASS_DEPTH"] = depth
        r = subprocess.run([sys.executable, "-c", _COUNTS_RUN, ROOT, lib] + [str(v) for v in (na, nb, ne, ka, kb, seed)],
                           capture_output=True, text=True, env=e, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "pass_steps %d" % pass_steps in r.stdout, r.stdout
        lines = [l for l in r.stderr.splitlines() if l.startswith("[pass_counts]")]
        assert lines, r.stderr[-3000:]
        tot = {}
        for l in lines:
            for name, v in re.findall(r"([a-z_]+) (\d+)", l):
                tot[name] = tot.get(name, 0) + int(v)
        print(sid, tot)
        assert tot["passes"] > 0 and tot["passes"] < tot["steps"] <= pass_steps * tot["passes"], (sid, tot)
        assert tot["deep_shared_block"] > 0, (sid, tot)
        assert tot["deep_kept"] > 0 and tot["deep_refused"] > 0, (sid, tot)
        assert tot["deep_kept_at_boundary"] <= tot["deep_kept"] and tot["deep_refused_at_boundary"] <= tot["deep_refused"], (sid, tot)
        if sid in BOUNDARY:
            assert tot["deep_kept_at_boundary"] > 0 and tot["deep_refused_at_boundary"] > 0, (sid, tot)


# id, na, nb, edges, Ka, Kb, graph seed, the pinned depths to compare (the last two references: two steps per pass, one step per pass)
GRAPHS = [("k32", 24000, 24000, 240000, 32, 32, 21, ("4",)),
          ("k16", 1600, 1300, 16000, 16, 13, 22, ("4",)),
          ("k8", 800, 700, 8000, 8, 7, 23, ("8", "4"))]
CHAINS = 4
SWEEPS = 3
SEED = 99


def _run(monkeypatch, graph, labels, na, nb, ka, kb, env, keep):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("BISBM_KEEP_SUM", keep)
    g = B.BlockModel(labels, SYN.types_vector(na, nb), ka + kb, ka, kb, 1.0, graph, n_chains=CHAINS, rng="philox", seed=SEED)
    g.shuffle_bisbm()
    rates = np.atleast_1d(B.MetropolisHasting().anneal(g, "constant", [1.0], SWEEPS * (na + nb), BIG)).copy()
    acc, sw = g.last_counts()
    out = dict(pass_steps=g.last_pass_steps(), rates=rates, acc=acc.copy(), sweeps=sw.copy(), cum=g.get_entropy().copy(),
               state=[(g.get_memberships(c), g.get_m(c), g.get_m_r(c), g.get_n_r(c), g.get_eta_rk_(c)) for c in range(CHAINS)])
    for k in list(env) + ["BISBM_KEEP_SUM"]:
        monkeypatch.delenv(k, raising=False)
    return out


@pytest.mark.parametrize("graph", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_deep_passes_equal_shallow_ones_to_the_bit(graph, monkeypatch):
    gid, na, nb, ne, ka, kb, seed, depths = graph
    csr = cases.random_graph(seed, na, nb, ne, ka, kb)
    labels = O.contiguous_labels(na, nb, ka, kb)
    for keep in ("0", "1"):
        refs = [(_run(monkeypatch, csr, labels, na, nb, ka, kb, {"BISBM_PASS_DEPTH": "2"}, keep), 2),
                (_run(monkeypatch, csr, labels, na, nb, ka, kb, {"BISBM_SINGLE_STEPS": "1"}, keep), 1)]
        for ref, steps in refs:
            assert ref["pass_steps"] == steps, (gid, keep, steps, ref["pass_steps"])
        assert (refs[0][0]["acc"] > 0).all() and (refs[0][0]["sweeps"] == SWEEPS).all(), gid
        for depth in depths:
            got = _run(monkeypatch, csr, labels, na, nb, ka, kb, {"BISBM_PASS_DEPTH": depth}, keep)
            assert got["pass_steps"] == int(depth), (gid, keep, depth, got["pass_steps"])
            for ref, steps in refs:
                what = (gid, keep, depth, steps)
                assert (got["rates"] == ref["rates"]).all(), what
                assert (got["acc"] == ref["acc"]).all() and (got["sweeps"] == ref["sweeps"]).all(), what
                for c in range(CHAINS):
                    for a, b in zip(got["state"][c], ref["state"][c]):
                        assert (np.asarray(a) == np.asarray(b)).all(), what + (c,)
                if keep == "1":  # the running sum kept step by step: the same additions in the same order
                    assert (got["cum"].view(np.uint64) == ref["cum"].view(np.uint64)).all(), what
