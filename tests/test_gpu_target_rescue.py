"""The exact target test of the multi-step passes against the oracle (-m gpu).

A two-steps pass evaluates step q + 1 against the state before step q.  When step q moves its node r -> s and step q + 1's
inverse-CDF target s' lies strictly between r and s, the running sums of s' and s' - 1 over column t' move by k = k_q[t'].
step_pair and step_pair64 keep step q + 1 when s' is still the first block whose sum exceeds x (k <= margin, target_margin in
bisbm_sweep_fast.hip) and evaluate it again otherwise.  Graphs with a few nodes per block make the column sums small, so
the target often does move: a margin off by one, or the wrong side of the scan, changes a chain, which the oracle sees.

Every pass depth runs pinned (BISBM_PASS_DEPTH), under a constant schedule, a cooling one and a cooling one with the early stop
in reach, with the running sum from the description length and step by step (BISBM_KEEP_SUM).  After each call rates, counts,
labels, m, m_r, n_r, eta and the running sum equal the oracle's.  A diagnostic build (BISBM_PASS_COUNTS) shows that the
same workloads take both branches of the test, at the boundary k == margin and k == margin + 1 too.  The bench regime itself
(BASELINE configs[2], chains 0, 517 and 1023 over two sweeps from the randomised start) is test_gpu_parity.py's
test_full_size_properties."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cases
import oracle_lib as O

pytestmark = pytest.mark.gpu

B = importlib.import_module("bipartitesbm-mcmc_amd")
SYN = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")
BIG = 1 << 60
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("BISBM_PASS_DEPTH", "BISBM_SINGLE_STEPS", "BISBM_FORCE_GENERIC", "BISBM_KEEP_SUM", "BISBM_LAUNCH_STEPS",
       "BISBM_FIXED_ROLES", "BISBM_ETA_WINDOW")

# id, na, nb, edges, Ka, Kb, BISBM_PASS_DEPTH, steps per pass the launch must report, graph seed: a handful of nodes per block
SHAPES = [("pair", 300, 260, 5000, 24, 20, "2", 2, 11),
          ("pair32", 200, 200, 4000, 32, 32, "2", 2, 12),
          ("pair64", 420, 380, 7000, 40, 36, None, 2, 13),
          ("quad32", 300, 260, 5000, 24, 20, "4", 4, 11),
          ("quad", 200, 180, 3000, 16, 13, "4", 4, 14),
          ("oct", 120, 110, 2000, 8, 7, "8", 8, 15)]
CHAINS = 4
PICKS = (0, CHAINS - 1)
SEED = 4242


def _graph(shape):
    sid, na, nb, ne, ka, kb, depth, pass_steps, seed = shape
    rowptr, col = cases.random_graph(seed, na, nb, ne, ka, kb)
    return rowptr, col, O.contiguous_labels(na, nb, ka, kb)


def _calls(n):
    alpha = 0.5 ** (1.0 / n)
    return [("constant", [1.0], 3 * n, BIG), ("exponential", [1.5, alpha], 2 * n, BIG), ("exponential", [0.9, alpha], n, n // 2)]


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_pinned_depths_match_oracle_on_small_column_sums(shape, monkeypatch):
    sid, na, nb, ne, ka, kb, depth, pass_steps, _ = shape
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if depth is not None:
        monkeypatch.setenv("BISBM_PASS_DEPTH", depth)
    n = na + nb
    rowptr, col, labels = _graph(shape)
    calls = _calls(n)
    mh = B.MetropolisHasting()
    runs = {}
    for keep in ("0", "1"):
        monkeypatch.setenv("BISBM_KEEP_SUM", keep)
        g = B.BlockModel(labels, SYN.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rowptr, col), n_chains=CHAINS, rng="philox",
                         seed=SEED)
        g.shuffle_bisbm()
        snaps = []
        for s_, kw, dur, aw in calls:
            rates = np.atleast_1d(mh.anneal(g, s_, kw, dur, aw)).copy()
            assert g.last_pass_steps() == pass_steps, (sid, s_, g.last_pass_steps())
            acc, sw = g.last_counts()
            snaps.append(dict(rates=rates, acc=acc.copy(), sweeps=sw.copy(), cum=g.get_entropy().copy(),
                              state=[(g.get_memberships(c), g.get_m(c), g.get_m_r(c), g.get_n_r(c), g.get_eta_rk_(c))
                                     for c in PICKS]))
        runs[keep] = snaps
    monkeypatch.delenv("BISBM_KEEP_SUM")
    for i, c in enumerate(PICKS):
        o = O.OracleModel(rowptr, col, na, nb, ka, kb, 1.0, labels)
        o.seed_philox(SEED, c)
        o.shuffle_bisbm()
        for j, (s_, kw, dur, aw) in enumerate(calls):
            ro = o.anneal(s_, kw, dur, aw)
            want = (o.memberships(), o.m(), o.m_r(), o.n_r(), o.eta())
            for keep in ("0", "1"):
                snap = runs[keep][j]
                what = (sid, s_, j, c, keep)
                assert snap["rates"][c] == ro, what
                assert snap["acc"][c] == o.last_accepted and snap["sweeps"][c] == o.last_sweeps, what
                for got, exp in zip(snap["state"][i], want):
                    assert (got == exp).all(), what
            want_sum = o.get_entropy()
            assert abs(runs["1"][j]["cum"][c] - want_sum) <= 1e-9 * abs(want_sum), (sid, j, c)
            assert abs(runs["0"][j]["cum"][c] - want_sum) <= 1e-9 * abs(want_sum) + 1e-12 * abs(o.entropy()), (sid, j, c)


_COUNTS_RUN = r"""
import importlib, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
B = importlib.import_module("bipartitesbm-mcmc_amd")
B.LIB_PATH = sys.argv[2]
SYN = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")
import cases, oracle_lib as O
na, nb, ne, ka, kb, seed = (int(v) for v in sys.argv[3:9])
rowptr, col = cases.random_graph(seed, na, nb, ne, ka, kb)
g = B.BlockModel(O.contiguous_labels(na, nb, ka, kb), SYN.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rowptr, col),
                 n_chains=64, rng="philox", seed=7)
g.shuffle_bisbm()
B.MetropolisHasting().anneal(g, "constant", [1.0], 4 * (na + nb), 1 << 60)
print("pass_steps", g.last_pass_steps())
"""


def test_diagnostic_build_sees_both_branches_of_the_target_test(tmp_path):
    """The BISBM_PASS_COUNTS build counts, over the passes whose first step moves, the second steps with a target strictly
    between r and s that the exact test keeps and those it refuses; both occur on these graphs, also at the boundary."""
    build = importlib.util.spec_from_file_location("_bisbm_build", os.path.join(ROOT, "bipartitesbm-mcmc_amd", "build.py"))
    mod = importlib.util.module_from_spec(build)
    build.loader.exec_module(mod)
    lib = str(tmp_path / "libbisbm_counts.so")
    mod.compile_library(lib, ["-DBISBM_PASS_COUNTS=1"], jobs=8)
    env = {k: v for k, v in os.environ.items() if k not in ENV}
    for sid, na, nb, ne, ka, kb, depth, _, seed in (SHAPES[0], SHAPES[2]):
        e = dict(env)
        if depth is not None:
            e["BISBM_PASS_DEPTH"] = depth
        r = subprocess.run([sys.executable, "-c", _COUNTS_RUN, ROOT, lib] + [str(v) for v in (na, nb, ne, ka, kb, seed)],
                           capture_output=True, text=True, env=e, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "pass_steps 2" in r.stdout, r.stdout
        lines = [l for l in r.stderr.splitlines() if l.startswith("[pass_counts]")]
        assert lines, r.stderr[-3000:]
        tot = {}
        for l in lines:
            for name, v in re.findall(r"([a-z_]+) (\d+)", l):
                tot[name] = tot.get(name, 0) + int(v)
        print(sid, tot)
        assert tot["passes"] > 0 and tot["passes"] < tot["steps"] <= 2 * tot["passes"], (sid, tot)
        assert tot["first_moves"] > 0 and tot["shared_block"] > 0, (sid, tot)
        assert tot["target_holds"] > 0 and tot["target_moves"] > 0, (sid, tot)
        assert tot["holds_at_boundary"] > 0 and tot["moves_at_boundary"] > 0, (sid, tot)
        assert tot["holds_at_boundary"] <= tot["target_holds"] and tot["moves_at_boundary"] <= tot["target_moves"], (sid, tot)
