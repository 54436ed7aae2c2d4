"""The update of m_r / n_r behind a deep pass's verdicts, on the GPU (-m gpu).

step_quad32 exists twice.  One kernel walks the movers of a pass one by one, as step_quad and step_oct do; in the other every row
of lanes forms its step's contribution to the lane's two blocks in the shadow of the table gathers (move_word,
csrc/bisbm_move_word.hpp; the lane arithmetic itself is checked on the CPU by test_move_word.py), and after the verdicts the
movers' words are combined with two lane swaps.  The host picks one per launch from the accepted fraction of the launch before;
BISBM_ONE_STAGE pins it.  Here the chains of a pinned deep pass equal those of two steps per pass and of one step per pass to
the bit -- rates, counts, labels, m, m_r, n_r, eta and, kept step by step, the bits of the running sum -- and one chain per
shape equals the oracle's, on the smallest graphs at which that stage can still go wrong:
  * hubs32: 20 + 27 blocks (step_quad32, BISBM_ONE_STAGE = 1 and 0: two blocks per lane column, blocks on both sides of 16,
    ka != kb) with hub nodes of degree 128, 200, 210 and 220 -- an m_r addend that fits no signed byte; the graph's largest
    degree puts eta in window mode, whose window [1, 225] holds them, so they take the hot pass (degree 255 itself is the CPU
    check's) -- and one of degree 300, which takes the general path in the middle of a chunk; more than half of the steps are
    accepted, so passes with two, three and four movers occur;
  * k16 (16 + 13, step_quad) and k8 (8 + 7, step_oct at depth 8, step_quad at depth 4), whose loop lives in the same
    apply_moves, from a randomised start on a weakly structured graph with more than half of the steps accepted;
  * every shape: type sizes that are no multiple of 64 (the last pass of a chunk has fewer steps than the pass is wide), and a
    second call under an exponential schedule that cools into the greedy T = 0 tail with steps_await in reach (the early-stop
    bookkeeping's path, which keeps the running sum and the minimum in step order)."""
import functools
import importlib

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_target_rescue import ENV

pytestmark = pytest.mark.gpu

B = importlib.import_module("bipartitesbm-mcmc_amd")
SYN = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")
BIG = 1 << 60
CHAINS = 4
SWEEPS = 3
SEED = 1234

# id, na, nb, edges, Ka, Kb, graph seed, hubs ((node, degree) ...), pinned depths, BISBM_ONE_STAGE pins (None: left to the host)
SHAPES = [("hubs32", 1517, 1490, 15000, 20, 27, 31, ((3, 200), (700, 220), (1400, 300), (1517 + 5, 128), (1517 + 800, 210)), ("4",), ("1", "0")),
          ("k16", 1610, 1390, 16000, 16, 13, 32, (), ("4",), (None,)),
          ("k8", 810, 690, 8000, 8, 7, 33, (), ("8", "4"), (None,))]


@functools.lru_cache(maxsize=None)
def _graph(sid):
    _, na, nb, ne, ka, kb, seed, hubs, _, _ = next(s for s in SHAPES if s[0] == sid)
    a, b = SYN.planted_edges(na, nb, ne, ka, kb, seed=seed, p_in=0.3)
    rng = np.random.default_rng(seed + 1000)
    deg = np.bincount(np.concatenate([a, b]).astype(np.int64), minlength=na + nb)
    for node, want in hubs:  # edges to uniform nodes of the other type until the hub has exactly its degree
        more = want - int(deg[node])
        assert more > 0, (sid, node, deg[node])
        other = rng.integers(na, na + nb, more) if node < na else rng.integers(0, na, more)
        other[np.isin(other, [h for h, _ in hubs])] += 1  # (no edge between two hubs: each keeps exactly its degree)
        mine = np.full(more, node)
        a = np.concatenate([a, (mine if node < na else other).astype(np.uint64)])
        b = np.concatenate([b, (other if node < na else mine).astype(np.uint64)])
        deg = np.bincount(np.concatenate([a, b]).astype(np.int64), minlength=na + nb)
    rowptr, col = O.edge_to_csr(a, b, na + nb)
    for node, want in hubs:
        assert int(rowptr[node + 1] - rowptr[node]) == want, (sid, node)
    return rowptr, col, O.contiguous_labels(na, nb, ka, kb)


def _calls(n):
    # the second call: T = 0.9 * 2^(-1200 t / n) is below 2^-1074 before the first sweep ends -- the rest is the greedy tail
    return [("constant", [1.0], SWEEPS * n, BIG), ("exponential", [0.9, 0.5 ** (1200.0 / n)], SWEEPS * n, n)]


def _run(monkeypatch, shape, env, keep):
    sid, na, nb, ne, ka, kb = shape[:6]
    for k in ENV + ("BISBM_ONE_STAGE",):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("BISBM_KEEP_SUM", keep)
    rowptr, col, labels = _graph(sid)
    g = B.BlockModel(labels, SYN.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rowptr, col), n_chains=CHAINS, rng="philox", seed=SEED)
    g.shuffle_bisbm()
    snaps = []
    for sched, kw, dur, aw in _calls(na + nb):
        rates = np.atleast_1d(B.MetropolisHasting().anneal(g, sched, kw, dur, aw)).copy()
        acc, sw = g.last_counts()
        snaps.append(dict(pass_steps=g.last_pass_steps(), rates=rates, acc=acc.copy(), sweeps=sw.copy(), cum=g.get_entropy().copy(),
                          state=[(g.get_memberships(c), g.get_m(c), g.get_m_r(c), g.get_n_r(c), g.get_eta_rk_(c)) for c in range(CHAINS)]))
    for k in list(env) + ["BISBM_KEEP_SUM"]:
        monkeypatch.delenv(k, raising=False)
    return snaps


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_deep_pass_updates_equal_shallow_ones_and_the_oracle(shape, monkeypatch):
    sid, na, nb, ne, ka, kb, _, hubs, depths, stages = shape
    n = na + nb
    assert na % 64 != 0 and nb % 64 != 0
    rowptr, col, labels = _graph(sid)
    calls = _calls(n)
    oracle = []  # chain 0, after each call
    o = O.OracleModel(rowptr, col, na, nb, ka, kb, 1.0, labels)
    o.seed_philox(SEED, 0)
    o.shuffle_bisbm()
    for sched, kw, dur, aw in calls:
        rate = o.anneal(sched, kw, dur, aw)
        oracle.append(dict(rate=rate, acc=o.last_accepted, sweeps=o.last_sweeps, cum=o.get_entropy(), entropy=o.entropy(),
                           state=(o.memberships(), o.m(), o.m_r(), o.n_r(), o.eta())))
    for keep in ("0", "1"):
        refs = [(_run(monkeypatch, shape, {"BISBM_PASS_DEPTH": "2"}, keep), 2), (_run(monkeypatch, shape, {"BISBM_SINGLE_STEPS": "1"}, keep), 1)]
        for ref, steps in refs:
            assert [s["pass_steps"] for s in ref] == [steps] * len(calls), (sid, keep, steps)
        for depth, stage in [(d, st) for d in depths for st in stages]:
            got = _run(monkeypatch, shape, dict({"BISBM_PASS_DEPTH": depth}, **({} if stage is None else {"BISBM_ONE_STAGE": stage})), keep)
            assert [s["pass_steps"] for s in got] == [int(depth)] * len(calls), (sid, keep, depth)
            accepted = got[0]["acc"].sum() / float(CHAINS * SWEEPS * n)
            print(sid, "keep", keep, "depth", depth, "one stage", stage, "accepted fraction of the constant call %.3f" % accepted, "sweeps of the cooling call",
                  got[1]["sweeps"])
            assert (got[0]["sweeps"] == SWEEPS).all(), (sid, keep, depth)
            assert accepted > 0.5, (sid, keep, depth, accepted)  # (otherwise passes with several movers are rare)
            for j in range(len(calls)):
                for ref, steps in refs:
                    what = (sid, keep, depth, stage, steps, j)
                    assert (got[j]["rates"] == ref[j]["rates"]).all(), what
                    assert (got[j]["acc"] == ref[j]["acc"]).all() and (got[j]["sweeps"] == ref[j]["sweeps"]).all(), what
                    for c in range(CHAINS):
                        for a, b in zip(got[j]["state"][c], ref[j]["state"][c]):
                            assert (np.asarray(a) == np.asarray(b)).all(), what + (c,)
                    if keep == "1":  # the running sum kept step by step: the same additions in the same order
                        assert (got[j]["cum"].view(np.uint64) == ref[j]["cum"].view(np.uint64)).all(), what
                want, what = oracle[j], (sid, keep, depth, stage, "oracle", j)
                assert got[j]["rates"][0] == want["rate"], what
                assert got[j]["acc"][0] == want["acc"] and got[j]["sweeps"][0] == want["sweeps"], what
                for a, b in zip(got[j]["state"][0], want["state"]):
                    assert (np.asarray(a) == np.asarray(b)).all(), what
                tol = 1e-9 * abs(want["cum"]) + (0. if keep == "1" else 1e-12 * abs(want["entropy"]))  # (test_gpu_target_rescue.py's bound)
                assert abs(got[j]["cum"][0] - want["cum"]) <= tol, what
