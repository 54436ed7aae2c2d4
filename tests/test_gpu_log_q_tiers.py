"""The production kernel's log_q tiers against the oracle, in every hot-step variant (-m gpu).

hot_log_q (bisbm_sweep_fast.hip) picks, from wave-wide ballots over the (m_r, n_r) arguments of a pass, the q table, log_q_closed
(u^2 > 324, u = n_r / sqrt(m_r)), log_q_closed2 (169..324), log_q_mid (64..169) or log_q<true> itself (lower u, or lanes of one
pass in different tiers).  A branch of that ladder that evaluates the wrong function changes dS, the accepted moves and the sum,
which only a comparison with the oracle sees (an error of a few ulps -- the size of the device-vs-host libm differences the
comparison tolerates -- stays below what it resolves).  Here graphs with
heterogeneous block sizes put several tiers into every pass, at block counts that select each variant (step_oct, step_quad,
step_quad32, step_pair, step_pair64, one step per pass; the generic kernel as the control), under the constant, cooling and
early-stop template variants.  Every parametrisation asserts from the oracle's own m_r / n_r that it reaches the tiers it is
meant to, at the start and at the end."""
import importlib

import numpy as np
import pytest

import cases
import oracle_lib as O

pytestmark = pytest.mark.gpu

B = importlib.import_module("bipartitesbm-mcmc_amd")
SYN = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")
BIG = 1 << 60

# mean degree, block sizes cycled over the blocks of a type, the tiers the family reaches.  With m_r ~ n_r d after a shuffle,
# u^2 ~ n_r / d: high (d = 8): 1000 -> table (m_r ~ 8000), 1700 / 2100 -> 212 / 262 (closed2), 3500 / 6000 -> 437 / 750 (closed);
# low (d = 40): 200 -> table, 600 / 1500 -> 15 / 37 (low), 3000 / 5000 -> 75 / 125 (mid).
FAMILIES = {"high": (8, (1000, 1700, 2100, 3500, 6000), ("table", "closed2", "closed")),
            "low": (40, (200, 600, 1500, 3000, 5000), ("table", "low", "mid"))}
TIER_FLOOR = 2  # blocks per intended tier, at the start and at the end of the run

# id, Ka, Kb, environment, steps per pass the launch must report (bisbm_last_pass_steps)
SHAPES = [("oct", 8, 7, {"BISBM_PASS_DEPTH": "8"}, 8),
          ("quad", 16, 13, {"BISBM_PASS_DEPTH": "4"}, 4),
          ("quad32", 24, 32, {"BISBM_PASS_DEPTH": "4"}, 4),
          ("pair", 32, 24, {"BISBM_PASS_DEPTH": "2"}, 2),
          ("pair64", 48, 64, {}, 2),
          ("single", 24, 32, {"BISBM_SINGLE_STEPS": "1"}, 1),
          ("generic", 16, 13, {"BISBM_FORCE_GENERIC": "1"}, 1)]
ENV = ("BISBM_PASS_DEPTH", "BISBM_SINGLE_STEPS", "BISBM_FORCE_GENERIC", "BISBM_KEEP_SUM", "BISBM_LAUNCH_STEPS",
       "BISBM_FIXED_ROLES", "BISBM_ETA_WINDOW")
CHAINS = 5
PICKS = (0, CHAINS // 2, CHAINS - 1)
SEED = 2718


def family_sizes(family, ka, kb):
    """Type a cycles the family's sizes; type b cycles them from another phase, scaled so that both types hold about as many
    nodes (each edge adds one to the degree of a node of each type: equal node counts give both types the mean degree d)."""
    d, base = FAMILIES[family][:2]
    a = [base[i % len(base)] for i in range(ka)]
    b_raw = [base[(i + 2) % len(base)] for i in range(kb)]
    f = sum(a) / sum(b_raw)
    return d, a, [int(round(x * f)) for x in b_raw]


def sum_dS_close(got, o, rel=1e-9):
    """(tests/test_gpu_parity.py) 1e-9 relative, plus 1e-12 |S| for a sum advanced by differences of description lengths."""
    want = o.get_entropy()
    return abs(got - want) <= rel * abs(want) + 1e-12 * abs(o.entropy())


def _assert_reaches(o, tiers, family, shape, when):
    counts = cases.tier_counts(o.m_r(), o.n_r())
    print("%s / %s, %s: %s" % (family, shape, when, counts))
    for t in tiers:
        assert counts[t] >= TIER_FLOOR, (family, shape, when, t, counts)
    return counts


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_log_q_tiers_match_oracle(family, shape, monkeypatch):
    sid, ka, kb, env, pass_steps = shape
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d, sa, sb = family_sizes(family, ka, kb)
    na, nb = sum(sa), sum(sb)
    n = na + nb
    a, b = SYN.planted_edges(na, nb, d * na, ka, kb, seed=3)
    rowptr, col = O.edge_to_csr(a, b, n)
    labels = O.labels_from_sizes(sa + sb)
    # constant T = 1, steps_await out of reach (CT); cooling, out of reach; cooling from below T = 1 with the early stop in reach (EL)
    alpha = 0.5 ** (1.0 / n)
    calls = [("constant", [1.0], n, BIG), ("exponential", [1.5, alpha], n, BIG), ("exponential", [0.9, alpha], n, n // 2)]
    mh = B.MetropolisHasting()
    runs = {}
    for keep in ("0", "1"):  # the default running sum (from the description length where it may) and the step-by-step one
        monkeypatch.setenv("BISBM_KEEP_SUM", keep)
        g = B.BlockModel(labels, SYN.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rowptr, col), n_chains=CHAINS, rng="philox",
                         seed=SEED)
        g.shuffle_bisbm()
        snaps = []
        for s_, kw, dur, aw in calls:
            rates = np.atleast_1d(mh.anneal(g, s_, kw, dur, aw)).copy()
            assert g.last_pass_steps() == pass_steps, (family, sid, s_, g.last_pass_steps())
            acc, sw = g.last_counts()
            snaps.append(dict(rates=rates, acc=acc.copy(), sweeps=sw.copy(), cum=g.get_entropy().copy(),
                              state=[(g.get_memberships(c), g.get_m(c), g.get_m_r(c), g.get_n_r(c), g.get_eta_rk_(c))
                                     for c in PICKS]))
        runs[keep] = snaps
    monkeypatch.delenv("BISBM_KEEP_SUM")
    tiers = FAMILIES[family][2]
    for i, c in enumerate(PICKS):
        o = O.OracleModel(rowptr, col, na, nb, ka, kb, 1.0, labels)
        o.seed_philox(SEED, c)
        o.shuffle_bisbm()
        _assert_reaches(o, tiers, family, sid, "start, chain %d" % c)
        for j, (s_, kw, dur, aw) in enumerate(calls):
            ro = o.anneal(s_, kw, dur, aw)
            want = (o.memberships(), o.m(), o.m_r(), o.n_r(), o.eta())
            for keep in ("0", "1"):
                snap = runs[keep][j]
                what = (family, sid, s_, j, c, keep)
                assert snap["rates"][c] == ro, what
                assert snap["acc"][c] == o.last_accepted and snap["sweeps"][c] == o.last_sweeps, what
                for got, exp in zip(snap["state"][i], want):
                    assert (got == exp).all(), what
            # the step-by-step sum: the tolerance of the sum itself, no absolute escape
            assert abs(runs["1"][j]["cum"][c] - o.get_entropy()) <= 1e-9 * abs(o.get_entropy()), (family, sid, j, c)
            assert sum_dS_close(runs["0"][j]["cum"][c], o), (family, sid, j, c)
        _assert_reaches(o, tiers, family, sid, "end, chain %d" % c)
