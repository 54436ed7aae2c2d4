"""GPU tests of population annealing (include/bisbm.h, "Population annealing"): one resampling step of a handle against its
definition (the parent map of bisbm_population_offspring, every copied state against its parent's, survivors untouched), a copy
that continues as the chain of its slot, the sum-of-dS bookkeeping across a step, two device entries against one, the evidence
estimate against exact enumeration, the refusals, the CLI and the example."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_population import PHX_RESAMPLE, model_step
from test_tempering import philox, u53

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
SYN = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu

NA, NB = 903, 701  # neither a multiple of 16; label rows are padded to 1792
SEED = 77


@pytest.fixture(scope="module")
def graph():
    return cases.random_graph(11, NA, NB, 8000, 6, 5)


def _model(graph, ka, kb, chains, **kw):
    return B.BlockModel(O.contiguous_labels(NA, NB, ka, kb), SYN.types_vector(NA, NB), ka + kb, ka, kb, 1.0, graph, n_chains=chains, seed=SEED, **kw)


def _spread(m):
    """Chains at different distances from a shuffle: chain c holds the partition it had after c mod 4 sweeps at T = 1.  The
    running sums of dS are those after 3 sweeps: a different number in every chain."""
    m.shuffle_bisbm()
    snap = {}
    for s in range(4):
        for c in range(s, m.n_chains, 4):
            snap[c] = m.get_memberships(c)
        if s < 3:
            m.run_sweeps(1)
    for c, lab in snap.items():
        m.set_memberships(lab, chain=c)
    m.init_bisbm()


def _state(m, c):
    return (m.get_memberships(c), m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c))


def _same(x, y):
    return all((u == v).all() for u, v in zip(x, y))


def _u(first_chain_id, rnd):
    w = philox(SEED, first_chain_id, PHX_RESAMPLE, rnd)
    return u53(w[0], w[1])


# ------------------------------------------------------------------ one step is its definition
@pytest.mark.parametrize("ka, kb", [(6, 5), (32, 32), (128, 128)])
@pytest.mark.parametrize("chains, first", [(7, 3), (33, 0)])
def test_one_step_is_its_definition(graph, ka, kb, chains, first):
    """Three steps in a row -- delta = 0, about 1 / std(S), 50 -- so the round counter moves and the last step meets the ties the
    one before left.  A chain's m is ka * kb * 4 bytes: 120 for 6 + 5, so the slices of chains 1, 3, 5 ... are not 16-byte aligned."""
    m = _model(graph, ka, kb, chains, first_chain_id=first)
    _spread(m)
    assert m.population_state()["rounds"] == 0 and (m.population_state()["ancestor"] == np.arange(chains)).all()
    ancestor, total, beta = np.arange(chains), 0.0, 0.25
    S0 = m.entropy()
    for rnd, delta in enumerate([0.0, 1.0 / S0.std(), 50.0]):
        S, cum = m.entropy(), m.get_entropy()
        before = [_state(m, c) for c in range(chains)]
        u = _u(first, rnd)
        delta = (beta + delta) - beta  # (what the step sees of it)
        want_n, want_parent, want_lr = B.population_offspring(S, delta, u)
        parent, lr = m.population_resample(beta, beta + delta)
        assert (beta + delta) - beta == delta
        beta += delta
        assert (parent == want_parent).all() and lr == want_lr, (rnd, parent, want_parent)
        mn, mparent, mlr, margin = model_step(S, delta, u)  # the numpy statement, where its integers are safe
        if delta > 0 and rnd == 1:
            print("ka %d kb %d C %d: delta %.4g, std(S) %.4g, margin %.3g, %d dead, largest family %d"
                  % (ka, kb, chains, delta, S.std(), margin, int((mn == 0).sum()), int(mn.max())))
            if margin >= 1e-9:
                assert (parent == mparent).all() and abs(lr - mlr) <= 1e-12 * abs(mlr)
        if rnd == 0:
            assert (parent == np.arange(chains)).all() and lr == 0.0
        if rnd == 1:
            assert 0 < (parent != np.arange(chains)).sum() < chains - 1, parent  # a step that copies some and keeps some
        if rnd == 2:
            assert (S[parent] == S.min()).all()  # (the copies of the lowest chain share the slots)
        S1, cum1 = m.entropy(), m.get_entropy()
        for c in range(chains):
            assert _same(_state(m, c), before[parent[c]]), (rnd, c, parent[c])
        assert (S1 == S[parent]).all() and (cum1 == cum[parent]).all()
        ancestor, total = ancestor[parent], total + lr
        st = m.population_state()
        assert (st["ancestor"] == ancestor).all() and st["rounds"] == rnd + 1 and st["log_ratio_total"] == total
    m.population_reset()
    st = m.population_state()
    assert (st["ancestor"] == np.arange(chains)).all() and st["rounds"] == 0 and st["log_ratio_total"] == 0.0
    m.close()


# ------------------------------------------------------------------ a copy continues as the chain of its slot
def test_a_copy_continues_as_the_chain_of_its_slot(graph):
    A, Bm = _model(graph, 6, 5, 33), _model(graph, 6, 5, 33)
    for m in (A, Bm):
        _spread(m)
    S = A.entropy()
    parent, _ = A.population_resample(1.0, 1.0 + 1.0 / S.std())
    dead = np.flatnonzero(parent != np.arange(33))
    assert len(dead) >= 4
    for d in dead:
        Bm.set_memberships(Bm.get_memberships(parent[d]), chain=int(d))
    Bm.init_bisbm()
    A.run_sweeps(3)
    Bm.run_sweeps(3)
    for c in range(33):
        assert _same(_state(A, c), _state(Bm, c)), c
    # the streams belong to the slot: copies of one parent part ways with it and with each other
    family = np.flatnonzero(parent == np.bincount(parent).argmax())
    assert len(family) >= 3
    labels = [A.get_memberships(c) for c in family]
    for i in range(len(family)):
        for j in range(i):
            assert (labels[i] != labels[j]).any(), (family[i], family[j])
    A.close()
    Bm.close()


# ------------------------------------------------------------------ sum-of-dS bookkeeping across a step
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_running_sum_follows_the_description_length_across_a_step(graph, devices):
    """The sweeps before the step leave the baseline of the running sum (the block-state part of every chain's description length)
    on the device; the step moves states under it.  After the step and 2 more sweeps the sum of every slot has moved, from its
    parent's, by the change of the description length -- to the tolerance tests/test_gpu_fuzz.py holds that identity to."""
    m = _model(graph, 32, 32, 33, **({"devices": devices} if devices else {}))
    _spread(m)
    m.run_sweeps(1)
    S, cum = m.entropy(), m.get_entropy()
    parent, _ = m.population_resample(1.0, 1.0 + 1.0 / S.std())
    assert (parent != np.arange(33)).sum() >= 4
    assert (m.entropy() == S[parent]).all() and (m.get_entropy() == cum[parent]).all()
    m.run_sweeps(2)
    S2, cum2 = m.entropy(), m.get_entropy()
    for c in range(33):
        d_cum, d_S = cum2[c] - cum[parent[c]], S2[c] - S[parent[c]]
        assert abs(d_cum - d_S) <= 1e-9 * max(1.0, abs(d_S)) + 1e-12 * abs(S2[c]), (c, parent[c], d_cum, d_S)
    m.close()


# ------------------------------------------------------------------ two device entries
def test_two_device_entries_equal_one(graph):
    one, two = _model(graph, 6, 5, 33), _model(graph, 6, 5, 33, devices=[0, 0])
    for m in (one, two):
        _spread(m)
    S = one.entropy()
    assert (two.entropy() == S).all()
    p1, l1 = one.population_resample(0.2, 0.2 + 1.0 / S.std())
    p2, l2 = two.population_resample(0.2, 0.2 + 1.0 / S.std())
    assert (p1 == p2).all() and l1 == l2
    first = two.device_layout()[1][1]  # the second entry's first chain
    assert first == 17
    assert any((p1[c] < first) != (c < first) for c in range(33)), p1  # some copy crosses the entries
    for c in range(33):
        assert _same(_state(one, c), _state(two, c)), c
    r1 = one.population_run([3, 2, 1.5, 1], 1)
    r2 = two.population_run([3, 2, 1.5, 1], 1)
    assert (r1["log_ratio"] == r2["log_ratio"]).all() and (r1["distinct"] == r2["distinct"]).all() and (r1["rates"] == r2["rates"]).all()
    assert (np.diff(r1["distinct"].astype(int)) <= 0).all()
    s1, s2 = one.population_state(), two.population_state()
    assert (s1["ancestor"] == s2["ancestor"]).all() and s1["rounds"] == s2["rounds"] == 4 and s1["log_ratio_total"] == s2["log_ratio_total"]
    assert len(np.unique(s1["ancestor"])) == r1["distinct"][-1]
    for c in range(33):
        assert _same(_state(one, c), _state(two, c)), c
    assert (one.entropy() == two.entropy()).all() and (one.get_entropy() == two.get_entropy()).all()
    one.close()
    two.close()


# ------------------------------------------------------------------ the evidence against exact enumeration
TEMPS = [4, 3, 2.4, 2, 1.7, 1.45, 1.25, 1.1, 1.0]


@pytest.fixture(scope="module")
def enumeration():
    states, _, S = cases.enumerable_states()
    return states, S


def _logsumexp(x):
    return float(x.max() + np.log(np.exp(x - x.max()).sum()))


@pytest.mark.parametrize("sweeps_per_step", [0, 2])
def test_evidence_against_exact_enumeration(enumeration, sweeps_per_step):
    """32768 chains on the 6 + 6-node graph, equilibrated at T = 4, annealed to T = 1 in 8 steps.  With sweeps_per_step = 0 the
    run is resampling only: no sweep can repair a wrong step.  log_ratio_total against ln sum exp(-S) - ln sum exp(-S / 4)
    over the 3844 states, within 6 sum_k sigma_k, sigma_k^2 = (E_k[w^2] / E_k[w]^2 - 1) / C at the step's own beta -- from the
    enumeration alone (exact value -32.3558, bound 0.027; weights without moved states are off by 0.26).  With sweeps the
    final population must also be a sample of exp(-S)."""
    states, S = enumeration
    rowptr, col = cases.enumerable_graph()
    na, nb = cases.ENUM_NA, cases.ENUM_NB
    C = 32768
    g = B.BlockModel(O.contiguous_labels(na, nb, 2, 2), SYN.types_vector(na, nb), 4, 2, 2, cases.ENUM_EPS, (rowptr, col), n_chains=C, seed=4242)
    g.shuffle_bisbm()
    g.run_sweeps(100, 4.0)
    out = g.population_run(TEMPS, sweeps_per_step)
    total = g.population_state()["log_ratio_total"]
    beta = [1.0 / float(np.float32(t)) for t in TEMPS]
    exact = _logsumexp(-beta[-1] * S) - _logsumexp(-beta[0] * S)
    sigma = 0.0
    for k in range(1, len(beta)):
        p = np.exp(-beta[k - 1] * (S - S.min()))
        p /= p.sum()
        w = np.exp(-(beta[k] - beta[k - 1]) * (S - S.min()))
        sigma += np.sqrt(((p * w * w).sum() / (p * w).sum() ** 2 - 1.0) / C)
    print("sweeps_per_step %d: log_ratio_total %.5f, exact %.5f, error %.5f, bound %.5f, distinct %s"
          % (sweeps_per_step, total, exact, total - exact, 6 * sigma, out["distinct"].tolist()))
    assert abs(out["log_ratio"].sum() - total) <= 1e-12 * abs(total)
    assert (np.diff(out["distinct"].astype(int)) <= 0).all() and out["distinct"][-1] < C
    assert abs(total - exact) <= 6 * sigma, (total, exact, 6 * sigma)
    if sweeps_per_step:
        codes = np.array([cases.state_code(g.get_memberships(c)) for c in range(C)])
        target = np.exp(-(S - S.min()))
        stat, dof, p = cases.chi_square(codes, states, target / target.sum())
        print("final population against exp(-S): chi2 = %.1f on %d dof, p = %.3g" % (stat, dof, p))
        assert p > 1e-3, (stat, dof, p)
    g.close()


# ------------------------------------------------------------------ refusals leave the handle as it was
def _refused(m, code, word):
    S, cum, lab, st = m.entropy(), m.get_entropy(), m.get_memberships(m.n_chains - 1), m.population_state()
    with pytest.raises(B.BisbmError) as e:
        m.population_resample(0.5, 1.0)
    assert e.value.code == code and word in str(e.value), str(e.value)
    with pytest.raises(B.BisbmError) as e:
        m.population_run([2, 1], 1)
    assert e.value.code == code and word in str(e.value), str(e.value)
    st1 = m.population_state()
    assert (st1["ancestor"] == st["ancestor"]).all() and st1["rounds"] == st["rounds"] and st1["log_ratio_total"] == st["log_ratio_total"]
    assert (m.get_entropy() == cum).all() and (m.get_memberships(m.n_chains - 1) == lab).all()
    assert (m.entropy() == S).all()


def test_refusals_leave_the_handle_as_it_was(graph):
    L = B.lib()
    # arguments, on a handle that is served
    m = _model(graph, 6, 5, 8)
    _spread(m)
    S, st = m.entropy(), m.population_state()
    for args in ((1.0, 0.5), (1.0, np.nan), (np.inf, np.inf), (-np.inf, 1.0)):
        with pytest.raises(B.BisbmError) as e:
            m.population_resample(*args)
        assert e.value.code == B.BISBM_ERR_INVALID_ARG
    for temps in ([1.0, 2.0], [2.0, 1.0, 1.5], [2.0, 0.0], [np.inf, 1.0], [2.0]):
        t = np.array(temps, dtype=np.float32)
        assert L.bisbm_population_run(m._h, len(t), t.ctypes.data_as(B._f32p), 1, None, None, None) == B.BISBM_ERR_INVALID_ARG, temps
        with pytest.raises(ValueError):
            m.population_run(temps, 1)
    assert (m.entropy() == S).all() and m.population_state()["rounds"] == st["rounds"] == 0
    # replica exchange on; static modes set (anchored modes are served)
    m.set_tempering([1.0, 2.0])
    _refused(m, B.BISBM_ERR_STATE, "replica exchange")
    m.set_tempering(None)
    m.marginals_set_modes([0, 0, 0, 0, 1, 1, 1, 1])
    _refused(m, B.BISBM_ERR_STATE, "mode")
    m.marginals_set_modes(None)
    m.population_resample(0.5, 1.0)
    assert m.population_state()["rounds"] == 1
    m.close()
    # mt19937-compat mode
    compat = _model(graph, 6, 5, 4, rng="mt19937-compat")
    compat.shuffle_bisbm()
    _refused(compat, B.BISBM_ERR_UNSUPPORTED, "Philox")
    compat.close()
    # two-byte labels
    _, na, nb, edges, ka, kb, eps, hubs, isolated = cases.CASE["wide_labels"]
    wide = B.BlockModel(O.contiguous_labels(na, nb, ka, kb), SYN.types_vector(na, nb), ka + kb, ka, kb, eps,
                        cases.random_graph(3, na, nb, edges, ka, kb, hubs, isolated), n_chains=2, seed=5)
    wide.init_bisbm()
    _refused(wide, B.BISBM_ERR_UNSUPPORTED, "wide")
    wide.close()
    # chains grouped by shape after a one-argument merge
    rowptr, col, na, nb = O.load_graph("n_1000")
    g = B.BlockModel(O.contiguous_labels(na, nb, 6, 6), SYN.types_vector(na, nb), 12, 6, 6, 1.0, (rowptr, col), n_chains=32, seed=4)
    g.shuffle_bisbm()
    g.run_sweeps(2)
    for _ in range(4):
        if g.mixed_shapes:
            break
        g.agg_merge(2, None, 10)
    assert g.mixed_shapes
    _refused(g, B.BISBM_ERR_STATE, "shape")
    g.close()


# ------------------------------------------------------------------ the CLI and the example
def test_cli_population_against_population_anneal():
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    sizes = [125, 125, 125, 125, 84, 84, 83, 83, 83, 83]
    temps = ["3", "2", "1.5", "1", "0.7"]
    r = subprocess.run([cli, "-e", el, "-y", "500", "500", "-z", "4", "6", "-n"] + [str(s) for s in sizes] +
                       ["-r", "-d", "7", "--rng", "philox", "--chains", "16", "--population"] + temps + ["--population_sweeps", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rowptr, col, na, nb = O.load_graph("n_1000")
    m = B.BlockModel(O.labels_from_sizes(sizes), SYN.types_vector(na, nb), 10, 4, 6, 1.0, (rowptr, col), n_chains=16, seed=7)
    m.shuffle_bisbm()
    out = B.population_anneal(m, [float(t) for t in temps], 2, burn_in_sweeps=2)
    assert r.stdout == B.output_vec(m.get_memberships(out["best_chain"]), stream=open(os.devnull, "w"))
    steps = [l.split() for l in r.stderr.splitlines() if l.startswith("population step ")]
    assert len(steps) == 4
    for k, w in enumerate(steps):  # population step K: T a -> b, log ratio X, distinct ancestors D
        assert float(w[9].rstrip(",")) == out["log_ratio"][k] and int(w[12]) == out["distinct"][k], w
    tot = [l.split() for l in r.stderr.splitlines() if l.startswith("population: ")]
    assert len(tot) == 1 and tot[0][1] == "4" and float(tot[0][-1]) == m.population_state()["log_ratio_total"]
    assert "printing chain %d\n" % out["best_chain"] in r.stderr
    m.close()


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "population_annealing.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "distinct ancestors after every step" in r.stdout and "evidence estimate" in r.stdout, r.stdout + r.stderr
