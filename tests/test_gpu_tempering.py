"""GPU tests of replica exchange (include/bisbm.h, "Replica exchange"): a chain at a rung is the one-chain run at that
temperature (every pass of the production kernel and the generic kernel), the oracle and a numpy recomputation of every exchange
round, equal temperatures, stationarity of the cold and the hot rung on a graph small enough to enumerate, cold-chain marginals
(raw and aligned), several device entries, the refusals and the CLI."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_tempering import exchange_round

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu

LADDER = [1.0, 1.3, 2.0, 3.5]


def _planted(na, nb, edges, ka, kb, chains, seed=9, first_chain_id=0, **kw):
    a, b = syn.planted_edges(na, nb, edges, ka, kb, seed=4)
    rp, cl = B.edge_to_adj((a, b), na + nb)
    return B.BlockModel(syn.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rp, cl), n_chains=chains,
                        seed=seed, first_chain_id=first_chain_id, **kw)


def _state(m, c):
    return (m.get_memberships(c), m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c))


def _assert_same(x, y, what):
    for u, v, name in zip(x, y, ("labels", "m", "m_r", "n_r", "eta")):
        assert (u == v).all(), (what, name)


@pytest.mark.parametrize("k, generic", [(8, False), (16, False), (32, False), (64, False), (8, True)])
def test_chain_at_a_rung_is_the_one_chain_run(k, generic, monkeypatch):
    """tempering_run(s, 0): every chain runs s sweeps at its rung's temperature, bit-equal to a one-chain handle of the same
    global id run through run_sweeps(s, T) -- with 8 / 16 / 32 / 64 blocks a type the eight-, four-, two- and two-leaf passes
    of the production kernel run, and BISBM_FORCE_GENERIC=1 the generic kernel."""
    if generic:
        monkeypatch.setenv("BISBM_FORCE_GENERIC", "1")
    na = nb = 600
    sweeps, chains = 5, 8
    m = _planted(na, nb, 6000, k, k, chains)
    m.shuffle_bisbm()
    m.set_tempering(LADDER)
    m.tempering_run(sweeps, 0)
    rung, T = m.tempering_state()
    assert list(rung) == [c % 4 for c in range(chains)] and list(T) == [np.float32(LADDER[c % 4]) for c in range(chains)]
    assert m.tempering_stats()[2] == 0
    for c in range(chains):
        one = _planted(na, nb, 6000, k, k, 1, first_chain_id=c)
        one.shuffle_bisbm()
        one.run_sweeps(sweeps, temperature=LADDER[c % 4])
        _assert_same(_state(m, c), _state(one, 0), (k, generic, c))
        one.close()
    m.close()


def _oracle_graph(name):
    if name == "southernWomen":
        rowptr, col, na, nb = O.load_graph("southernWomen")
        return rowptr, col, na, nb, 3, 3
    rowptr, col, na, nb = O.load_graph("n_1000")
    return rowptr, col, na, nb, 4, 4


@pytest.mark.parametrize("graph", ["southernWomen", "n_1000"])
def test_exchanges_against_the_oracle(graph):
    """2 ensembles of L = 4, several calls of tempering_run(s, s): every chain equals an oracle chain annealed at its rung's
    temperature segment by segment, and the rungs and the counters equal a numpy recomputation of every round fed with the
    handle's own description lengths."""
    rowptr, col, na, nb, ka, kb = _oracle_graph(graph)
    n, L, chains, seed, s = na + nb, 4, 8, 21, 2
    ladder = [1.0, 1.2, 1.6, 2.5]
    labels = O.contiguous_labels(na, nb, ka, kb)
    m = B.BlockModel(labels, syn.types_vector(na, nb), ka + kb, ka, kb, 0.001 if graph == "southernWomen" else 1.0, (rowptr, col),
                     n_chains=chains, seed=seed)
    m.shuffle_bisbm()
    orc = []
    for c in range(chains):
        o = O.OracleModel(rowptr, col, na, nb, ka, kb, m.epsilon, labels)
        o.seed_philox(seed, c)
        o.shuffle_bisbm()
        orc.append(o)
    m.set_tempering(ladder)
    rung = np.array([c % L for c in range(chains)], dtype=np.uint32)
    att, acc = np.zeros(L - 1, dtype=np.uint64), np.zeros(L - 1, dtype=np.uint64)
    calls = 6
    for r in range(calls):
        for c in range(chains):
            orc[c].anneal("constant", [float(np.float32(ladder[rung[c]]))], s * n, 1 << 60)
        m.tempering_run(s, s)
        S = m.entropy()
        for c in range(chains):
            assert (orc[c].memberships() == m.get_memberships(c)).all(), (r, c)
            assert (orc[c].m() == m.get_m(c)).all(), (r, c)
            assert abs(orc[c].entropy() - S[c]) <= 1e-9 * abs(S[c]), (r, c)
        exchange_round(rung, S, ladder, seed, 0, r, att, acc)
        got_rung, got_T = m.tempering_state()
        assert (got_rung == rung).all(), (r, got_rung, rung)
        assert (got_T == np.array([np.float32(ladder[i]) for i in rung])).all()
        a2, c2, rounds = m.tempering_stats()
        assert (a2 == att).all() and (c2 == acc).all() and rounds == r + 1
    if graph == "southernWomen":
        assert acc.sum() > 0  # (swaps happened; on n_1000 the colder chains keep the shorter descriptions)
    m.close()


def test_ladder_of_equal_temperatures_is_a_no_op():
    chains, L = 16, 4
    m = _planted(500, 400, 5000, 6, 5, chains)
    plain = _planted(500, 400, 5000, 6, 5, chains)
    for g in (m, plain):
        g.shuffle_bisbm()
    m.set_tempering([1.0] * L)
    m.tempering_run(9, 1)
    plain.run_sweeps(9)
    for c in range(chains):
        assert (m.get_memberships(c) == plain.get_memberships(c)).all(), c
    att, acc, rounds = m.tempering_stats()
    assert rounds == 9 and (att == acc).all() and att.sum() == (chains // L) * (5 * 2 + 4 * 1)  # rounds 0, 2, ..: 2 pairs; odd: 1
    m.close()
    plain.close()


def _enum_model(chains, seed=3):
    rowptr, col = cases.enumerable_graph()
    na, nb = cases.ENUM_NA, cases.ENUM_NB
    return B.BlockModel(O.contiguous_labels(na, nb, 2, 2), syn.types_vector(na, nb), 4, 2, 2, cases.ENUM_EPS, (rowptr, col),
                        n_chains=chains, seed=seed)


def test_cold_and_hot_rungs_are_stationary():
    """Rung 0 samples exp(-S), rung 3 exp(-S / 4) on the enumerable graph (a sign error in delta sends the hot states to the cold
    rung and fails the cold check)."""
    states, prob1, S = cases.enumerable_states()
    ladder = [1.0, 1.6, 2.5, 4.0]
    chains = 4096
    m = _enum_model(chains)
    m.shuffle_bisbm()
    m.set_tempering(ladder)
    m.tempering_run(200, 1)
    cold, hot = [], []
    for _ in range(4):
        m.tempering_run(25, 1)
        rung, _ = m.tempering_state()
        for c in range(chains):
            if rung[c] == 0:
                cold.append(cases.state_code(m.get_memberships(c)))
            elif rung[c] == 3:
                hot.append(cases.state_code(m.get_memberships(c)))
    stat0, dof0, p0 = cases.chi_square(cold, states, prob1)
    assert p0 > 1e-3, (stat0, dof0)
    # exp(-S / 4) spreads over all 3844 states: compared in 12 bins of S, each of about equal probability
    w4 = np.exp(-(S - S.min()) / 4.0)
    w4 /= w4.sum()
    order = np.argsort(S, kind="stable")
    edges = np.searchsorted(np.cumsum(w4[order]), np.arange(1, 12) / 12.0)
    bin_of = np.empty(len(S), dtype=np.int64)
    bin_of[order] = np.searchsorted(edges, np.arange(len(S)), side="right")
    index = {int(x): i for i, x in enumerate(states)}
    obs = np.bincount([bin_of[index[h]] for h in hot], minlength=12)
    expct = np.bincount(bin_of, weights=w4, minlength=12) * len(hot)
    from scipy import stats
    stat3 = float(((obs - expct) ** 2 / expct).sum())
    p3 = float(stats.chi2.sf(stat3, 11))
    assert p3 > 1e-3, (stat3, obs, expct)
    att, acc, _ = m.tempering_stats()
    assert (acc > 0).all() and (acc < att).all()
    m.close()


def test_marginals_count_the_cold_chains_only():
    chains, L = 32, 4
    na, nb, ka, kb = 300, 200, 4, 4
    m = _planted(na, nb, 3000, ka, kb, chains)
    m.shuffle_bisbm()
    m.set_tempering([1.0] * L)  # (every swap accepted: the cold chains are others than at the start)
    m.tempering_run(5, 1)
    rung, _ = m.tempering_state()
    assert not (rung == np.array([c % L for c in range(chains)])).all()
    cold = [c for c in range(chains) if rung[c] == 0]
    assert len(cold) == chains // L
    lab = np.array([m.get_memberships(c) for c in range(chains)])
    m.marginals_reset()
    m.marginals_accumulate()
    assert (m.marginals_get() == D.numpy_marginals(lab[cold], na, ka, kb)).all()
    # aligned: the reference is the lowest-description-length cold chain, and only cold chains are counted through their perms
    S = m.entropy()
    m.marginals_reset()
    m.marginals_set_alignment(True)
    m.marginals_accumulate()
    ref, ref_chain = m.marginals_reference()
    assert ref_chain == cold[int(np.argmin(S[cold]))] and rung[ref_chain] == 0
    want = np.zeros((na + nb, max(ka, kb)), dtype=np.int64)
    base = np.where(np.arange(na + nb) >= na, ka, 0)
    for c in cold:
        perm, _ = m.marginals_alignment(c)
        np.add.at(want, (np.arange(na + nb), perm[lab[c]].astype(np.int64) - base), 1)
    assert (m.marginals_get() == want).all()
    # marginalize(tempering=...) takes its samples from the cold chains the same way
    m2 = _planted(na, nb, 3000, ka, kb, chains)
    m2.shuffle_bisbm()
    labels, counts = B.marginalize(m2, 3, 2, 1, tempering=[1.0, 1.5, 2.2, 3.0], exchange_every=1)
    assert counts.sum() == 2 * (chains // L) * (na + nb)
    assert m2.tempering_stats()[2] == 5
    m.close()
    m2.close()


def test_aligned_marginals_count_the_cold_chains_across_staging_chunks():
    # 136 chains: the permutation rows are staged 64 chains at a time, the 34 cold chains lie scattered over the three chunks
    chains, L = 136, 4
    na, nb, ka, kb = 300, 200, 4, 4
    m = _planted(na, nb, 3000, ka, kb, chains)
    m.shuffle_bisbm()
    m.set_tempering([1.0] * L)
    m.tempering_run(5, 1)
    rung, _ = m.tempering_state()
    cold = [c for c in range(chains) if rung[c] == 0]
    assert len(cold) == chains // L and cold[0] < 64 and 64 <= cold[len(cold) // 2] < 128 and cold[-1] >= 128
    lab = np.array([m.get_memberships(c) for c in range(chains)])
    S = m.entropy()
    m.marginals_reset()
    m.marginals_set_alignment(True)
    m.marginals_accumulate()
    ref, ref_chain = m.marginals_reference()
    assert ref_chain == cold[int(np.argmin(S[cold]))] and rung[ref_chain] == 0
    want = np.zeros((na + nb, max(ka, kb)), dtype=np.int64)
    base = np.where(np.arange(na + nb) >= na, ka, 0)
    for c in cold:
        perm, _ = m.marginals_alignment(c)
        np.add.at(want, (np.arange(na + nb), perm[lab[c]].astype(np.int64) - base), 1)
    assert (m.marginals_get() == want).all()
    m.close()


def test_several_entries_equal_one():
    chains = 16
    kw = dict(na=400, nb=300, edges=4000, ka=5, kb=5, chains=chains)
    one = _planted(**kw)
    many = _planted(**kw, devices=[0, 0])
    for g in (one, many):
        g.shuffle_bisbm()
        g.set_tempering(LADDER)
        g.tempering_run(7, 2)
        g.marginals_reset()
        g.marginals_accumulate()
    for c in range(chains):
        assert (one.get_memberships(c) == many.get_memberships(c)).all(), c
    r1, t1 = one.tempering_state()
    r2, t2 = many.tempering_state()
    assert (r1 == r2).all() and (t1 == t2).all()
    s1, s2 = one.tempering_stats(), many.tempering_stats()
    assert (s1[0] == s2[0]).all() and (s1[1] == s2[1]).all() and s1[2] == s2[2] == 3
    assert (one.marginals_get() == many.marginals_get()).all()
    # an entry of 6 chains cannot hold whole ensembles of 4
    odd = _planted(**dict(kw, chains=12), devices=[0, 0])
    with pytest.raises(B.BisbmError) as e:
        odd.set_tempering(LADDER)
    assert e.value.code == B.BISBM_ERR_INVALID_ARG and "straddle" in str(e.value)
    for g in (one, many, odd):
        g.close()


def test_refusals():
    L = B.lib()
    m = _planted(300, 200, 3000, 4, 4, 8)
    m.shuffle_bisbm()
    lad = np.array([1.0, 2.0, 1.5, 3.0], dtype=np.float32)
    assert L.bisbm_tempering_set(m._h, 4, lad.ctypes.data_as(B._f32p)) == B.BISBM_ERR_INVALID_ARG
    assert b"non-decreasing" in L.bisbm_last_error(m._h)
    lad = np.array([0.0, 1.0], dtype=np.float32)
    assert L.bisbm_tempering_set(m._h, 2, lad.ctypes.data_as(B._f32p)) == B.BISBM_ERR_INVALID_ARG
    lad = np.array([1.0, 2.0, 3.0], dtype=np.float32)
    assert L.bisbm_tempering_set(m._h, 3, lad.ctypes.data_as(B._f32p)) == B.BISBM_ERR_INVALID_ARG  # 8 chains, L = 3
    with pytest.raises(ValueError):
        m.set_tempering([1.0, 2.0, 3.0])
    with pytest.raises(B.BisbmError) as e:
        m.tempering_run(1, 1)
    assert e.value.code == B.BISBM_ERR_STATE
    # bisbm_anneal while tempering is on
    m.set_tempering(LADDER)
    with pytest.raises(B.BisbmError) as e:
        m.run_sweeps(1)
    assert e.value.code == B.BISBM_ERR_STATE and "bisbm_tempering_run" in str(e.value)
    m.set_tempering(None)
    m.run_sweeps(1)
    with pytest.raises(B.BisbmError):
        m.tempering_state()
    m.close()
    # a first global id inside an ensemble
    off = _planted(300, 200, 3000, 4, 4, 8, first_chain_id=2)
    with pytest.raises(B.BisbmError) as e:
        off.set_tempering(LADDER)
    assert e.value.code == B.BISBM_ERR_INVALID_ARG
    off.close()
    # mt19937-compat mode
    compat = _planted(300, 200, 3000, 4, 4, 4, rng="mt19937-compat")
    with pytest.raises(B.BisbmError) as e:
        compat.set_tempering(LADDER)
    assert e.value.code == B.BISBM_ERR_UNSUPPORTED
    compat.close()
    # mixed shapes after a one-argument merge
    rowptr, col, na, nb = O.load_graph("n_1000")
    g = B.BlockModel(O.contiguous_labels(na, nb, 6, 6), syn.types_vector(na, nb), 12, 6, 6, 1.0, (rowptr, col), n_chains=32, seed=4)
    g.shuffle_bisbm()
    g.run_sweeps(2)
    for _ in range(4):
        if g.mixed_shapes:
            break
        g.agg_merge(2, None, 10)
    assert g.mixed_shapes
    with pytest.raises(B.BisbmError) as e:
        g.set_tempering(LADDER)
    assert e.value.code == B.BISBM_ERR_STATE and "shape" in str(e.value)
    g.close()
    # tempering set first, then the device entries of a two-entry handle grouped by a one-argument merge: no sweeps, and no
    # histogram -- raw or aligned -- that would count the hot chains
    g = B.BlockModel(O.contiguous_labels(na, nb, 6, 6), syn.types_vector(na, nb), 12, 6, 6, 1.0, (rowptr, col), n_chains=32, seed=4,
                     devices=[0, 0])
    g.shuffle_bisbm()
    g.run_sweeps(2)
    g.set_tempering(LADDER)
    for _ in range(4):
        if g.mixed_shapes:
            break
        g.agg_merge(2, None, 10)
    assert g.mixed_shapes
    with pytest.raises(B.BisbmError) as e:
        g.tempering_run(1, 1)
    assert e.value.code == B.BISBM_ERR_STATE
    for align in (False, True):
        g.marginals_set_alignment(align)
        with pytest.raises(B.BisbmError) as e:
            g.marginals_accumulate()
        assert e.value.code == B.BISBM_ERR_STATE and "grouped by shape" in str(e.value), align
    g.close()


def test_cli_marginalize_with_tempering(tmp_path):
    n = 18 + 14
    el = os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    r = subprocess.run([cli, "-e", el, "-y", "18", "14", "-z", "2", "2", "-n", "9", "9", "7", "7", "-d", "5", "--rng", "philox", "--chains", "8",
                        "-b", str(20 * n), "-t", str(4 * n), "-f", str(n), "--marginalize", "--tempering", "1", "1.5", "2.5", "4"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert len(r.stdout.split()) == n
    assert "swap acceptance: 1<->1.5 " in r.stderr and "24 exchange round(s)" in r.stderr
