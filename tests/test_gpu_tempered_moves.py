"""GPU tests of heat-bath sweeps and pair reshuffles inside replica exchange (include/bisbm.h, "Heat-bath sweeps and pair
reshuffles inside replica exchange").

The replay drives an ensemble handle through tempering_rounds one round per call and, beside it, one one-chain handle per chain
(the same seed, first_chain_id = the chain's global id) through the EXISTING calls -- run_sweeps at the temperature the chain
holds, heatbath_sweeps and reshuffle at the host's quotient 1.0 / T -- and compares the two after every round: labels and block
state as integers, the running sum of dS on bit patterns.  The exchanges are recomputed in numpy (test_tempering.exchange_round)
from the handle's own description lengths, the per-rung tally (numpy_rung_tally) from what the one-chain handles report."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_gpu_heatbath import _bits, _case, _model, _refused
from test_tempering import exchange_round, philox

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu

SEED = 21


def _state(m, c):
    return (m.get_memberships(c), m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c))


def _assert_same(x, y, what):
    for u, v, name in zip(x, y, ("labels", "m", "m_r", "n_r", "eta")):
        assert (u == v).all(), (what, name)


def _oracle_model(graph, ka, kb, chains, seed=SEED, **kw):
    rowptr, col, na, nb = O.load_graph(graph)
    return B.BlockModel(O.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, 0.001 if graph == "southernWomen" else 1.0,
                        (rowptr, col), n_chains=chains, seed=seed, **kw)


def _beta(T):
    """the beta of a rung: the f64 quotient of the float temperature, as the host computes it"""
    return 1.0 / float(np.float32(T))


def _replay(make, ladder, chains, first_id, rounds, mh, hb, rs, scans):
    """make(n_chains, first_chain_id) -> a model.  Returns what the callers assert their edge on: the accepted exchanges, the
    chains that were compared after they had changed rung, the reshuffle records of every round."""
    L = len(ladder)
    m = make(chains, first_id)
    m.shuffle_bisbm()
    ones = []
    for c in range(chains):
        one = make(1, first_id + c)
        one.shuffle_bisbm()
        ones.append(one)
    n = m.n
    m.set_tempering(ladder)
    rung = np.array([c % L for c in range(chains)], dtype=np.uint32)
    att, acc = np.zeros(L - 1, dtype=np.uint64), np.zeros(L - 1, dtype=np.uint64)
    tally = np.zeros((L, 6), dtype=np.uint64)
    moved_rung, records = set(), []
    for r in range(rounds):
        m.tempering_rounds(1, mh=mh, heatbath=hb, reshuffles=rs, scans=scans)
        mh_acc, hb_moves, rs_acc = np.zeros(chains, np.uint64), np.zeros(chains, np.uint64), np.zeros(chains, np.uint64)
        for c, one in enumerate(ones):
            T = float(np.float32(ladder[rung[c]]))
            if mh:
                one.run_sweeps(mh, temperature=T)
                mh_acc[c] = one.last_counts()[0][0]
            if hb:
                hb_moves[c] = one.heatbath_sweeps(hb, _beta(T))[0]
            if rs:
                rs_acc[c] = one.reshuffle(rs, scans, _beta(T))[0]
            _assert_same(_state(m, c), _state(one, 0), (r, c))
            assert _bits(m.get_entropy())[c] == _bits(one.get_entropy())[0], (r, c)
            if rung[c] != c % L:
                moved_rung.add(c)
        if rs:
            records.append(m.reshuffle_last())
        B.numpy_rung_tally(tally, rung, mh_steps=mh * n, mh_accepted=mh_acc, heatbath_steps=hb * n, heatbath_moves=hb_moves, reshuffles=rs,
                           reshuffles_accepted=rs_acc)
        got = m.tempering_rung_stats()
        for i, name in enumerate(B.RUNG_STAT_COLUMNS):
            assert (got[name] == tally[:, i]).all(), (r, name, got[name], tally[:, i])
        # the exchange, recomputed from the handle's own description lengths
        S = m.entropy()
        exchange_round(rung, S, ladder, SEED, first_id, r, att, acc)
        got_rung, got_T = m.tempering_state()
        assert (got_rung == rung).all(), (r, got_rung, rung)
        assert (got_T == np.array([np.float32(ladder[i]) for i in rung])).all()
        a2, c2, n_rounds = m.tempering_stats()
        assert (a2 == att).all() and (c2 == acc).all() and n_rounds == r + 1
    # the columns add up to the chains' own totals
    got = m.tempering_rung_stats()
    assert got["reshuffles"].sum() == m.reshuffles_total().sum() == rs * rounds * chains
    assert got["mh_steps"].sum() == mh * n * rounds * chains and got["heatbath_steps"].sum() == hb * n * rounds * chains
    last_acc, last_sw = m.last_counts()  # (of the last kernel of the last round that writes them: heat bath, else MH)
    assert (last_sw == (hb if hb else mh)).all()
    assert last_acc.sum() == (hb_moves if hb else mh_acc).sum()
    for x in ones + [m]:
        x.close()
    return acc, moved_rung, records


def test_replay_southern_women_four_rungs():
    """3 + 3 blocks, L = 4, two ensembles, 6 rounds of {1, 1, 2 scans 2}: swaps occur, and chains that have changed rung are among
    those compared (they run their next round at the new temperature, which the one-chain handle is told)."""
    acc, moved, _ = _replay(lambda ch, first: _oracle_model("southernWomen", 3, 3, ch, first_chain_id=first), [1.0, 1.2, 1.6, 2.5], 8, 0, 6, 1, 1, 2, 2)
    print("southernWomen: accepted exchanges per pair %s, chains compared after a change of rung: %s" % (acc.tolist(), sorted(moved)))
    assert acc.sum() > 0 and len(moved) > 0


def test_replay_hubs_isolated_inexact_beta_and_a_second_chunk_of_members():
    """5 + 7 blocks on 300 + 200 nodes with hubs (rows past 64) and isolated nodes, ladder [1, 1.5] (1 / 1.5 is inexact), first id 4,
    3 rounds of {0, 1, 1 scans 1}: a pair of type-a blocks holds about 120 members, a second chunk of 64."""
    name = "hubs_isolated"
    _, _, recs = _replay(lambda ch, first: _model(name, ch, first_chain_id=first), [1.0, 1.5], 4, 4, 3, 0, 1, 1, 1)
    assert max(x["M"] for rec in recs for x in rec) > 64


def test_replay_n1000_unequal_block_counts():
    """4 + 6 blocks, L = 2, 2 rounds of {1, 0, 1 scans 3}: ka != kb, and the pairs drawn include one of type b."""
    _, _, recs = _replay(lambda ch, first: _oracle_model("n_1000", 4, 6, ch, first_chain_id=first), [1.0, 1.3], 4, 0, 2, 1, 0, 1, 3)
    types = {x["type"] for rec in recs for x in rec}
    assert types == {0, 1}, types
    # ... as the host's restatement of the pair says
    want = {D.numpy_reshuffle_pair(philox(SEED, g, B.PHILOX_PURPOSE_RESHUFFLE, j << 32)[0], 4, 6)[0] for g in range(4) for j in range(2)}
    assert want == {0, 1}


def test_replay_eta_in_hbm():
    """10 + 10 blocks and a hub of degree ~600: eta stays in HBM (the EL = false kernels); 1 round of {0, 1, 1}."""
    name = "hb_eta_in_hbm"
    _replay(lambda ch, first: _model(name, ch, first_chain_id=first), [1.0, 1.4], 2, 0, 1, 0, 1, 1, 3)


# ------------------------------------------------------------------------------------------------------------ equivalences
def _planted(chains, **kw):
    a, b = syn.planted_edges(400, 300, 4000, 5, 4, seed=4)
    rp, cl = B.edge_to_adj((a, b), 700)
    return B.BlockModel(syn.contiguous_labels(400, 300, 5, 4), syn.types_vector(400, 300), 9, 5, 4, 1.0, (rp, cl), n_chains=chains, seed=9, **kw)


LADDER = [1.0, 1.3, 2.0, 3.5]


def test_mh_only_rounds_are_tempering_run():
    chains, R, k = 8, 4, 2
    a, b = _planted(chains), _planted(chains)
    for g in (a, b):
        g.shuffle_bisbm()
        g.set_tempering(LADDER)
    a.tempering_rounds(R, mh=k, heatbath=0, reshuffles=0)
    b.tempering_run(R * k, k)
    for c in range(chains):
        _assert_same(_state(a, c), _state(b, c), c)
    assert (_bits(a.get_entropy()) == _bits(b.get_entropy())).all()
    assert all((x == y).all() for x, y in zip(a.tempering_state(), b.tempering_state()))
    sa, sb = a.tempering_stats(), b.tempering_stats()
    assert (sa[0] == sb[0]).all() and (sa[1] == sb[1]).all() and sa[2] == sb[2] == R
    ra, rb = a.tempering_rung_stats(), b.tempering_rung_stats()
    for name in B.RUNG_STAT_COLUMNS:
        assert (ra[name] == rb[name]).all(), name
    assert ra["mh_steps"].sum() == R * k * a.n * chains and ra["mh_accepted"].sum() > 0 and ra["heatbath_steps"].sum() == 0
    a.close()
    b.close()


def test_a_ladder_of_equal_temperatures_is_the_plain_calls():
    chains, R = 8, 3
    a, plain = _planted(chains), _planted(chains)
    for g in (a, plain):
        g.shuffle_bisbm()
    a.set_tempering([1.0, 1.0])
    a.tempering_rounds(R, mh=1, heatbath=1, reshuffles=2, scans=3)
    for _ in range(R):
        plain.run_sweeps(1)
        plain.heatbath_sweeps(1, 1.0)
        plain.reshuffle(2, 3, 1.0)
    for c in range(chains):
        _assert_same(_state(a, c), _state(plain, c), c)
    assert (_bits(a.get_entropy()) == _bits(plain.get_entropy())).all()
    rec_a, rec_p = a.reshuffle_last(), plain.reshuffle_last()
    assert rec_a == rec_p
    a.close()
    plain.close()


def test_several_entries_equal_one():
    chains = 16
    one, many = _planted(chains), _planted(chains, devices=[0, 0])
    for g in (one, many):
        g.shuffle_bisbm()
        g.set_tempering(LADDER)
        g.tempering_rounds(3, mh=1, heatbath=1, reshuffles=2, scans=2)
    for c in range(chains):
        assert (one.get_memberships(c) == many.get_memberships(c)).all(), c
    assert (_bits(one.get_entropy()) == _bits(many.get_entropy())).all()
    assert all((x == y).all() for x, y in zip(one.tempering_state(), many.tempering_state()))
    s1, s2 = one.tempering_stats(), many.tempering_stats()
    assert (s1[0] == s2[0]).all() and (s1[1] == s2[1]).all() and s1[2] == s2[2] == 3
    r1, r2 = one.tempering_rung_stats(), many.tempering_rung_stats()
    for name in B.RUNG_STAT_COLUMNS:
        assert (r1[name] == r2[name]).all(), name
    assert one.reshuffle_last() == many.reshuffle_last()
    one.close()
    many.close()


def test_without_exchange_rungs_and_rounds_stay():
    chains = 8
    m = _planted(chains)
    m.shuffle_bisbm()
    m.set_tempering(LADDER)
    m.tempering_rounds(3, mh=1, heatbath=1, reshuffles=1, exchange=False)
    rung, T = m.tempering_state()
    assert list(rung) == [c % 4 for c in range(chains)] and list(T) == [np.float32(LADDER[c % 4]) for c in range(chains)]
    att, acc, rounds = m.tempering_stats()
    assert rounds == 0 and att.sum() == 0 and acc.sum() == 0
    got = m.tempering_rung_stats()
    assert (got["reshuffles"] == 3 * chains // 4).all() and (got["heatbath_steps"] == 3 * m.n * chains // 4).all()
    m.close()


# ------------------------------------------------------------------------------------------------------------ stationarity
def test_both_rungs_are_stationary_under_mixed_rounds():
    """65536 chains on the enumerable 6 + 6 graph as 32768 ensembles of L = 2, ladder [1, 1.6], 60 rounds of {1, 1, 2 scans 1} with
    exchange from a randomised start (heat-bath sweeps alone pass their test after 100 sweeps, reshuffles alone after 400 moves of
    acceptance >= 0.1; a round here holds one MH sweep, one heat-bath sweep, two reshuffles and an exchange).  The 32768 chains on
    rung 0 against exp(-(S - S_min) / T0), those on rung 1 against T1; a state with an empty block makes chi_square raise.  A
    beta taken from the wrong rung, or the launch-wide beta, fails one of the two."""
    rowptr, col = cases.enumerable_graph()
    na, nb = cases.ENUM_NA, cases.ENUM_NB
    chains, rounds = 65536, 60
    ladder = [1.0, 1.6]
    g = B.BlockModel(O.contiguous_labels(na, nb, 2, 2), syn.types_vector(na, nb), 4, 2, 2, cases.ENUM_EPS, (rowptr, col), n_chains=chains,
                     rng="philox", seed=4242)
    g.shuffle_bisbm()
    g.set_tempering(ladder)
    g.tempering_rounds(rounds, mh=1, heatbath=1, reshuffles=2, scans=1)
    rung, _ = g.tempering_state()
    codes = np.array([cases.state_code(g.get_memberships(c)) for c in range(chains)])
    att, acc, n_rounds = g.tempering_stats()
    st = g.tempering_rung_stats()
    g.close()
    states, _, S = cases.enumerable_states()
    assert n_rounds == rounds and (rung == 0).sum() == (rung == 1).sum() == chains // 2
    rs_rate = st["reshuffles_accepted"] / st["reshuffles"]
    print("swaps %d / %d; reshuffle acceptance per rung %s; heat-bath move share per rung %s"
          % (acc[0], att[0], rs_rate.tolist(), (st["heatbath_moves"] / st["heatbath_steps"]).tolist()))
    assert 0 < acc[0] < att[0] and (st["reshuffles_accepted"] > 0).all()
    for i, T in enumerate(ladder):
        T = float(np.float32(T))
        target = np.exp(-(S - S.min()) / T)
        stat, dof, p = cases.chi_square(codes[rung == i], states, target / target.sum())
        print("rung %d (T = %g): chi2 = %.1f on %d dof, p = %.3g" % (i, T, stat, dof, p))
        assert p > 1e-3, (i, stat, dof, p)
        if i == 0:
            flat = np.exp(-(S - S.min()) / (1.25 * T))
            p_flat = cases.chi_square(codes[rung == i], states, flat / flat.sum())[2]
            print("rung 0 against the target flattened by 1.25: p = %.3g" % p_flat)
            assert p_flat < 1e-6


# ------------------------------------------------------------------------------------------------------------ population
def test_population_rounds_are_the_existing_calls():
    chains, temps, rounds = 64, [2.0, 1.5, 1.2, 1.0], 2
    a, b = _planted(chains), _planted(chains)
    for g in (a, b):
        g.shuffle_bisbm()
        g.run_sweeps(3, temperature=temps[0])
    out = a.population_rounds(temps, rounds, mh=1, heatbath=1, reshuffles=2, scans=2)
    T = B.validate_population_temps(temps)
    lr = []
    for k in range(1, len(T)):
        beta = 1.0 / float(T[k])
        lr.append(b.population_resample(1.0 / float(T[k - 1]), beta)[1])
        for _ in range(rounds):
            b.run_sweeps(1, temperature=float(T[k]))
            b.heatbath_sweeps(1, beta)
            b.reshuffle(2, 2, beta)
    for c in range(chains):
        _assert_same(_state(a, c), _state(b, c), c)
    sa, sb = a.population_state(), b.population_state()
    assert (sa["ancestor"] == sb["ancestor"]).all() and sa["rounds"] == sb["rounds"] == 3
    assert (_bits(out["log_ratio"]) == _bits(np.array(lr))).all() and _bits(sa["log_ratio_total"]) == _bits(sb["log_ratio_total"])
    assert len(set(sa["ancestor"].tolist())) < chains  # (the resampling did something)
    assert (out["distinct"] <= chains).all() and ((out["rates"] > 0) & (out["rates"] < 1)).all()
    # population_anneal(rung_moves=) is the same run
    c2 = _planted(chains)
    c2.shuffle_bisbm()
    res = B.population_anneal(c2, temps, rounds, burn_in_sweeps=3, rung_moves={"mh": 1, "heatbath": 1, "reshuffles": 2, "scans": 2})
    assert (_bits(res["log_ratio"]) == _bits(out["log_ratio"])).all() and (_bits(res["entropy"]) == _bits(a.entropy())).all()
    # refused as population_run, and a recipe of all zeros
    a.set_tempering([1.0, 2.0])
    assert "replica exchange" in _refused(lambda: a.population_rounds(temps, 1), B.BISBM_ERR_STATE)
    a.set_tempering(None)
    import ctypes as C
    rec = B.RoundRecipe(0, 0, 0, 3)
    assert B.lib().bisbm_rounds_population_run(a._h, len(T), T.ctypes.data_as(B._f32p), 1, C.byref(rec), None, None, None) == B.BISBM_ERR_INVALID_ARG
    assert B.lib().bisbm_rounds_population_run(a._h, len(T), T.ctypes.data_as(B._f32p), 1, None, None, None, None) == B.BISBM_ERR_INVALID_ARG
    for g in (a, b, c2):
        g.close()


# ------------------------------------------------------------------------------------------------------------ surfaces
def test_marginalize_runs_rounds():
    chains, ladder, moves = 8, [1.0, 1.5], {"mh": 1, "heatbath": 0, "reshuffles": 2, "scans": 3}
    m, m2 = _planted(chains), _planted(chains)
    for g in (m, m2):
        g.shuffle_bisbm()
    labels, counts = B.marginalize(m, 4, 3, 2, tempering=ladder, rung_moves=moves)
    m2.set_tempering(ladder)
    m2.tempering_rounds(4, mh=1, heatbath=0, reshuffles=2, scans=3)
    m2.marginals_reset()
    for _ in range(3):
        m2.tempering_rounds(2, mh=1, heatbath=0, reshuffles=2, scans=3)
        m2.marginals_accumulate(None)
    assert (counts == m2.marginals_get()).all() and counts.sum() == 3 * (chains // 2) * m.n
    assert m.tempering_stats()[2] == 10 and (m.tempering_rung_stats()["reshuffles"] == 10 * 2 * chains // 2).all()
    # marginalize_modes(reassign=True, tempering=, rung_moves=) runs rounds too
    m3 = _planted(chains)
    m3.shuffle_bisbm()
    res = B.marginalize_modes(m3, 2, 2, 1, threshold=0.5, reassign=True, tempering=ladder, rung_moves={"mh": 0, "heatbath": 1})
    assert m3.tempering_stats()[2] == 4 and (m3.tempering_rung_stats()["heatbath_steps"] == 4 * m3.n * chains // 2).all()
    assert res["counts"].sum() + res["unassigned"] * m3.n == 2 * (chains // 2) * m3.n
    for g in (m, m2, m3):
        g.close()


def test_the_cli_runs_rounds_and_reports_the_rungs():
    rowptr, col, na, nb = O.load_graph("n_1000")
    n, chains, seed = na + nb, 8, 5
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    labels0 = O.contiguous_labels(na, nb, 3, 3)
    m = B.BlockModel(labels0, syn.types_vector(na, nb), 6, 3, 3, 1.0, (rowptr, col), n_chains=chains, seed=seed)
    m.shuffle_bisbm()
    labels, counts = B.marginalize(m, 5, 3, 2, align=True, tempering=[1.0, 1.5], rung_moves={"mh": 1, "heatbath": 1, "reshuffles": 2, "scans": 2})
    st = m.tempering_rung_stats()
    sizes = [str(x) for x in np.bincount(labels0)]
    r = subprocess.run([cli, "-e", el, "-y", str(na), str(nb), "-z", "3", "3", "-n", *sizes, "-r", "-d", str(seed), "--rng", "philox", "--chains",
                        str(chains), "-b", str(5 * n), "-t", str(6 * n), "-f", str(2 * n), "--marginalize", "--align", "--tempering", "1", "1.5",
                        "--rung_moves", "1", "1", "2", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout == B.output_vec(labels, stream=open(os.devnull, "w"))
    assert "11 exchange round(s)" in r.stderr
    for i, T in enumerate(("1", "1.5")):
        want = " T=%s mh %d/%d heatbath %d/%d reshuffle %d/%d (" % (T, st["mh_accepted"][i], st["mh_steps"][i], st["heatbath_moves"][i],
                                                                   st["heatbath_steps"][i], st["reshuffles_accepted"][i], st["reshuffles"][i])
        assert want in r.stderr, (want, r.stderr)
    # --population_moves: the population run as rounds
    r = subprocess.run([cli, "-e", el, "-y", str(na), str(nb), "-z", "3", "3", "-n", *sizes, "-r", "-d", str(seed), "--rng", "philox", "--chains",
                        str(chains), "--population", "2", "1.5", "1", "--population_sweeps", "2", "--population_moves", "1", "1", "1", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "population: 2 steps" in r.stderr and len(r.stdout.split()) == n, r.stderr
    m2 = B.BlockModel(labels0, syn.types_vector(na, nb), 6, 3, 3, 1.0, (rowptr, col), n_chains=chains, seed=seed)
    m2.shuffle_bisbm()
    res = B.population_anneal(m2, [2, 1.5, 1], 2, burn_in_sweeps=2, rung_moves={"mh": 1, "heatbath": 1, "reshuffles": 1, "scans": 2})
    assert "log ratio %.17g" % res["log_ratio"][1] in r.stderr, r.stderr
    m.close()
    m2.close()


def test_refusals():
    m = _planted(8)
    assert "bisbm_tempering_set" in _refused(lambda: m.tempering_rounds(1), B.BISBM_ERR_STATE)  # tempering off
    m.set_tempering(LADDER)
    assert "bisbm_init" in _refused(lambda: m.tempering_rounds(1, heatbath=1), B.BISBM_ERR_STATE)  # (labels set, block state not built)
    m.shuffle_bisbm()
    import ctypes as C
    L = B.lib()
    rec = B.RoundRecipe(0, 0, 0, 3)
    assert L.bisbm_tempering_run_rounds(m._h, 1, C.byref(rec), 1) == B.BISBM_ERR_INVALID_ARG and b"runs nothing" in L.bisbm_last_error(m._h)
    assert L.bisbm_tempering_run_rounds(m._h, 1, None, 1) == B.BISBM_ERR_INVALID_ARG and b"recipe is NULL" in L.bisbm_last_error(m._h)
    assert L.bisbm_tempering_rung_stats(m._h, None) == B.BISBM_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        m.tempering_rounds(1, mh=0)
    # the plain calls stay refused while replica exchange is on
    assert "replica exchange" in _refused(lambda: m.heatbath_sweeps(1), B.BISBM_ERR_STATE)
    assert "replica exchange" in _refused(lambda: m.reshuffle(1), B.BISBM_ERR_STATE)
    m.tempering_rounds(1, heatbath=1, reshuffles=1)  # (and the handle is served after the refusals)
    m.close()
    # compat mode never gets as far: set_tempering refuses it
    compat = _planted(4, rng="mt19937-compat")
    _refused(lambda: compat.set_tempering([1.0, 2.0]), B.BISBM_ERR_UNSUPPORTED)
    _refused(lambda: compat.tempering_rounds(1), B.BISBM_ERR_STATE)
    compat.close()
    # a wide handle (200 + 150 blocks: two-byte labels): heat bath and reshuffles are not served
    wide = _model("wide_labels", 2)
    wide.shuffle_bisbm()
    wide.set_tempering([1.0, 2.0])
    assert "byte labels" in _refused(lambda: wide.tempering_rounds(1, mh=1, heatbath=1), B.BISBM_ERR_UNSUPPORTED)
    assert "byte labels" in _refused(lambda: wide.tempering_rounds(1, mh=1, reshuffles=1), B.BISBM_ERR_UNSUPPORTED)
    wide.close()
    # chains grouped by shape after tempering was set (a two-entry handle, as tests/test_gpu_tempering.py groups it)
    rowptr, col, na, nb = O.load_graph("n_1000")
    g = B.BlockModel(O.contiguous_labels(na, nb, 6, 6), syn.types_vector(na, nb), 12, 6, 6, 1.0, (rowptr, col), n_chains=32, seed=4, devices=[0, 0])
    g.shuffle_bisbm()
    g.run_sweeps(2)
    g.set_tempering(LADDER)
    for _ in range(4):
        if g.mixed_shapes:
            break
        g.agg_merge(2, None, 10)
    assert g.mixed_shapes
    assert "shape" in _refused(lambda: g.tempering_rounds(1, heatbath=1), B.BISBM_ERR_STATE)
    g.close()


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "tempered_moves.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "rung  T" in r.stdout and "reshuffles accepted" in r.stdout, r.stdout + r.stderr
