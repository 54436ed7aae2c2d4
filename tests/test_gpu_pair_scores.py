"""GPU tests of the pair scores (include/bisbm.h, "Posterior-predictive pair scores").  The reference is
distributed.numpy_pair_scores fed with what the handle's own getters return for every counted chain at every sample (the
getters are pinned to the checker library by the parity tests).

Tolerance of a sum of T chain terms: the device's terms equal numpy's bit for bit (same f64 operations in the same order), all
are non-negative, so any order of adding T of them is within (T - 1) 2^-53 relative of their exact sum, and so is numpy's:
|sum - ref| <= T 2^-52 ref, T = `terms`.  One term (one chain, one sample) has nothing to reorder: bit-equal."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_pair_scores import all_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def _planted(na, nb, edges, ka, kb, chains, seed=9, **kw):
    a, b = syn.planted_edges(na, nb, edges, ka, kb, seed=4)
    rp, cl = B.edge_to_adj((a, b), na + nb)
    m = B.BlockModel(syn.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rp, cl), n_chains=chains,
                     seed=seed, **kw)
    return m, np.diff(rp.astype(np.int64))


def _random_pairs(na, nb, count, seed=3):
    rs = np.random.default_rng(seed)
    return np.stack([rs.integers(0, na, count), na + rs.integers(0, nb, count)], axis=1)


def _sample_ref(m, deg, pairs, chains=None):
    """numpy's sample of the given chains (default: all) from the handle's getters"""
    chains = range(m.n_chains) if chains is None else chains
    return D.numpy_pair_scores([m.get_memberships(c) for c in chains], [m.get_m(c) for c in chains], [m.get_m_r(c) for c in chains],
                               deg, pairs)


def _close(got, ref, terms):
    return (np.abs(got - ref) <= terms * EPS * ref).all()


@pytest.mark.parametrize("k", [4, 8, 32, 64])
def test_one_chain_one_sample_is_numpy_bit_for_bit(k):
    na, nb = 900, 700
    m, deg = _planted(na, nb, 9000, k, k, 1)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    pairs = _random_pairs(na, nb, 5000)
    pairs[:3] = pairs[3:6]  # (pairs may repeat)
    m.pair_scores_set(pairs)
    m.pair_scores_accumulate()
    s, terms = m.pair_scores()
    ref = _sample_ref(m, deg, pairs)
    assert terms == 1 and (s == ref).all(), np.abs(s - ref).max()
    assert (s[:3] == s[3:6]).all() and s.max() > 0
    m.close()


def test_one_chain_wide_and_compat_are_numpy_bit_for_bit():
    """200 + 150 blocks: two-byte labels, m read from HBM; and the mt19937-compat mode (the call only reads state)."""
    name, na, nb, ne, ka, kb, eps, hubs, isolated = cases.CASE["wide_labels"]
    rowptr, col = cases.random_graph(5, na, nb, ne, ka, kb, hubs, isolated)
    deg = np.diff(rowptr.astype(np.int64))
    pairs = all_pairs(na, nb)[::7]
    m = B.BlockModel(O.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, eps, (rowptr, col), seed=2)
    m.shuffle_bisbm()
    m.run_sweeps(1)
    m.pair_scores_set(pairs)
    m.pair_scores_accumulate()
    s, terms = m.pair_scores()
    assert terms == 1 and (s == _sample_ref(m, deg, pairs)).all()
    m.close()
    c, deg = _planted(500, 400, 5000, 6, 5, 1, rng="mt19937-compat", gen_seed=10)
    c.shuffle_bisbm()
    c.run_sweeps(2)
    pairs = _random_pairs(500, 400, 3000)
    c.pair_scores_set(pairs)
    c.pair_scores_accumulate()
    s, terms = c.pair_scores()
    assert terms == 1 and (s == _sample_ref(c, deg, pairs)).all()
    c.close()


def test_sixteen_chains_five_samples():
    na, nb, chains = 900, 700, 16
    m, deg = _planted(na, nb, 9000, 8, 8, chains)
    m.shuffle_bisbm()
    pairs = _random_pairs(na, nb, 6000)
    m.pair_scores_set(pairs)
    ref = np.zeros(len(pairs))
    for _ in range(5):
        m.run_sweeps(3)
        ref += _sample_ref(m, deg, pairs)
        m.pair_scores_accumulate()
    s, terms = m.pair_scores()
    assert terms == 80
    assert _close(s, ref, terms), (np.abs(s - ref) / np.maximum(ref, 1e-300)).max() / EPS
    # reset keeps the pairs and zeroes sums and terms
    m.pair_scores_reset()
    s0, t0 = m.pair_scores()
    assert t0 == 0 and (s0 == 0).all()
    m.pair_scores_accumulate()
    s1, t1 = m.pair_scores()
    assert t1 == chains and _close(s1, _sample_ref(m, deg, pairs), t1)
    m.close()


def test_sum_rule_on_the_device():
    """All 18 x 14 pairs of southernWomen: per sample the scores add up to E x chains.  Every term carries at most two
    roundings, a pair's sum T - 1 more, numpy's sum over the P pairs P - 1 more: within (T + P + 1) 2^-52 of E x terms."""
    rowptr, col, na, nb = O.load_graph("southernWomen")
    E, chains = len(col) // 2, 8
    m = B.BlockModel(O.contiguous_labels(na, nb, 3, 3), syn.types_vector(na, nb), 6, 3, 3, 0.001, (rowptr, col), n_chains=chains, seed=5)
    m.shuffle_bisbm()
    pairs = all_pairs(na, nb)
    m.pair_scores_set(pairs)
    for sample in range(1, 4):
        m.run_sweeps(2)
        m.pair_scores_accumulate()
        s, terms = m.pair_scores()
        assert terms == sample * chains
        assert abs(s.sum() - E * terms) <= (terms + len(pairs) + 1) * EPS * E * terms, (s.sum(), E * terms)
    m.close()


def test_same_calls_same_bits():
    sums = []
    for _ in range(2):
        m, _deg = _planted(900, 700, 9000, 8, 8, 16)
        m.shuffle_bisbm()
        m.pair_scores_set(_random_pairs(900, 700, 6000))
        for _ in range(3):
            m.run_sweeps(2)
            m.pair_scores_accumulate()
        sums.append(m.pair_scores())
        m.close()
    assert sums[0][1] == sums[1][1] == 48
    assert (sums[0][0].view(np.uint64) == sums[1][0].view(np.uint64)).all()


def test_a_device_listed_twice_against_one_handle():
    chains = 16
    one, deg = _planted(600, 500, 6000, 5, 6, chains)
    two, _ = _planted(600, 500, 6000, 5, 6, chains, devices=[0, 0])
    pairs = _random_pairs(600, 500, 4000)
    for g in (one, two):
        g.shuffle_bisbm()
        g.pair_scores_set(pairs)
        for _ in range(2):
            g.run_sweeps(2)
            g.pair_scores_accumulate()
    (s1, t1), (s2, t2) = one.pair_scores(), two.pair_scores()
    assert t1 == t2 == 2 * chains
    assert _close(s2, s1, t1)
    two.pair_scores_reset()
    assert two.pair_scores()[1] == 0 and (two.pair_scores()[0] == 0).all()
    one.close()
    two.close()


def test_tempering_counts_the_cold_chains_only():
    chains, L = 8, 4
    m, deg = _planted(600, 500, 6000, 5, 5, chains)
    m.shuffle_bisbm()
    m.set_tempering([1.0, 1.4, 2.0, 3.0])
    pairs = _random_pairs(600, 500, 3000)
    m.pair_scores_set(pairs)
    ref = np.zeros(len(pairs))
    for sample in range(1, 5):
        m.tempering_run(3, 1)
        cold = np.flatnonzero(m.tempering_state()[0] == 0)
        assert len(cold) == chains // L
        ref += _sample_ref(m, deg, pairs, cold)
        m.pair_scores_accumulate()
        s, terms = m.pair_scores()
        assert terms == 2 * sample
        assert _close(s, ref, terms)
    # marginalize(tempering=..., score_pairs=...) samples the same way
    m2, _ = _planted(600, 500, 6000, 5, 5, chains)
    m2.shuffle_bisbm()
    B.marginalize(m2, 2, 3, 1, tempering=[1.0, 1.4, 2.0, 3.0], score_pairs=pairs)
    assert m2.pair_scores()[1] == 3 * chains // L
    m.close()
    m2.close()


def _mixed_shapes_model(**kw):
    rowptr, col, na, nb = O.load_graph("n_1000")
    g = B.BlockModel(O.contiguous_labels(na, nb, 6, 6), syn.types_vector(na, nb), 12, 6, 6, 1.0, (rowptr, col), n_chains=32, seed=4, **kw)
    g.shuffle_bisbm()
    g.run_sweeps(2)
    return g, np.diff(rowptr.astype(np.int64)), na, nb


def _merge_until_mixed(g):
    for _ in range(4):
        if g.mixed_shapes:
            break
        g.agg_merge(2, None, 10)
    assert g.mixed_shapes


def test_chains_of_different_shapes_pool_and_rungs_over_groups_are_refused():
    g, deg, na, nb = _mixed_shapes_model()
    pairs = _random_pairs(na, nb, 4000)
    g.pair_scores_set(pairs)
    g.pair_scores_accumulate()  # one shape still
    before = _sample_ref(g, deg, pairs)
    _merge_until_mixed(g)
    assert len({g.ka_kb(c) for c in range(g.n_chains)}) > 1
    g.run_sweeps(1)
    g.pair_scores_accumulate()
    s, terms = g.pair_scores()
    assert terms == 64
    assert _close(s, before + _sample_ref(g, deg, pairs), terms)
    g.close()
    # replica exchange set first, then the chains grouped by a one-argument merge: a group engine knows no rungs
    g, deg, na, nb = _mixed_shapes_model(devices=[0, 0])
    g.set_tempering([1.0, 1.3, 2.0, 3.5])
    g.pair_scores_set(pairs)
    g.pair_scores_accumulate()
    assert g.pair_scores()[1] == 8
    _merge_until_mixed(g)
    with pytest.raises(B.BisbmError) as e:
        g.pair_scores_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "grouped by shape" in str(e.value)
    assert g.pair_scores()[1] == 8
    g.close()


def test_sums_are_carried_across_merges_and_the_label_width():
    """128 + 129 blocks (two-byte labels) -> a two-argument merge to 128 + 128 (byte labels) -> a merge to 100 + 90: after every
    step `get` returns what was there plus the new sample."""
    rowptr, col = cases.random_graph(17, 400, 400, 6000, 128, 129)
    na = nb = 400
    deg = np.diff(rowptr.astype(np.int64))
    chains = 3
    g = B.BlockModel(O.contiguous_labels(na, nb, 128, 129), syn.types_vector(na, nb), 257, 128, 129, 1.0, (rowptr, col), n_chains=chains, seed=21)
    g.shuffle_bisbm()
    pairs = all_pairs(na, nb)[::11]
    g.pair_scores_set(pairs)
    total = np.zeros(len(pairs))
    for step, (da, db) in enumerate(((0, 0), (0, 1), (28, 38))):
        if da or db:
            g.agg_merge(da, db, 6)
        g.run_sweeps(1)
        total += _sample_ref(g, deg, pairs)
        g.pair_scores_accumulate()
        s, terms = g.pair_scores()
        assert terms == (step + 1) * chains and _close(s, total, terms), step
    assert (g.KA, g.KB) == (100, 90)
    g.close()


def test_refusals():
    m, deg = _planted(300, 200, 3000, 4, 4, 4)
    with pytest.raises(B.BisbmError) as e:  # no pairs
        m.pair_scores_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "pairs" in str(e.value)
    with pytest.raises(B.BisbmError) as e:
        m.pair_scores()
    assert e.value.code == B.BISBM_ERR_STATE
    pairs = _random_pairs(300, 200, 100)
    m.pair_scores_set(pairs)
    with pytest.raises(B.BisbmError) as e:  # no block state yet
        m.pair_scores_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "bisbm_init" in str(e.value)
    m.init_bisbm()
    m.pair_scores_accumulate()
    s, terms = m.pair_scores()
    for bad, index in (([[0, 300], [5, 5]], 1), ([[300, 301]], 0), ([[0, 300], [1, 301], [2, 500]], 2)):
        with pytest.raises(B.BisbmError) as e:
            m.pair_scores_set(np.array(bad))
        assert e.value.code == B.BISBM_ERR_INVALID_ARG and ("pair %d " % index) in str(e.value), str(e.value)
        s2, t2 = m.pair_scores()  # the earlier pairs and their sums are intact
        assert t2 == terms == 4 and (s2 == s).all()
    with pytest.raises(ValueError):
        m.pair_scores_set(np.zeros((3, 3), dtype=np.int64))
    m.pair_scores_set(np.zeros((0, 2), dtype=np.int64))  # frees everything
    with pytest.raises(B.BisbmError):
        m.pair_scores_accumulate()
    m.close()


def test_cli_scores_equal_the_python_driver(tmp_path):
    rowptr, col, na, nb = O.load_graph("n_1000")
    n, chains, seed = na + nb, 8, 5
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    pairs = _random_pairs(na, nb, 500)
    pin, pout = tmp_path / "pairs.txt", tmp_path / "scores.txt"
    pin.write_text("".join("%d %d\n" % (u, v) for u, v in pairs))
    sizes = [str(x) for x in np.bincount(O.contiguous_labels(na, nb, 4, 4))]
    common = [cli, "-e", el, "-y", str(na), str(nb), "-z", "4", "4", "-n", *sizes, "-r", "-d", str(seed), "--rng", "philox", "--chains", str(chains),
              "-b", str(10 * n), "-t", str(6 * n), "-f", str(2 * n), "--marginalize"]
    r = subprocess.run(common + ["--score_pairs", str(pin), str(pout)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    plain = subprocess.run(common, capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and plain.stdout == r.stdout and len(r.stdout.split()) == n  # stdout is unchanged
    rows = [line.split() for line in pout.read_text().splitlines()]
    assert [(int(x[0]), int(x[1])) for x in rows] == [tuple(p) for p in pairs.tolist()]
    m = B.BlockModel(O.contiguous_labels(na, nb, 4, 4), syn.types_vector(na, nb), 8, 4, 4, 1.0, (rowptr, col), n_chains=chains, seed=seed)
    m.shuffle_bisbm()
    B.marginalize(m, 10, 3, 2, score_pairs=pairs)
    s, terms = m.pair_scores()
    assert terms == 3 * chains
    assert (np.array([float(x[2]) for x in rows]) == s / terms).all()
    m.close()
    # --reorder: the pairs are given, and printed, in the file's own ids; the engine scores the renumbered nodes -- another chain,
    # so only the sum rule is checked: all pairs add up to E
    allp = all_pairs(na, nb)[::50]
    pin.write_text("".join("%d %d\n" % (u, v) for u, v in allp))
    r = subprocess.run(common + ["--reorder", "--score_pairs", str(pin), str(pout)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rows = [line.split() for line in pout.read_text().splitlines()]
    assert [(int(x[0]), int(x[1])) for x in rows] == [tuple(p) for p in allp.tolist()]
    lo = B.locality_order(rowptr, col, na, nb)
    rp2, cl2 = lo.apply(rowptr, col)
    m = B.BlockModel(lo.to_new(O.contiguous_labels(na, nb, 4, 4)), syn.types_vector(na, nb), 8, 4, 4, 1.0, (rp2, cl2), n_chains=chains, seed=seed)
    m.shuffle_bisbm()
    B.marginalize(m, 10, 3, 2, score_pairs=lo.new_id[allp])
    s, terms = m.pair_scores()
    assert (np.array([float(x[2]) for x in rows]) == s / terms).all()
    m.close()


def test_example_runs():
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "link_prediction.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "terms per pair: 1280" in r.stdout, r.stdout + r.stderr


def _auc(score, positive):
    from scipy.stats import rankdata
    r = rankdata(score)
    n1 = int(positive.sum())
    n0 = len(positive) - n1
    return (r[positive].sum() - n1 * (n1 + 1) / 2) / (n1 * n0)


def test_held_out_edges_are_ranked_above_non_edges():
    """It means what it says.  planted_edges(2000, 2000, 40000, 8, 8, seed=4); a tenth of the edges held out, as many random
    non-edges as negatives; 64 chains from shuffle_bisbm on the training graph, burn-in, samples through
    marginalize(score_pairs=...).  The bar comes from two numbers computed here with numpy from the PLANTED labels on the
    training graph, neither from the code under test: the AUC of the planted partition's scores (0.868 on this input) and that
    of the degree-only score d(u) d(v), the one-block model (0.510).  The sampler must reach the midpoint: half the gap is the
    margin for chains that sit in a mode with merged blocks; a score that ignored the partition, or read another chain's tables,
    lands at the degree-only figure.  (Six chains of the checker library, rehearsed on the CPU: 0.81 - 0.86 each, 0.865 pooled.)"""
    from test_pair_scores import block_state
    na = nb = 2000
    a, b = syn.planted_edges(na, nb, 40000, 8, 8, seed=4)
    E = len(a)
    rng = np.random.default_rng(7)
    held = rng.choice(E, E // 10, replace=False)
    keep = np.ones(E, dtype=bool)
    keep[held] = False
    edges = set(zip(a.tolist(), b.tolist()))
    neg = []
    while len(neg) < len(held):
        u, v = int(rng.integers(0, na)), int(na + rng.integers(0, nb))
        if (u, v) not in edges:
            neg.append((u, v))
    pairs = np.concatenate([np.stack([a[held], b[held]], axis=1).astype(np.int64), np.array(neg)])
    positive = np.arange(len(pairs)) < len(held)
    ta, tb = a[keep], b[keep]
    planted = syn.contiguous_labels(na, nb, 8, 8)
    m_pl, m_r_pl, deg = block_state(ta, tb, planted, 16)
    auc_planted = _auc(D.numpy_pair_scores([planted], [m_pl], [m_r_pl], deg, pairs), positive)
    auc_degree = _auc(deg[pairs[:, 0]].astype(np.float64) * deg[pairs[:, 1]], positive)
    assert auc_planted > 0.8 and auc_degree < 0.6, (auc_planted, auc_degree)
    bar = 0.5 * (auc_planted + auc_degree)

    rp, cl = B.edge_to_adj((ta, tb), na + nb)
    m = B.BlockModel(planted, syn.types_vector(na, nb), 16, 8, 8, 1.0, (rp, cl), n_chains=64, seed=11)
    m.shuffle_bisbm()
    B.marginalize(m, 200, 10, 5, score_pairs=pairs)
    s, terms = m.pair_scores()
    assert terms == 640
    auc = _auc(s / terms, positive)
    print("held-out AUC: sampler %.4f, planted partition %.4f, degree only %.4f, bar %.4f" % (auc, auc_planted, auc_degree, bar))
    assert auc >= bar, "held-out AUC %.4f below the bar %.4f (planted partition %.4f, degree only %.4f)" % (auc, bar, auc_planted, auc_degree)
    m.close()
