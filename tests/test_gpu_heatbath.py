"""GPU tests of the heat-bath sweeps and the greedy polishing (include/bisbm.h, "Heat-bath sweeps and greedy polishing").

The replay tests walk the last chain of a handle on the host: the visit order from the oracle's orc_philox_visit, the uniform
from the oracle's Philox with purpose 9, every step's dS and P rows from a one-chain helper handle that is set to the replay's
current labels (bisbm_conditionals_accumulate with KEEP_LAST: the device's own rows, which the kernel's rows must equal bit for
bit), and the choice from distributed.numpy_heatbath_choice (tests/test_heatbath.py ties that to the literal loop).  Labels,
move counts and the block state are integers, the running sum of dS is compared on bit patterns."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_gpu_pair_scores import _merge_until_mixed, _mixed_shapes_model
from test_tempering import philox, u53

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu

SEED = 21
FIRST_ID = 5
INF = float("inf")


@pytest.fixture(autouse=True)
def _every_launch_keeps_its_own_sum(monkeypatch):
    """the MH sweeps of these tests keep the sum of their own dS values (tests/test_gpu_scale.py explains): a check of that sum
    against the description length would otherwise hold by construction"""
    monkeypatch.setenv("BISBM_KEEP_SUM", "1")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


_GRAPHS = {}


def _case(name):
    if name not in _GRAPHS:
        _, na, nb, ne, ka, kb, eps, hubs, iso = next(d[name] for d in (cases.HEATBATH_CASES, cases.HELD_WIDE_CASES, cases.CASE) if name in d)
        _GRAPHS[name] = (cases.random_graph(11, na, nb, ne, ka, kb, hubs, iso), na, nb, ka, kb, eps)
    return _GRAPHS[name]


def _model(name, chains, seed=SEED, labels=None, **kw):
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    lab = O.contiguous_labels(na, nb, ka, kb) if labels is None else labels
    return B.BlockModel(lab, syn.types_vector(na, nb), ka + kb, ka, kb, eps, (rowptr, col), n_chains=chains, seed=seed, **kw)


def _make_alone(m, na, ka, kb, chains):
    """every chain: the other nodes of the blocks of node 1 and node na + 1 move to the next block of their type (where the
    type has one), then the block state is rebuilt -- what test_gpu_conditionals._make_alone does on its graph"""
    for c in chains:
        lab = m.get_memberships(c).astype(np.int64)
        for v, lo, k in ((1, 0, ka), (na + 1, ka, kb)):
            if k < 2:
                continue
            r = lab[v]
            others = np.flatnonzero(lab == r)
            lab[others[others != v]] = lo + (r - lo + 1) % k
        m.set_memberships(lab.astype(np.uint32), chain=c)
    m.init_bisbm()


def _state_from_labels(rowptr, col, lab, K, max_degree):
    """m (K x K, symmetric), m_r, n_r, eta (K x (max_degree + 1)) of init_bisbm, in numpy"""
    lab = np.asarray(lab, dtype=np.int64)
    deg = np.diff(rowptr.astype(np.int64))
    src = np.repeat(np.arange(len(lab)), deg)
    m = np.zeros((K, K), dtype=np.int64)
    np.add.at(m, (lab[src], lab[col.astype(np.int64)]), 1)
    eta = np.zeros((K, max_degree + 1), dtype=np.int64)
    np.add.at(eta, (lab, deg), 1)
    return m, m.sum(axis=1), np.bincount(lab, minlength=K), eta


def _assert_state_is_a_rebuild(m, rowptr, col, c):
    ka, kb = m.ka_kb(c)
    want = _state_from_labels(rowptr, col, m.get_memberships(c), ka + kb, m.max_degree)
    got = (m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c))
    for name, g, w in zip(("m", "m_r", "n_r", "eta"), got, want):
        assert (g.astype(np.int64) == w).all(), (c, name)


# ------------------------------------------------------------------------------------------------------- 1. exact replay
def _replay(name, sweeps, beta, after_polish=False, alone=True, labels=None):
    """alone: a node of each type is made the only one of its block first (on a graph of 2 + 2 blocks that would turn the sizes
    into (1, n - 1) and take the blocks out of their log_q tier); labels: every chain starts from these through init_bisbm, with
    no sweep run before.  Returns what the callers assert their edge on: per free step (v, deg, the number of distinct blocks
    among the neighbours, k_own, r, s, whether the device's P row holds an exact 0), r and s within the type, and the replayed
    chain's (m_r, n_r) before and after the device call."""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, chains, greedy = na + nb, 3, beta == INF
    m = _model(name, chains, first_chain_id=FIRST_ID, labels=labels)
    if labels is None:
        m.shuffle_bisbm()
        m.run_sweeps(3)
    else:
        m.init_bisbm()
    if alone:
        _make_alone(m, na, ka, kb, range(chains))
    # (three MH sweeps so far, or none: the chain's sweep index)
    c, gid, sweep0 = chains - 1, FIRST_ID + chains - 1, 3 if labels is None else 0
    if after_polish:  # a polish that stops early first: the counter has advanced by the sweeps it ran, and by no more
        ran_before = m.polish(100)[1]
        assert (ran_before < 100).all() and len(set(ran_before.tolist())) > 1  # (the chains' counters now differ)
        sweep0 += int(ran_before[c])
    lab = m.get_memberships(c).astype(np.int64)
    cum, S0 = m.get_entropy()[c], m.entropy()[c]
    before = m.get_m_r(c).copy(), m.get_n_r(c).copy()
    rp, steps = rowptr.astype(np.int64), []
    helper = _model(name, 1, labels=lab.astype(np.uint32))
    helper.conditionals_set(None, 1.0 if greedy else beta, keep_last=True)

    def sync():
        helper.set_memberships(lab.astype(np.uint32))
        helper.init_bisbm()
        helper.conditionals_accumulate()
    sync()
    if greedy:
        moved_gpu, sweeps_gpu = m.polish(sweeps)
    else:
        moved_gpu, sweeps_gpu = m.heatbath_sweeps(sweeps, beta), None
    L = O.lib()
    for v, k in ((1, ka), (na + 1, kb)):  # (the set-up: a node alone in its block in every type that has two blocks)
        assert k < 2 or after_polish or not alone or int((lab == lab[v]).sum()) == 1
    moved, total, free_seen, ran = 0, 0.0, 0, 0
    for sw in range(sweeps):
        order = [int(L.orc_philox_visit(SEED, gid, sweep0 + sw, na, nb, i)) for i in range(n)]
        assert sorted(order) == list(range(n)) and all(v < na for v in order[:na])  # once each, type a before type b
        moved_before = moved
        for pos, v in enumerate(order):
            k_own, lo = (ka, 0) if v < na else (kb, ka)
            r = int(lab[v]) - lo
            free = k_own > 1 and int((lab == lab[v]).sum()) > 1
            free_seen += free
            dS, P = (x[0] for x in helper.conditionals_last(v))
            o = philox(SEED, gid, B.PHILOX_PURPOSE_HEATBATH, (sweep0 + sw) * n + pos)
            s = D.numpy_heatbath_choice(dS, P, r, free, u53(o[0], o[1]), greedy)
            if free:
                steps.append((v, int(rp[v + 1] - rp[v]), len(set(lab[col[rp[v]:rp[v + 1]]].tolist())), k_own, r, s,
                              bool((P[:k_own] == 0.0).any())))
            if s != r:
                lab[v] = lo + s
                cum = cum + dS[s]
                total = total + dS[s]
                moved += 1
                sync()
        ran += 1
        if greedy and moved == moved_before:
            break
    assert free_seen > 0
    assert moved > 0, "the replay moved nothing: the case checks nothing"
    assert (m.get_memberships(c) == lab).all()
    assert int(moved_gpu[c]) == moved
    if greedy:
        assert int(sweeps_gpu[c]) == ran
    acc, sw_counts = m.last_counts()
    assert int(acc[c]) == moved and int(sw_counts[c]) == ran
    for got, want in ((m.get_m(c), helper.get_m(0)), (m.get_m_r(c), helper.get_m_r(0)), (m.get_n_r(c), helper.get_n_r(0)),
                      (m.get_eta_rk_(c), helper.get_eta_rk_(0))):
        assert (got == want).all()
    assert _bits(m.get_entropy()[c]) == _bits(cum)
    S1 = m.entropy()[c]
    print("%s beta %g: %d moves in %d sweep(s), sum dS %.6f, S %.6f -> %.6f" % (name, beta, moved, ran, total, S0, S1))
    assert abs((S1 - S0) - total) <= 1e-9 * abs(S0)
    for other in range(chains - 1):  # (the other chains ran too, and are consistent)
        _assert_state_is_a_rebuild(m, rowptr, col, other)
    after = m.get_m_r(c).copy(), m.get_n_r(c).copy()
    m.close()
    helper.close()
    return {"steps": steps, "before": before, "after": after}


@pytest.mark.parametrize("name,sweeps", [("tiny", 2), ("ka1", 2), ("hubs_isolated", 2), ("huge_hub", 1), ("wideK", 1)])
def test_heat_bath_sweeps_are_the_host_replay(name, sweeps):
    _replay(name, sweeps, 1.0)


def test_greedy_sweeps_are_the_host_replay():
    _replay("hubs_isolated", 2, INF)


def test_heat_bath_sweeps_after_a_polish_that_stopped_early_are_the_host_replay():
    _replay("hubs_isolated", 1, 1.0, after_polish=True)


# ------------------------------------------------------------------------------- 1a. the replay through the log_q tiers
# log_q<true> looks at the log n it is handed only past the q table (n > 10^4); the kernel hands it over per evaluation -- the
# target after and before the move, then the r side by lane parity -- so only blocks outside the table tell a mixed-up triple.
def _assert_every_block_in_its_tier(rec, name):
    for when in ("before", "after"):
        got = cases.log_q_tiers(*rec[when])
        assert (got == cases.CASE_TIERS[name]).all(), (name, when, cases.tier_counts(*rec[when]))


def _reassign_every_fifth(lab, na, ka, kb):
    """about 20 % of the nodes get a label drawn uniformly within their type (seeded)"""
    lab = np.asarray(lab).astype(np.int64)
    rng = np.random.default_rng(12)
    again = np.flatnonzero(rng.random(len(lab)) < 0.2)
    lab[again] = np.where(again < na, rng.integers(0, ka, len(again)), ka + rng.integers(0, kb, len(again)))
    return lab.astype(np.uint32)


@pytest.mark.parametrize("name", ["dense_low_tier", "mid_tier_low", "closed2_tier", "mid_tier"])
def test_heat_bath_sweep_through_a_log_q_tier_is_the_host_replay(name):
    _assert_every_block_in_its_tier(_replay(name, 1, 1.0, alone=False), name)


def test_heat_bath_sweep_through_the_literal_log_q_tier_is_the_host_replay():
    """big_m_r plants 2 + 3 groups: group i of type a goes with group i of type b, so the third group of type b receives the
    uniform fifth of the edges only, some 4000 ends, and any labelling near the planted one has a block on the q table -- which
    is where the three MH sweeps of the usual start take the chain.  The start here keeps all five blocks past the table for
    the one sweep: the first group of type b split evenly over the first and the third block (about 14 000 ends each), the
    other two groups together in the second."""
    name = "big_m_r"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    b = np.arange(nb)
    lab = O.contiguous_labels(na, nb, ka, kb)
    lab[na:] = ka + np.where(b < nb // 3, 2 * (b % 2), 1)
    rec = _replay(name, 1, 1.0, alone=False, labels=lab)
    _assert_every_block_in_its_tier(rec, name)
    assert np.median([deg for _, deg, *_ in rec["steps"]]) > 256  # (rows of about 400 neighbours: the tail loop past the LDS labels)


def test_greedy_sweep_through_a_log_q_tier_is_the_host_replay():
    """(from the planted labels with every fifth node reassigned: a greedy sweep from the shuffled start empties two of the
    four blocks far enough to leave the tier)"""
    name = "mid_tier_low"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    lab = _reassign_every_fifth(O.contiguous_labels(na, nb, ka, kb), na, ka, kb)
    _assert_every_block_in_its_tier(_replay(name, 1, INF, alone=False, labels=lab), name)


MIXED_SIZES = (700, 1900, 3500)


def test_heat_bath_sweep_with_three_tiers_in_one_evaluation_is_the_host_replay():
    """blocks of 700, 1900 and 3500 nodes per type at mean degree 8: m_r about 8000 / 15000 / 26000, the q table, log_q_closed2
    and log_q_closed side by side in the lanes of one evaluation.  From the planted labels with every fifth node reassigned
    uniformly within its type (the planted labelling itself would leave a sweep at beta = 1 next to nothing to move)."""
    name, k = "mixed_tiers", len(MIXED_SIZES)
    if name not in _GRAPHS:
        graph, na, nb = cases.unequal_groups_graph(11, MIXED_SIZES, MIXED_SIZES, 8)
        _GRAPHS[name] = (graph, na, nb, k, k, 1.0)
    _, na, nb, ka, kb, _ = _GRAPHS[name]
    lab = _reassign_every_fifth(O.labels_from_sizes(MIXED_SIZES + MIXED_SIZES), na, ka, kb)
    rec = _replay(name, 1, 1.0, alone=False, labels=lab)
    for when in ("before", "after"):
        counts = cases.tier_counts(*rec[when])
        assert min(counts["table"], counts["closed2"], counts["closed"]) >= 1, (when, counts, rec[when])


# ------------------------------------------------------------------- 1b. lane chunks, list lengths, row lengths, eta in HBM
def _moves(rec, type_b, na):
    return [(r, s) for v, _, _, _, r, s, _ in rec["steps"] if (v >= na) == type_b and s != r]


@pytest.mark.parametrize("beta,sweeps", [(1.0, 1), (INF, 1)])
def test_64_and_65_targets_are_the_host_replay(beta, sweeps):
    """64 blocks of type a: exactly one full chunk of target lanes; 65 of type b: a second chunk that holds one target"""
    name = "hb_k64_k65"
    na = _case(name)[1]
    rec = _replay(name, sweeps, beta)
    assert any(63 in rs for rs in _moves(rec, False, na)), "no move into or out of the last block of type a"
    assert any(64 in rs for rs in _moves(rec, True, na)), "no move into or out of the last block of type b"


@pytest.mark.parametrize("beta", [1.0, INF])
def test_130_targets_are_the_host_replay(beta):
    """three chunks of target lanes, the last one two wide"""
    name = "hb_k130"
    na = _case(name)[1]
    rec = _replay(name, 1, beta)
    assert any(s >= 128 for r, s in _moves(rec, False, na)), "no move into the third chunk"


def _eta_is_outside_the_lds(name):
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    return 4 * (ka + kb) * (int(np.diff(rowptr.astype(np.int64)).max()) + 1) > 40 * 1024


def test_a_list_longer_than_one_wave_is_the_host_replay():
    """100 blocks of type b and a type-a hub with some 610 neighbours: its list of non-zero (t, k_t) runs into a second chunk of
    64 lanes; six type-b rows of about 400 neighbours; eta in HBM"""
    name = "hb_long_list"
    assert _eta_is_outside_the_lds(name)
    rec = _replay(name, 1, 1.0, alone=False)
    assert max(blocks for _, _, blocks, *_ in rec["steps"]) > 64
    hub = [(deg, blocks) for v, deg, blocks, *_ in rec["steps"] if v == 0]  # (a step is recorded only when the node is free)
    assert len(hub) == 1 and hub[0][0] > 600 and hub[0][1] > 64, hub


@pytest.mark.parametrize("beta,sweeps", [(1.0, 2), (INF, 1)])
def test_eta_in_hbm_is_the_host_replay(beta, sweeps):
    """10 + 10 blocks and a hub of degree 600: eta stays in HBM, where lane 0 rewrites the entries of r and s with atomics and
    every lane reads them back with plain loads in later steps -- with so few rows, soon after"""
    name = "hb_eta_in_hbm"
    assert _eta_is_outside_the_lds(name)
    _replay(name, sweeps, beta)


DEGREES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)


def test_rows_of_64_and_65_neighbours_and_a_class_of_64_and_65_nodes_are_the_host_replay():
    """rows that end at, one past and far past the 64 labels the chunk header parks in LDS (and at 128 and 256, the trip counts
    of the tail loop); 64 nodes of type a: one chunk of exactly 64 positions; 65 of type b: a chunk of 64 and a chunk of one"""
    name, na, nb, ka, kb = "hb_degrees", 64, 65, 3, 4
    if name not in _GRAPHS:
        a, b = [], []
        for i in range(na):
            for j in range(DEGREES[i] if i < len(DEGREES) else 3):
                a.append(i)
                b.append(na + ((11 * i + j) if i < len(DEGREES) else (7 * i + 5 * j)) % nb)
        _GRAPHS[name] = (O.edge_to_csr(np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64), na + nb), na, nb, ka, kb, 1.0)
    deg = np.diff(_GRAPHS[name][0][0].astype(np.int64))
    assert tuple(deg[:len(DEGREES)]) == DEGREES and (deg[len(DEGREES):na] == 3).all()
    assert deg[na:].min() == 21 and deg[na:].max() == 24  # (multi-edges are kept)
    rec = _replay(name, 2, 1.0, alone=False)
    seen = {d for v, d, *_ in rec["steps"] if v < na}
    assert set(DEGREES) <= seen, sorted(set(DEGREES) - seen)


# ------------------------------------------------------------------------------------------ 1c. the choice at extreme beta
def test_exact_zeros_in_P_at_a_large_beta_are_the_host_replay():
    """beta (dS - dS_min) > 700 makes w an exact 0: the first s with u < C_s, else the largest s with P_s > 0"""
    rec = _replay("hubs_isolated", 1, 200.0)
    assert any(zero for *_, zero in rec["steps"])


def test_a_nearly_flat_P_at_a_small_beta_is_the_host_replay():
    rec = _replay("hubs_isolated", 1, 1e-3)
    assert 2 * sum(s != r for _, _, _, _, r, s, _ in rec["steps"]) >= len(rec["steps"])


# ------------------------------------------------------------------------------------------- 2. stationary distribution
@pytest.mark.parametrize("beta", [1.0, 5.0 / 3.0])
def test_heat_bath_chains_sample_exp_minus_beta_S(beta):
    """32768 chains on the enumerable 6 + 6 graph, one sample each after 100 heat-bath sweeps from a randomised start, against
    exp(-beta (S - S_min)) over the 3844 admissible states (the set-up of test_gpu_scale.py::test_gpu_chains_sample_exp_minus_S;
    a state with an empty block makes chi_square raise)"""
    rowptr, col = cases.enumerable_graph()
    na, nb = cases.ENUM_NA, cases.ENUM_NB
    chains = 32768
    g = B.BlockModel(O.contiguous_labels(na, nb, 2, 2), syn.types_vector(na, nb), 4, 2, 2, cases.ENUM_EPS, (rowptr, col),
                     n_chains=chains, rng="philox", seed=4242)
    g.shuffle_bisbm()
    g.heatbath_sweeps(100, beta)
    codes = np.array([cases.state_code(g.get_memberships(c)) for c in range(chains)])
    g.close()
    states, _, S = cases.enumerable_states()
    target = np.exp(-beta * (S - S.min()))
    stat, dof, p = cases.chi_square(codes, states, target / target.sum())
    flat = np.exp(-beta * (S - S.min()) / 1.25)
    p_flat = cases.chi_square(codes, states, flat / flat.sum())[2]
    print("heat bath, beta = %g: chi2 = %.1f on %d dof, p = %.3g; flattened target p = %.3g" % (beta, stat, dof, p, p_flat))
    assert p > 1e-3, (stat, dof, p)
    assert p_flat < 1e-6


# ---------------------------------------------------------------------------------------------------------- 3. polish
def test_polish_reaches_a_local_minimum_and_a_second_polish_moves_nothing():
    name, chains = "hubs_isolated", 4
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    m = _model(name, chains)
    m.shuffle_bisbm()
    m.run_sweeps(5)
    before = m.entropy()
    moved, sweeps = m.polish(100)
    after = m.entropy()
    print("polish: moved %s in %s sweeps, S %s -> %s" % (moved, sweeps, before, after))
    assert (sweeps < 100).all()  # every chain settled within the cap
    assert (after <= before).all() and (after[moved > 0] < before[moved > 0]).all()
    m.conditionals_set(None, keep_last=True)
    m.conditionals_accumulate()
    labels = [m.get_memberships(c) for c in range(chains)]
    n_r = [m.get_n_r(c) for c in range(chains)]
    for v in range(na + nb):
        k_own = ka if v < na else kb
        dS = m.conditionals_last(v)[0]
        for c in range(chains):
            if k_own > 1 and n_r[c][labels[c][v]] > 1:
                assert not (dS[c, :k_own] < 0).any(), (c, v, dS[c])
    again, one = m.polish(100)
    assert (again == 0).all() and (one == 1).all()
    for c in range(chains):
        assert (m.get_memberships(c) == labels[c]).all()
    m.close()


# --------------------------------------------------------------------------------- 4. same bits however it is launched
def _run(m):
    m.shuffle_bisbm()
    moved = m.heatbath_sweeps(2, 1.0)
    return [m.get_memberships(c) for c in range(m.n_chains)], moved, m.get_entropy()


def test_one_handle_device_entries_and_split_handles_give_the_same_bits():
    name = "hubs_isolated"
    one = _model(name, 6)
    labels, moved, cum = _run(one)
    assert (moved > 0).all()
    for entries in (2, 3):
        many = _model(name, 6, devices=[0] * entries)
        l2, m2, c2 = _run(many)
        assert all((a == b).all() for a, b in zip(labels, l2)) and (moved == m2).all() and (_bits(cum) == _bits(c2)).all(), entries
        many.close()
    for first in (0, 3):
        part = _model(name, 3, first_chain_id=first)
        l2, m2, c2 = _run(part)
        assert all((a == b).all() for a, b in zip(labels[first:first + 3], l2)), first
        assert (moved[first:first + 3] == m2).all() and (_bits(cum[first:first + 3]) == _bits(c2)).all(), first
        part.close()
    one.close()


def test_chains_grouped_by_shape_are_served():
    g, deg, na, nb = _mixed_shapes_model()
    _merge_until_mixed(g)
    rowptr, col, _, _ = O.load_graph("n_1000")
    before = [g.get_memberships(c) for c in range(g.n_chains)]
    moved = g.heatbath_sweeps(1, 1.0)
    assert len({g.ka_kb(c) for c in range(g.n_chains)}) > 1 and (moved > 0).all()
    for c in range(g.n_chains):
        assert int((g.get_memberships(c) != before[c]).sum()) <= int(moved[c])
        _assert_state_is_a_rebuild(g, rowptr, col, c)
    moved, sweeps = g.polish(50)
    assert (sweeps >= 1).all() and (sweeps <= 50).all()
    for c in range(g.n_chains):
        _assert_state_is_a_rebuild(g, rowptr, col, c)
    g.close()


def test_eta_outside_the_lds():
    """K = 16 + 13 with a hub of degree 600: eta (29 x 601 words) stays in HBM (the kernel's other instantiation)"""
    name, chains = "k16_eta_in_hbm", 2
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    assert 4 * (ka + kb) * (int(np.diff(rowptr.astype(np.int64)).max()) + 1) > 40 * 1024
    m = _model(name, chains)
    m.shuffle_bisbm()
    S0, cum0 = m.entropy(), m.get_entropy()
    moved = m.heatbath_sweeps(1, 1.0)
    moved2, sweeps = m.polish(2)
    S1, cum1 = m.entropy(), m.get_entropy()
    assert (moved > 0).all() and (moved2 > 0).all()
    for c in range(chains):
        _assert_state_is_a_rebuild(m, rowptr, col, c)
    assert (np.abs((S1 - S0) - (cum1 - cum0)) <= 1e-9 * np.abs(S0)).all(), (S1 - S0, cum1 - cum0)
    m.close()


# ---------------------------------------------------------------------------------------------------- 5. state hygiene
def test_mh_sweeps_after_heat_bath_calls_are_those_of_a_fresh_handle_with_the_same_counter():
    """set_memberships and init_bisbm leave a chain's sweep counter alone, so a fresh one-chain handle with the chain's global id
    that runs as many sweeps as the chain has run in all -- 2 MH, 2 heat-bath and what its polish ran before it stopped --, then
    takes the chain's labels, has the same labels and the same counter: its next 2 MH sweeps must be the chain's, label for label
    and count for count.  A handle whose counter is one short must not."""
    name, chains = "hubs_isolated", 4
    m = _model(name, chains)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    assert (m.heatbath_sweeps(2, 1.0) > 0).all()
    ran = m.polish(100)[1]
    assert (ran < 100).all() and len(set(ran.tolist())) > 1  # (stopped early, and not all after the same number of sweeps)
    labels = [m.get_memberships(c) for c in range(chains)]
    m.run_sweeps(2)
    accepted = m.last_counts()[0]
    for c in range(chains):
        for short in ((0, 1) if c == 0 else (0,)):
            f = _model(name, 1, labels=labels[c], first_chain_id=c)
            f.init_bisbm()
            f.run_sweeps(4 + int(ran[c]) - short)
            f.set_memberships(labels[c])
            f.init_bisbm()
            f.run_sweeps(2)
            same = bool((f.get_memberships(0) == m.get_memberships(c)).all()) and int(f.last_counts()[0][0]) == int(accepted[c])
            assert same == (short == 0), (c, short)
            f.close()
    m.close()


def test_the_production_sum_of_dS_across_a_heat_bath_call(monkeypatch):
    """without BISBM_KEEP_SUM (what users run): a production MH call at T = 1 advances the running sum by the change of the block
    entropy and keeps the value for the next call; a heat-bath call in between adds its own dS and must make that kept value
    stale, or its moves would be counted twice"""
    monkeypatch.delenv("BISBM_KEEP_SUM")
    name, chains = "hubs_isolated", 4
    m = _model(name, chains)
    m.shuffle_bisbm()
    S0, cum0 = m.entropy(), m.get_entropy()
    m.run_sweeps(2)
    S1, cum1 = m.entropy(), m.get_entropy()
    assert (m.heatbath_sweeps(1, 1.0) > 0).all()
    S2, cum2 = m.entropy(), m.get_entropy()
    m.run_sweeps(2)
    S3, cum3 = m.entropy(), m.get_entropy()
    assert (np.abs(S2 - S1) > 1e-6 * np.abs(S0)).all()  # (the heat-bath call moved the description length by far more than the bound)
    for (Sa, ca), (Sb, cb) in (((S0, cum0), (S1, cum1)), ((S1, cum1), (S2, cum2)), ((S2, cum2), (S3, cum3)), ((S0, cum0), (S3, cum3))):
        assert (np.abs((Sb - Sa) - (cb - ca)) <= 1e-9 * np.abs(S0)).all(), (Sb - Sa, cb - ca)
    m.close()


def test_the_sums_of_the_analysis_calls_and_the_state_after_mh_sweeps():
    """a heat-bath call leaves the sums of the analysis calls alone, and MH sweeps after it leave a block state that is a rebuild
    of the labels and a sum of dS that tracks the description length"""
    name, chains = "hubs_isolated", 4
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    m = _model(name, chains)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    q = np.array([0, na + 3, 17, na - 1, na + nb - 1], dtype=np.uint32)
    pairs = np.array([[0, na], [5, na + 7], [na - 1, na + nb - 1]], dtype=np.uint32)
    m.conditionals_set(q, keep_last=True)
    m.conditionals_accumulate()
    m.pair_scores_set(pairs)
    m.pair_scores_accumulate()
    m.marginals_reset()
    m.marginals_accumulate(None)

    def sums():
        st = m.conditionals_stats()
        rows = [m.conditionals_last(i) for i in range(len(q))]
        return st, rows, m.pair_scores(), m.marginals_get().copy()
    a = sums()
    S0, cum0 = m.entropy(), m.get_entropy()
    m.heatbath_sweeps(2, 1.0)
    m.polish(3)
    b = sums()
    for key in ("stay", "entropy", "margin"):
        assert (_bits(a[0][key]) == _bits(b[0][key])).all()
    assert (a[0]["free"] == b[0]["free"]).all() and a[0]["terms"] == b[0]["terms"]
    for (d0, p0), (d1, p1) in zip(a[1], b[1]):
        assert (_bits(d0) == _bits(d1)).all() and (_bits(p0) == _bits(p1)).all()
    assert (_bits(a[2][0]) == _bits(b[2][0])).all() and a[2][1] == b[2][1]
    assert (a[3] == b[3]).all()
    m.run_sweeps(2)
    S1, cum1 = m.entropy(), m.get_entropy()
    for c in range(chains):
        _assert_state_is_a_rebuild(m, rowptr, col, c)
    assert (np.abs((S1 - S0) - (cum1 - cum0)) <= 1e-9 * np.abs(S0)).all(), (S1 - S0, cum1 - cum0)
    m.close()


# ------------------------------------------------------------------------------------------------------- 6. refusals
def _refused(call, code):
    with pytest.raises(B.BisbmError) as e:
        call()
    assert e.value.code == code, str(e.value)
    assert len(str(e.value).split(": ", 1)[1]) > 0  # (bisbm_last_error is not empty)
    return str(e.value)


def test_refusals():
    name = "tiny"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    m = _model(name, 4)
    assert "bisbm_init" in _refused(lambda: m.heatbath_sweeps(1), B.BISBM_ERR_STATE)  # (labels set, block state not built)
    m.shuffle_bisbm()
    state = [m.get_memberships(c) for c in range(4)], m.get_entropy(), m.last_counts()
    for beta in (float("nan"), 0.0, -1.0, -INF):
        assert "beta" in _refused(lambda: m.heatbath_sweeps(1, beta), B.BISBM_ERR_INVALID_ARG)
    m.set_tempering([1.0, 2.0])
    assert "replica exchange" in _refused(lambda: m.heatbath_sweeps(1), B.BISBM_ERR_STATE)
    _refused(lambda: m.polish(3), B.BISBM_ERR_STATE)
    m.set_tempering(None)
    after = [m.get_memberships(c) for c in range(4)], m.get_entropy(), m.last_counts()
    assert all((x == y).all() for x, y in zip(state[0], after[0])) and (_bits(state[1]) == _bits(after[1])).all()
    assert all((x == y).all() for x, y in zip(state[2], after[2]))
    # sweeps = 0: a no-op that returns OK
    assert (m.heatbath_sweeps(0) == 0).all()
    assert all((x == y).all() for x, y in zip(state[0], [m.get_memberships(c) for c in range(4)]))
    assert all((x == y).all() for x, y in zip(state[2], m.last_counts()))
    assert B.lib().bisbm_heatbath_run(m._h, 1, 1.0, 0, None, None) == B.BISBM_OK  # (both outputs may be NULL)
    m.close()
    compat = _model(name, 2, rng="mt19937-compat")
    compat.shuffle_bisbm()
    assert "MT19937" in _refused(lambda: compat.heatbath_sweeps(1), B.BISBM_ERR_UNSUPPORTED)
    compat.close()
    wide = _model("wide_labels", 2)
    wide.init_bisbm()
    assert "byte labels" in _refused(lambda: wide.heatbath_sweeps(1), B.BISBM_ERR_UNSUPPORTED)
    wide.close()


# --------------------------------------------------------------------------- 7. marginalize, the command line, the example
def test_marginalize_and_the_cli_reproduce_the_python_calls():
    rowptr, col, na, nb = O.load_graph("n_1000")
    n, chains, seed = na + nb, 8, 5
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    labels0 = O.contiguous_labels(na, nb, 3, 3)

    def model():
        m = B.BlockModel(labels0, syn.types_vector(na, nb), 6, 3, 3, 1.0, (rowptr, col), n_chains=chains, seed=seed)
        m.shuffle_bisbm()
        return m
    # marginalize(sampler="heatbath") is the Python calls
    m = model()
    labels, counts = B.marginalize(m, 10, 3, 2, align=True, sampler="heatbath")
    m2 = model()
    m2.heatbath_sweeps(10, 1.0)
    m2.marginals_reset()
    m2.marginals_set_alignment(True)
    for _ in range(3):
        m2.heatbath_sweeps(2, 1.0)
        m2.marginals_accumulate(None)
    assert (counts == m2.marginals_get()).all() and counts.sum() == 3 * chains * n
    m3 = model()
    assert not (B.marginalize(m3, 10, 3, 2, align=True)[1] == counts).all()  # (the default is still the MH sweeps)
    m4 = model()
    modes = B.marginalize_modes(m4, 10, 3, 2, mode_of_chain=np.zeros(chains, dtype=np.uint32), sampler="heatbath")
    assert (modes["counts"][0] == counts).all()  # (one mode of all chains: the aligned pooled histogram)
    for x in (m, m2, m3, m4):
        x.close()
    # mcmc --marginalize --heatbath
    sizes = [str(x) for x in np.bincount(labels0)]
    base = [cli, "-e", el, "-y", str(na), str(nb), "-z", "3", "3", "-n", *sizes, "-r", "-d", str(seed), "--rng", "philox", "--chains", str(chains)]
    r = subprocess.run(base + ["-b", str(10 * n), "-t", str(6 * n), "-f", str(2 * n), "--marginalize", "--align", "--heatbath"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout == B.output_vec(labels, stream=open(os.devnull, "w"))
    # mcmc --polish
    r = subprocess.run(base + ["-c", "constant", "-x", "100000000", "-t", str(5 * n), "--polish", "50"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    m = model()
    B.MetropolisHasting().anneal(m, "constant", [1.0], 5 * n, 100000000)
    moved, sweeps = m.polish(50)
    best = int(np.argmin(m.entropy()))
    assert r.stdout == B.output_vec(m.get_memberships(best), stream=open(os.devnull, "w"))
    lines = [l for l in r.stderr.splitlines() if l.startswith("polish: ")]
    assert lines == ["polish: chain %d moved %d node(s) in %d sweep(s)" % (c, moved[c], sweeps[c]) for c in range(chains)]
    assert "printing chain %d\n" % best in r.stderr
    m.close()


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "polish.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "a second polish moves nothing: 0 moves, 1 sweep(s) per chain" in r.stdout, r.stdout + r.stderr
