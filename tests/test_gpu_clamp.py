"""GPU tests of the clamped nodes (include/bisbm.h, "Clamped nodes").

Every sampler is held to what the header says of a clamped node: the heat-bath sweeps and the pair reshuffles to the host
replays of tests/test_gpu_heatbath.py and tests/test_gpu_reshuffle.py with the clamp added (free and not clamped; members
filtered to the open nodes), the MH sweeps to the oracle sweep by sweep, the shuffle to the oracle's shuffle of the compacted
label vectors, all of them together to the exact distribution of the enumerable graph restricted to the states that agree
with the clamp.  Labels, counts and the block state are integers; running sums and records are compared on bit patterns."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_gpu_heatbath import _assert_state_is_a_rebuild, _bits, _case, _model, _refused
from test_gpu_reshuffle import _Helper, _draw, _pair_of_move
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
    """the unclamped MH sweeps of these tests keep the sum of their own dS values (tests/test_gpu_heatbath.py does the same)"""
    monkeypatch.setenv("BISBM_KEEP_SUM", "1")


def _visit(gid, sweep, na, nb):
    L = O.lib()
    return [int(L.orc_philox_visit(SEED, gid, sweep, na, nb, i)) for i in range(na + nb)]


def _state(m, c):
    return (m.get_memberships(c), m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c))


def _same_state(x, y):
    return all((u == v).all() for u, v in zip(x, y))


def _random_mask(n, share, seed):
    return np.random.default_rng(seed).random(n) < share


# ------------------------------------------------------------------------------------------------------- 1. heat bath
def _heatbath_replay(name, sweeps, make_mask, beta=1.0):
    """chain 2 of a three-chain handle with first chain id 5, after a shuffle and three unclamped MH sweeps; make_mask(visit
    order of the first replayed sweep) -> the clamp.  Returns (mask, that visit order)."""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, chains = na + nb, 3
    m = _model(name, chains, first_chain_id=FIRST_ID)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    c, gid, sweep0 = chains - 1, FIRST_ID + chains - 1, 3
    first_order = _visit(gid, sweep0, na, nb)
    mask = np.asarray(make_mask(first_order), dtype=bool)
    m.clamp(mask)
    assert (m.clamped() == mask).all()
    lab = m.get_memberships(c).astype(np.int64)
    start = lab.copy()
    cum, S0 = m.get_entropy()[c], m.entropy()[c]
    helper = _model(name, 1, labels=lab.astype(np.uint32))
    helper.conditionals_set(None, beta, keep_last=True)

    def sync():
        helper.set_memberships(lab.astype(np.uint32))
        helper.init_bisbm()
        helper.conditionals_accumulate()
    sync()
    moved_gpu = m.heatbath_sweeps(sweeps, beta)
    moved, total, open_free, held_free = 0, 0.0, 0, 0
    for sw in range(sweeps):
        order = first_order if sw == 0 else _visit(gid, sweep0 + sw, na, nb)
        for pos, v in enumerate(order):
            k_own, lo = (ka, 0) if v < na else (kb, ka)
            r = int(lab[v]) - lo
            free = k_own > 1 and int((lab == lab[v]).sum()) > 1
            held_free += free and bool(mask[v])
            free = free and not mask[v]
            open_free += free
            dS, P = (x[0] for x in helper.conditionals_last(v))
            o = philox(SEED, gid, B.PHILOX_PURPOSE_HEATBATH, (sweep0 + sw) * n + pos)
            s = D.numpy_heatbath_choice(dS, P, r, free, u53(o[0], o[1]), False)
            if s != r:
                lab[v] = lo + s
                cum = cum + dS[s]
                total = total + dS[s]
                moved += 1
                sync()
    assert open_free > 0 and held_free > 0 and moved > 0, (open_free, held_free, moved)
    got = m.get_memberships(c)
    assert (got[mask] == start[mask]).all()
    assert (got == lab).all()
    assert int(moved_gpu[c]) == moved
    acc, sw_counts = m.last_counts()
    assert int(acc[c]) == moved and int(sw_counts[c]) == sweeps
    for x, y in zip(_state(m, c)[1:], _state(helper, 0)[1:]):
        assert (x == y).all()
    assert _bits(m.get_entropy()[c]) == _bits(cum)
    S1 = m.entropy()[c]
    print("%s: %d of %d nodes clamped, %d moves in %d sweep(s), sum dS %.6f, S %.6f -> %.6f" % (name, mask.sum(), n, moved, sweeps, total, S0, S1))
    assert abs((S1 - S0) - total) <= 1e-9 * abs(S0)
    for other in range(chains - 1):  # (the other chains ran too: consistent, and their clamped nodes stayed)
        _assert_state_is_a_rebuild(m, rowptr, col, other)
    m.close()
    helper.close()
    return mask, first_order


def test_heat_bath_sweeps_on_the_tiny_graph_are_the_host_replay():
    _heatbath_replay("tiny", 3, lambda order: np.arange(21) % 3 == 0)


def test_heat_bath_sweep_with_a_skipped_chunk_and_a_chunk_of_one_open_node_is_the_host_replay():
    """300 + 200 nodes: positions 64 .. 127 of the type-a phase are all clamped (a chunk that reads no row), positions 128 .. 191
    hold one open node, every third node of the rest is clamped, and the hub (node 0, degree 179) is open"""
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    deg = np.diff(rowptr.astype(np.int64))
    hub = int(np.argmax(deg))

    def make(order):
        mask = np.arange(na + nb) % 3 == 1
        mask[order[64:192]] = True
        mask[order[150]] = False
        mask[hub] = False
        return mask
    mask, order = _heatbath_replay(name, 1, make)
    assert mask[order[64:128]].all()
    assert int((~mask[order[128:192]]).sum()) == 1
    assert deg[hub] > 64 and not mask[hub] and all(v < na for v in order[:192])


# -------------------------------------------------------------------------------------------------------- 2. polishing
def test_polish_settles_the_open_nodes_and_leaves_the_clamped_ones_off_their_minimum():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    m = _model(name, 2)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    m.polish(100)
    m.conditionals_set(None, 1.0, keep_last=True)

    def rows(c):
        m.conditionals_accumulate()
        return [m.conditionals_last(v)[0][c] for v in range(n)]
    lab = m.get_memberships(0).astype(np.int64)
    dS = rows(0)
    rng = np.random.default_rng(8)
    sizes = np.bincount(lab, minlength=ka + kb)
    held = []
    for v in rng.permutation(n):  # 40 nodes, each to the block its row likes least, while its own block keeps others
        v = int(v)
        lo = 0 if v < na else ka
        worst = lo + int(np.argmax(dS[v]))
        if len(held) < 40 and sizes[lab[v]] > 5 and worst != lab[v] and dS[v][worst - lo] > 0:
            sizes[lab[v]] -= 1
            sizes[worst] += 1
            lab[v] = worst
            held.append(v)
    assert len(held) == 40
    mask = np.zeros(n, dtype=bool)
    mask[held] = True
    m.set_memberships(lab.astype(np.uint32))
    m.init_bisbm()
    m.clamp(mask)
    moved, sweeps = m.polish(100)
    assert (sweeps < 100).all()
    for c in range(2):
        after = m.get_memberships(c).astype(np.int64)
        assert (after[mask] == lab[mask]).all()
        dS = rows(c)
        free = np.bincount(after, minlength=ka + kb)[after] > 1
        assert not any(free[v] and not mask[v] and (dS[v] < 0).any() for v in range(n)), c
        assert any((dS[v] < 0).any() for v in held), c  # (the clamp is what holds them)
        _assert_state_is_a_rebuild(m, rowptr, col, c)
    m.close()


# ------------------------------------------------------------------------------------------------------- 3. reshuffles
def _reshuffle_replay(m, c, gid, name, moves, scans, beta, mask):
    """tests/test_gpu_reshuffle.py::_replay_moves with the members filtered to the open nodes; a move with fewer than two
    members is a counted no-op.  Returns per move (pair, M, original labels of the members, launch labels)."""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    lab = m.get_memberships(c).astype(np.int64)
    start = lab.copy()
    cum, S0 = m.get_entropy()[c], m.entropy()[c]
    j0 = int(m.reshuffles_total()[c])
    helper = _Helper(name, lab, beta)
    exp = lambda x: m.debug_exp([float(x)])[0]
    accepted_gpu = m.reshuffle(moves, scans, beta)
    got = m.reshuffle_last()[c]
    out, n_acc, total = [], 0, 0.0
    for j in range(j0, j0 + moves):
        t, rg, sg = _pair_of_move(SEED, gid, j, ka, kb)
        own0 = t * ka
        lo, hi = (na, na + nb) if t else (0, na)
        members = [v for v in range(lo, hi) if lab[v] in (rg, sg) and not mask[v]]
        M, W = len(members), (len(members) + 127) >> 7
        last = j == j0 + moves - 1
        if M < 2:
            if last:
                assert (got["type"], got["r"], got["s"], got["M"]) == (t, rg, sg, M) and not got["accepted"]
                assert got["dS_fwd"] == 0.0 and got["dS_rev"] == 0.0 and got["A"] == 0.0 and got["u_acc"] == 0.0
            out.append({"pair": (t, rg, sg), "M": M, "orig": lab[members].copy(), "launch": None, "accepted": False})
            continue
        orig = lab[members].copy()
        bits = [(_draw(SEED, gid, j, 2 + (i >> 7))[(i >> 5) & 3] >> (i & 31)) & 1 for i in range(M)]
        launch = np.asarray(D.numpy_reshuffle_launch(bits, rg, sg))
        lab[members] = launch

        def scan(scan_t=None, forced=None):
            factors, dsum = [], 0.0
            for i, v in enumerate(members):
                cur = int(lab[v])
                o = sg if cur == rg else rg
                free = int((lab == cur).sum()) > 1  # (the clamped nodes of the block count)
                dS_o = helper.dS(lab, v, o - own0) if free else None
                if forced is None:
                    U = _draw(SEED, gid, j, 2 + W + scan_t * M + i)
                    to_r, f, dead = D.numpy_reshuffle_step(dS_o, cur == rg, free, beta, u=u53(U[0], U[1]), exp=exp)
                else:
                    to_r, f, dead = D.numpy_reshuffle_step(dS_o, cur == rg, free, beta, forced_to_r=int(forced[i]) == rg, exp=exp)
                if dead:
                    return factors, dsum, True
                factors.append(f)
                if (rg if to_r else sg) != cur:
                    lab[v] = rg if to_r else sg
                    dsum = dsum + dS_o
            return factors, dsum, False
        for s_t in range(scans):
            scan(scan_t=s_t)
        L = lab[members].copy()
        f_rev, dS_rev, dead = scan(forced=orig)
        lab[members] = orig
        q_rev = (0.0, 0) if dead else D.numpy_reshuffle_q(f_rev)
        if dead:
            dS_fwd, q_fwd, A, acc = 0.0, (0.0, 0), 0.0, False
        else:
            lab[members] = L
            f_fwd, dS_fwd, _ = scan(scan_t=scans)
            q_fwd = D.numpy_reshuffle_q(f_fwd)
            A, acc = D.numpy_reshuffle_accept(dS_fwd, dS_rev, q_fwd, q_rev, beta, 0.0)
        U = _draw(SEED, gid, j, 1)
        u_acc = u53(U[0], U[1])
        if last:
            assert (got["type"], got["r"], got["s"], got["M"]) == (t, rg, sg, M)
            assert got["u_acc"] == u_acc
            assert _bits(got["dS_fwd"]) == _bits(dS_fwd) and _bits(got["dS_rev"]) == _bits(dS_rev), (got, dS_fwd, dS_rev)
            assert got["q_fwd"][1] == q_fwd[1] and got["q_rev"][1] == q_rev[1], (got, q_fwd, q_rev)
            assert _bits(got["q_fwd"][0]) == _bits(q_fwd[0]) and _bits(got["q_rev"][0]) == _bits(q_rev[0]), (got, q_fwd, q_rev)
            assert got["A"] == A or abs(got["A"] - A) <= 1e-12 * abs(A), (got["A"], A)
            assert got["accepted"] == (u_acc < got["A"])
            acc = got["accepted"]
        else:
            acc = u_acc < A
        if acc:
            cum = cum + (dS_fwd - dS_rev)
            total = total + (dS_fwd - dS_rev)
            n_acc += 1
        else:
            lab[members] = orig
        out.append({"pair": (t, rg, sg), "M": M, "orig": orig, "launch": launch, "accepted": bool(acc)})
    after = m.get_memberships(c)
    assert (after[mask] == start[mask]).all()
    assert (after == lab).all()
    assert int(accepted_gpu[c]) == n_acc
    assert int(m.reshuffles_total()[c]) == j0 + moves
    for got_x, want_x in zip(_state(m, c)[1:], helper.state(lab)):
        assert (got_x == want_x).all()
    assert _bits(m.get_entropy()[c]) == _bits(cum)
    S1 = m.entropy()[c]
    print("%s: %d move(s), %d scan(s), %d clamped: pairs %s, M %s, accepted %d, sum dS %.6f" % (name, moves, scans, mask.sum(), [x["pair"] for x in out], [x["M"] for x in out], n_acc, total))
    assert abs((S1 - S0) - total) <= 1e-9 * abs(S0)
    helper.m.close()
    return out


@pytest.mark.parametrize("name,moves,scans,share", [("tiny", 3, 1, None), ("hubs_isolated", 2, 3, 0.3)])
def test_reshuffles_are_the_host_replay_over_the_open_members(name, moves, scans, share):
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    chains, c = 3, 2
    m = _model(name, chains, first_chain_id=FIRST_ID)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    mask = np.arange(na + nb) % 3 == 0 if share is None else _random_mask(na + nb, share, 17)
    m.clamp(mask)
    out = _reshuffle_replay(m, c, FIRST_ID + c, name, moves, scans, 1.0, mask)
    lab = m.get_memberships(c)
    assert any(x["M"] >= 2 for x in out)
    assert any(x["M"] < int(np.isin(lab, x["pair"][1:]).sum()) for x in out)  # (a clamped node sat in a chosen pair)
    for other in range(chains - 1):
        _assert_state_is_a_rebuild(m, rowptr, col, other)
    m.close()


def _constructed(clamp_all_but_one):
    """tiny, chain 2 of three with first id 5: the pair of the chain's move 0 is (r, s).  Either block r is made of two clamped
    nodes and every other node of r and s sits open in s, or all nodes of r and s but one are clamped."""
    name = "tiny"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    chains, c = 3, 2
    gid = FIRST_ID + c
    t, rg, sg = _pair_of_move(SEED, gid, 0, ka, kb)
    lo, hi = (na, na + nb) if t else (0, na)
    lab = O.contiguous_labels(na, nb, ka, kb).astype(np.int64)
    own = np.arange(lo, hi)
    pool = own[np.isin(lab[own], (rg, sg))]
    mask = np.zeros(na + nb, dtype=bool)
    if clamp_all_but_one:
        mask[pool[:-1]] = True
    else:
        lab[pool] = sg
        lab[pool[:2]] = rg
        mask[pool[:2]] = True
    m = _model(name, chains, first_chain_id=FIRST_ID, labels=lab.astype(np.uint32))
    m.init_bisbm()
    m.clamp(mask)
    before = _state(m, c), m.get_entropy()[c]
    out = _reshuffle_replay(m, c, gid, name, 1, 1, 1.0, mask)[0]
    assert out["pair"] == (t, rg, sg)
    return m, c, out, before, len(pool), rg, sg


def test_a_block_of_clamped_nodes_only_gets_a_member_from_the_launch():
    m, c, out, before, pool, rg, sg = _constructed(False)
    assert out["M"] == pool - 2 >= 2 and (out["orig"] == sg).all()
    assert (out["launch"] == rg).any() and (out["launch"] == sg).any()  # (the launch put a member into r)
    m.close()


def test_one_open_node_in_the_pair_is_a_counted_no_op():
    m, c, out, before, pool, rg, sg = _constructed(True)
    assert out["M"] == 1
    assert _same_state(_state(m, c), before[0]) and _bits(m.get_entropy()[c]) == _bits(before[1])
    assert int(m.reshuffles_total()[c]) == 1
    m.close()


# --------------------------------------------------------------------------------------------- 4. MH against the oracle
LOW_T = 0.3


def test_mh_sweeps_follow_the_oracle_up_to_the_first_move_of_a_clamped_node():
    """Sweep by sweep: the oracle, set to the device's labels, runs the unclamped sweep; p* = the first position at which it
    changed a clamped node.  Up to p* the device made the oracle's steps; in a sweep without a p* it made all of them.  The
    accepted counts of such a sweep differ by exactly the clamped positions at which the oracle accepted a step that proposed
    the node's own block (an accepted step that moves nothing; under the clamp it is a step that was not accepted): these are
    recomputed from the step's own Philox draws on an oracle set to the state at that position."""
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, chains, c = na + nb, 3, 2
    gid = FIRST_ID + c
    m = _model(name, chains, first_chain_id=FIRST_ID)
    m.init_bisbm()
    base = 3
    m.run_sweeps(base)  # (unclamped, from the contiguous labels: the chain is still settling when the clamp is set)
    mask = _random_mask(n, 0.05, 4)
    assert 10 <= mask.sum() <= 50
    m.clamp(mask)
    o = O.OracleModel(rowptr, col, na, nb, ka, kb, eps, O.contiguous_labels(na, nb, ka, kb))
    o.seed_philox(SEED, gid)
    probe = O.OracleModel(rowptr, col, na, nb, ka, kb, eps, O.contiguous_labels(na, nb, ka, kb))
    o.init_bisbm()
    o.anneal("constant", [1.0], base * n, 1 << 60)  # (the oracle's sweep counter follows the device's)
    assert (o.memberships() == m.get_memberships(c)).all()
    with_p, without_p = 0, 0
    for sweep in range(base, base + 50):
        T = 1.0 if sweep < base + 10 else LOW_T
        lab0 = m.get_memberships(c)
        S_before, cum_before = m.entropy()[c], m.get_entropy()[c]
        o.set_memberships(lab0)
        o.init_bisbm()
        m.run_sweeps(1, temperature=T)
        o.anneal("constant", [T], n, 1 << 60)
        lab_d, lab_o = m.get_memberships(c), o.memberships()
        order = _visit(gid, sweep, na, nb)
        p_star = next((p for p, v in enumerate(order) if mask[v] and lab_o[v] != lab0[v]), None)
        assert (lab_d[mask] == lab0[mask]).all(), sweep
        before = order[:p_star] if p_star is not None else order
        assert (lab_d[before] == lab_o[before]).all(), (sweep, p_star)
        acc_d, sw_d = (int(x[c]) for x in m.last_counts())
        assert sw_d == 1
        if p_star is None:
            without_p += 1
            assert (lab_d == lab_o).all(), sweep
            own_block = 0  # clamped positions at which the oracle accepted a proposal of the node's own block
            for p, v in enumerate(order):
                if not mask[v]:
                    continue
                now = lab0.copy()
                now[order[:p]] = lab_o[order[:p]]
                probe.set_memberships(now)
                probe.init_bisbm()
                A, Bw = philox(SEED, gid, 0, sweep * n + p), philox(SEED, gid, 1, sweep * n + p)
                s = probe.propose_philox(v, u53(A[0], A[1]), u53(A[2], A[3]), u53(Bw[0], Bw[1]))
                own_block += int(s == now[v] and probe.n_r()[now[v]] > 1)
            assert acc_d == o.last_accepted - own_block, (sweep, acc_d, o.last_accepted, own_block)
        else:
            with_p += 1
            assert acc_d <= n - int(mask.sum())
        _assert_state_is_a_rebuild(m, rowptr, col, c)
        S_after, cum_after = m.entropy()[c], m.get_entropy()[c]
        assert abs((cum_after - cum_before) - (S_after - S_before)) <= 1e-9 * abs(S_before), sweep
    print("MH under a clamp of %d nodes: %d sweeps with a p*, %d without" % (mask.sum(), with_p, without_p))
    assert with_p >= 5 and without_p >= 5, (with_p, without_p)
    for other in range(chains - 1):
        _assert_state_is_a_rebuild(m, rowptr, col, other)
    m.close()


# ------------------------------------------------------------------------------------------ 5. stationary distribution
ENUM_HELD = {0: 0, 3: 1, 6: 2, 9: 3}
_ENUM = {}


def _enumeration():
    """the 256 states of the enumerable graph that agree with the clamp, and their S"""
    if not _ENUM:
        states, _, S = cases.enumerable_states()
        keep = np.array([all(((int(code) >> v) & 1) == (b & 1) for v, b in ENUM_HELD.items()) for code in states])
        assert keep.sum() == 256
        _ENUM["states"], _ENUM["S"] = states[keep], S[keep]
    return _ENUM["states"], _ENUM["S"]


@pytest.mark.parametrize("sampler,beta", [("mh", 1.0), ("mh", 5.0 / 3.0), ("heatbath", 1.0), ("reshuffle", 1.0)])
def test_clamped_chains_sample_the_target_restricted_to_the_clamp(sampler, beta):
    rowptr, col = cases.enumerable_graph()
    na, nb = cases.ENUM_NA, cases.ENUM_NB
    chains, moves = 8192, 400
    start = np.array([0, 0, 1, 1, 1, 0, 2, 2, 3, 3, 3, 2], dtype=np.uint32)  # (admissible: it agrees with the clamp)
    g = B.BlockModel(start, syn.types_vector(na, nb), 4, 2, 2, cases.ENUM_EPS, (rowptr, col), n_chains=chains, rng="philox", seed=4242)
    g.clamp(sorted(ENUM_HELD))
    g.shuffle_bisbm()
    if sampler == "mh":
        g.run_sweeps(moves, temperature=1.0 / beta)
    elif sampler == "heatbath":
        g.heatbath_sweeps(moves, beta)
    else:
        g.reshuffle(moves, 1, beta)
    codes = np.array([cases.state_code(g.get_memberships(c)) for c in range(chains)])
    g.close()
    states, S = _enumeration()
    target = np.exp(-beta * (S - S.min()))
    stat, dof, p = cases.chi_square(codes, states, target / target.sum())  # (KeyError: a clamped node moved)
    flat = np.exp(-beta * (S - S.min()) / 1.25)
    p_flat = cases.chi_square(codes, states, flat / flat.sum())[2]
    print("%s under a clamp, beta = %g: chi2 = %.1f on %d dof, p = %.3g; flattened target p = %.3g" % (sampler, beta, stat, dof, p, p_flat))
    assert p > 1e-3, (stat, dof, p)
    assert p_flat < 1e-6


# ------------------------------------------------------------------------------------------------------------ 6. shuffle
@pytest.mark.parametrize("b_open", [1, 0])
def test_the_shuffle_permutes_the_open_nodes_as_the_oracle_shuffles_the_compacted_labels(b_open):
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, chains = na + nb, 3
    mask = _random_mask(n, 0.4, 5)
    mask[na:] = True
    if b_open:
        mask[na + 77] = False
    m = _model(name, chains, first_chain_id=FIRST_ID)
    m.shuffle_bisbm()
    m.run_sweeps(2)  # (every chain its own labels)
    m.clamp(mask)
    F = np.flatnonzero(~mask)
    fa, fb = int((F < na).sum()), int((F >= na).sum())
    assert fb == b_open and fa > 64
    edgeless = (np.zeros(fa + fb + 1, dtype=np.uint64), np.zeros(1, dtype=np.uint32))
    start = [m.get_memberships(c) for c in range(chains)]
    oracles = []
    for c in range(chains):
        o = O.OracleModel(edgeless[0], edgeless[1], fa, fb, ka, kb, eps, start[c][F])
        o.seed_philox(SEED, FIRST_ID + c)
        o.shuffle_bisbm()  # (epoch 0: the handle's first shuffle above)
        o.set_memberships(start[c][F])
        oracles.append(o)
    for call in range(2):
        m.shuffle_bisbm()
        for c in range(chains):
            got = m.get_memberships(c)
            oracles[c].shuffle_bisbm()
            want = oracles[c].memberships()
            assert (got[mask] == start[c][mask]).all(), (call, c)
            assert (got[F] == want).all(), (call, c)
            assert (np.bincount(got, minlength=ka + kb) == np.bincount(start[c], minlength=ka + kb)).all()
            _assert_state_is_a_rebuild(m, rowptr, col, c)
        assert any((m.get_memberships(c)[F] != start[c][F]).any() for c in range(chains)), call
    m.close()


# ----------------------------------------------------------------------------------------------------------- 7. dispatch
def _three_calls(m):
    out = []
    m.run_sweeps(1)
    out.append(([m.get_memberships(c) for c in range(m.n_chains)], m.last_counts()[0].copy(), _bits(m.get_entropy()).copy()))
    moved = m.heatbath_sweeps(1, 1.0)
    out.append(([m.get_memberships(c) for c in range(m.n_chains)], moved, _bits(m.get_entropy()).copy()))
    acc = m.reshuffle(2, 1, 1.0)
    out.append(([m.get_memberships(c) for c in range(m.n_chains)], acc, _bits(m.get_entropy()).copy()))
    return out


def test_device_entries_behind_one_handle_give_one_handles_clamped_chains():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    mask = _random_mask(na + nb, 0.3, 9)
    runs = []
    for kw in ({}, {"devices": [0, 0, 0]}):
        m = _model(name, 6, first_chain_id=3, **kw)
        m.shuffle_bisbm()
        start = [m.get_memberships(c) for c in range(6)]
        m.clamp(mask)
        assert (m.clamped() == mask).all()
        runs.append(_three_calls(m))
        for c in range(6):
            assert (m.get_memberships(c)[mask] == start[c][mask]).all()
        m.close()
    for (l1, n1, s1), (l2, n2, s2) in zip(*runs):
        assert all((x == y).all() for x, y in zip(l1, l2)) and (n1 == n2).all() and (s1 == s2).all()


def test_replica_exchange_rounds_under_a_clamp_are_the_one_chain_handles():
    """the construction of tests/test_gpu_tempered_moves.py: 4 chains as 2 ensembles of 2 rungs, 3 rounds of {1 MH sweep, 1
    heat-bath sweep, 1 reshuffle}, every chain against the one-chain handle of its global id with the same clamp, run through
    the same calls at the temperature tempering_get reported"""
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    ladder, chains, first = [1.0, 1.5], 4, 4
    mask = _random_mask(na + nb, 0.25, 13)
    m = _model(name, chains, first_chain_id=first)
    m.shuffle_bisbm()
    m.clamp(mask)
    ones = []
    for c in range(chains):
        one = _model(name, 1, first_chain_id=first + c)
        one.shuffle_bisbm()
        one.clamp(mask)
        ones.append(one)
        assert _same_state(_state(m, c), _state(one, 0))
    start = [m.get_memberships(c) for c in range(chains)]
    m.set_tempering(ladder)
    changed_rung = False
    for r in range(3):
        T_now = m.tempering_state()[1]
        m.tempering_rounds(1, mh=1, heatbath=1, reshuffles=1, scans=1)
        for c, one in enumerate(ones):
            T = float(T_now[c])
            changed_rung = changed_rung or T != float(np.float32(ladder[c % 2]))
            one.run_sweeps(1, temperature=T)
            one.heatbath_sweeps(1, 1.0 / T)
            one.reshuffle(1, 1, 1.0 / T)
            assert _same_state(_state(m, c), _state(one, 0)), (r, c)
            assert _bits(m.get_entropy())[c] == _bits(one.get_entropy())[0], (r, c)
            assert (m.get_memberships(c)[mask] == start[c][mask]).all()
    print("replica exchange under a clamp: a chain ran a round off its first rung: %s" % changed_rung)
    for x in ones + [m]:
        x.close()


def test_a_resampling_step_carries_the_clamped_labels_of_the_ancestor():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    chains = 16
    mask = _random_mask(na + nb, 0.2, 21)
    m = _model(name, chains)
    m.shuffle_bisbm()
    m.clamp(mask)
    m.run_sweeps(2)
    held = [m.get_memberships(c)[mask] for c in range(chains)]
    assert len({x.tobytes() for x in held}) == chains  # (after the shuffle every chain holds other labels)
    S = m.entropy()
    parent, _ = m.population_resample(1.0, 1.0 + 1.0 / S.std())
    assert len(set(parent.tolist())) < chains  # (some slot took another chain's state)
    for c in range(chains):
        assert (m.get_memberships(c)[mask] == held[int(parent[c])]).all(), c
    m.heatbath_sweeps(1, 1.0)
    m.run_sweeps(1)
    for c in range(chains):
        assert (m.get_memberships(c)[mask] == held[int(parent[c])]).all(), c
    m.close()


# ----------------------------------------------------------------------------------------------------------- 8. clearing
@pytest.mark.parametrize("how", ["unclamp", "zeros"])
def test_a_cleared_clamp_leaves_the_handle_of_one_that_never_had_one(how):
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, chains = na + nb, 3
    a = _model(name, chains, first_chain_id=FIRST_ID)
    a.shuffle_bisbm()
    a.clamp(_random_mask(n, 0.3, 2))
    a.run_sweeps(1)
    if how == "unclamp":
        a.unclamp()
    else:
        a.clamp(np.zeros(n, dtype=np.uint8))
    assert not a.clamped().any()
    b = _model(name, chains, first_chain_id=FIRST_ID)
    b.shuffle_bisbm()   # (the shuffle epoch of a)
    b.run_sweeps(1)     # (... and its sweep counter)
    for c in range(chains):
        b.set_memberships(a.get_memberships(c), chain=c)
    b.init_bisbm()
    cum_a, cum_b = a.get_entropy(), b.get_entropy()

    def step(m, base):
        out = []
        m.run_sweeps(2)
        out.append((m.last_counts()[0].copy(), m.last_pass_steps()))
        out.append(m.heatbath_sweeps(1, 1.0))
        out.append(m.reshuffle(2, 1, 1.0))
        rec = [{k: (_bits(v).tolist() if isinstance(v, float) else v) for k, v in x.items()} for x in m.reshuffle_last()]
        return out, rec, [_state(m, c) for c in range(chains)], _bits(m.get_entropy() - base)
    ra, rb = step(a, cum_a), step(b, cum_b)
    assert ra[0][0][1] == rb[0][0][1] and ra[0][0][1] > 1  # (the production kernel runs again: more than one step per pass)
    for x, y in zip(ra[0], rb[0]):
        assert (np.asarray(x[0] if isinstance(x, tuple) else x) == np.asarray(y[0] if isinstance(y, tuple) else y)).all()
    assert ra[1] == rb[1]
    assert all(_same_state(x, y) for x, y in zip(ra[2], rb[2]))
    a.close()
    b.close()


# ----------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_and_the_round_trip():
    name = "tiny"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    mask = np.arange(n) % 4 == 1
    m = _model(name, 2)
    m.shuffle_bisbm()
    count = B.C.c_uint64(99)
    assert B.lib().bisbm_clamp_get(m._h, None, B.C.byref(count)) == B.BISBM_OK and count.value == 0
    m.clamp(np.flatnonzero(mask))  # (node ids)
    assert (m.clamped() == mask).all()
    assert B.lib().bisbm_clamp_get(m._h, None, B.C.byref(count)) == B.BISBM_OK and count.value == mask.sum()
    assert B.lib().bisbm_clamp_get(m._h, None, None) == B.BISBM_OK
    m.clamp(mask.astype(np.uint8) * 7)  # (any non-zero byte)
    assert (m.clamped() == mask).all()
    state = [_state(m, c) for c in range(2)]
    assert "bisbm_clamp_set(h, NULL)" in _refused(lambda: m.agg_merge(1, 0), B.BISBM_ERR_STATE)
    assert "bisbm_clamp_set(h, NULL)" in _refused(lambda: m.agg_merge(1), B.BISBM_ERR_STATE)
    assert all(_same_state(_state(m, c), state[c]) for c in range(2)) and m.ka_kb(0) == (ka, kb)
    assert (m.clamped() == mask).all()
    m.unclamp()
    m.agg_merge(1, 0)  # (allowed again)
    assert m.ka_kb(0) == (ka - 1, kb)
    m.close()
    compat = _model(name, 2, rng="mt19937-compat")
    compat.shuffle_bisbm()
    before = [compat.get_memberships(c) for c in range(2)]
    assert "MT19937" in _refused(lambda: compat.clamp(mask), B.BISBM_ERR_UNSUPPORTED)
    assert not compat.clamped().any() and all((x == compat.get_memberships(c)).all() for c, x in enumerate(before))
    compat.close()
    wide = _model("wide_labels", 2)
    wide.init_bisbm()
    _, wna, wnb = _case("wide_labels")[:3]
    assert "byte labels" in _refused(lambda: wide.clamp([0, 1]), B.BISBM_ERR_UNSUPPORTED)
    assert not wide.clamped().any()
    wide.close()
    from test_gpu_pair_scores import _merge_until_mixed, _mixed_shapes_model
    g, deg, gna, gnb = _mixed_shapes_model()
    _merge_until_mixed(g)
    assert len({g.ka_kb(c) for c in range(g.n_chains)}) > 1
    labels = [g.get_memberships(c) for c in range(g.n_chains)]
    assert "block counts" in _refused(lambda: g.clamp([0, 1, 2]), B.BISBM_ERR_STATE)
    assert not g.clamped().any() and all((x == g.get_memberships(c)).all() for c, x in enumerate(labels))
    g.close()
    with pytest.raises(ValueError):
        _model(name, 1).clamp([n])
    with pytest.raises(ValueError):
        _model(name, 1).clamp(np.zeros(n + 1, dtype=bool))


# --------------------------------------------------------------------------------------------- 10. the CLI and the example
def test_the_command_line_holds_the_listed_nodes(tmp_path):
    rowptr, col, na, nb = O.load_graph("n_1000")
    n = na + nb
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    # a membership file that is deliberately NOT the planted partition at the held nodes: they sit one block further
    planted = O.contiguous_labels(na, nb, 4, 6).astype(np.int64)
    held = np.arange(7, n, 20)
    labels = planted.copy()
    labels[held] = np.where(held < na, (planted[held] + 1) % 4, 4 + (planted[held] - 4 + 1) % 6)
    mb, cl = tmp_path / "labels.txt", tmp_path / "clamp.txt"
    mb.write_text("".join("%d\n" % x for x in labels))
    cl.write_text(" ".join(str(int(v)) for v in held[::-1]) + "\n%d\n" % held[0])  # (any order, a repeat)
    base = [cli, "-e", el, "-y", str(na), str(nb), "-z", "4", "6", "--membership_path", str(mb), "-d", "5", "--rng", "philox", "--chains", "4",
            "-b", str(3 * n), "-t", str(4 * n), "-f", str(2 * n), "--marginalize"]
    r = subprocess.run(base + ["--clamp", str(cl)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "clamp: %d of %d nodes held" % (len(held), n) in r.stderr
    out = np.array(r.stdout.split(), dtype=np.int64)
    assert len(out) == n and (out[held] == labels[held]).all()
    free = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert free.returncode == 0, free.stderr
    assert (np.array(free.stdout.split(), dtype=np.int64)[held] != labels[held]).any()  # (unheld, they leave the wrong block)
    bad = subprocess.run(base[:-1] + ["--clamp", str(cl), "--rng", "mt19937-compat"], capture_output=True, text=True, timeout=600)
    assert bad.returncode == 1 and "--rng philox" in bad.stderr
    cl.write_text("3 1000 4\n")
    bad = subprocess.run(base + ["--clamp", str(cl)], capture_output=True, text=True, timeout=600)
    assert bad.returncode == 1 and "'1000'" in bad.stderr and bad.stdout == ""


def test_marginalize_sets_the_clamp_before_the_burn_in():
    rowptr, col, na, nb = O.load_graph("n_1000")
    n, chains = na + nb, 8
    planted = O.contiguous_labels(na, nb, 4, 6)
    held = np.arange(0, n, 20)
    for kw in ({}, {"sampler": "heatbath"}, {"reshuffles": 1}, {"tempering": [1.0, 1.3], "rung_moves": {"mh": 1, "heatbath": 1, "reshuffles": 1}}):
        m = B.BlockModel(planted, syn.types_vector(na, nb), 10, 4, 6, 1.0, (rowptr, col), n_chains=chains, seed=5)
        m.init_bisbm()
        labels, counts = B.marginalize(m, 2, 2, 1, clamp=held, **kw)[:2]
        assert m.clamped().sum() == len(held) and (labels[held] == planted[held]).all(), kw
        assert all((m.get_memberships(c)[held] == planted[held]).all() for c in range(chains)), kw
        m.close()
    m = B.BlockModel(planted, syn.types_vector(na, nb), 10, 4, 6, 1.0, (rowptr, col), n_chains=chains, seed=5)
    m.init_bisbm()
    out = B.marginalize_modes(m, 1, 2, 1, threshold=0.5, clamp=held)
    assert all((m.get_memberships(c)[held] == planted[held]).all() for c in range(chains)) and out["labels"].shape[1] == n
    m.close()
    m = B.BlockModel(planted, syn.types_vector(na, nb), 10, 4, 6, 1.0, (rowptr, col), n_chains=chains, seed=5)
    m.init_bisbm()
    m.clamp(held)
    res = B.population_anneal(m, [2.0, 1.5, 1.0], 1, rung_moves={"mh": 1, "heatbath": 1, "reshuffles": 1})
    assert all((m.get_memberships(c)[held] == planted[held]).all() for c in range(chains)) and len(res["log_ratio"]) == 2
    m.close()


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "semi_supervised.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "clamped" in r.stdout and "no clamp" in r.stdout, r.stdout
