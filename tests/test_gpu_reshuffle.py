"""GPU tests of the pair reshuffles (include/bisbm.h, "Pair reshuffles").

The replay walks the moves of one chain on the host: the pair, the launch bits and every uniform from the oracle's Philox with
purpose 10, every evaluated step's dS from a one-chain helper handle that is set to the replay's current labels
(bisbm_conditionals_accumulate with KEEP_LAST: the device's own rows, whose entry of the other block the kernel's dS must equal
bit for bit), the exponentials from the device's probe (bisbm_debug_exp), and the choice, the factors and the acceptance from
distributed.numpy_reshuffle_* (tests/test_reshuffle.py ties those to the literal loops).  Labels, counts and the block state are
integers; dS_fwd, dS_rev, both Q and the running sum of dS are compared on bit patterns."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_gpu_heatbath import _assert_state_is_a_rebuild, _bits, _case, _model, _refused
from test_gpu_pair_scores import _merge_until_mixed, _mixed_shapes_model
from test_tempering import philox, u53

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu

SEED = 21
FIRST_ID = 5
PURPOSE = B.PHILOX_PURPOSE_RESHUFFLE
SEEN = {"accepted": 0, "rejected": 0}  # over all replays of this module (test_the_replays_saw_both_outcomes)


@pytest.fixture(autouse=True)
def _every_launch_keeps_its_own_sum(monkeypatch):
    """the MH sweeps of these tests keep the sum of their own dS values (tests/test_gpu_heatbath.py does the same)"""
    monkeypatch.setenv("BISBM_KEEP_SUM", "1")


def _draw(seed, gid, j, k):
    return philox(seed, gid, PURPOSE, (j << 32) | k)


def _pair_of_move(seed, gid, j, ka, kb):
    """(type, r, s) in global labels of the pair move j of the chain selects"""
    t, r, s = D.numpy_reshuffle_pair(_draw(seed, gid, j, 0)[0], ka, kb)
    return t, r + t * ka, s + t * ka


class _Helper:
    """a one-chain handle that returns the device's conditional rows of the replay's current labels"""

    def __init__(self, name, lab, beta):
        self.m = _model(name, 1, labels=lab.astype(np.uint32))
        self.m.conditionals_set(None, beta, keep_last=True)
        self.synced = None

    def dS(self, lab, v, o_loc):
        if self.synced is None or not (self.synced == lab).all():
            self.m.set_memberships(lab.astype(np.uint32))
            self.m.init_bisbm()
            self.m.conditionals_accumulate()
            self.synced = lab.copy()
        return float(self.m.conditionals_last(v)[0][0][o_loc])

    def state(self, lab):
        self.m.set_memberships(lab.astype(np.uint32))
        self.m.init_bisbm()
        self.synced = None
        return self.m.get_m(0), self.m.get_m_r(0), self.m.get_n_r(0), self.m.get_eta_rk_(0)


def _replay_moves(m, c, gid, name, moves, scans, beta, seed=SEED):
    """Runs `moves` moves on the device in one call and replays chain c of `m` on the host; asserts everything the two share and
    returns what the callers assert their edge on: per move the pair, M, L (the labels after the launch scans), whether a member
    that was not free stayed, whether the reverse pass died, and the outcome."""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    rowptr, col = rowptr.astype(np.int64), col.astype(np.int64)
    lab = m.get_memberships(c).astype(np.int64)
    cum = m.get_entropy()[c]
    S0 = m.entropy()[c]
    j0 = int(m.reshuffles_total()[c])
    helper = _Helper(name, lab, beta)
    exp = lambda x: m.debug_exp([float(x)])[0]
    accepted_gpu = m.reshuffle(moves, scans, beta)
    got = m.reshuffle_last()[c]
    out, n_acc, total = [], 0, 0.0
    for j in range(j0, j0 + moves):
        t, rg, sg = _pair_of_move(seed, gid, j, ka, kb)
        own0 = t * ka
        lo, hi = (na, na + nb) if t else (0, na)
        members = [v for v in range(lo, hi) if lab[v] in (rg, sg)]
        M, W = len(members), (len(members) + 127) >> 7
        assert M >= 2
        orig = lab[members].copy()
        info = {"pair": (t, rg, sg), "M": M, "not_free_stayed": 0, "dead": False, "evaluated": 0, "longest_list": 0, "highest_t": 0}
        bits = [(_draw(seed, gid, j, 2 + (i >> 7))[(i >> 5) & 3] >> (i & 31)) & 1 for i in range(M)]
        lab[members] = D.numpy_reshuffle_launch(bits, rg, sg)

        def scan(scan_t=None, forced=None):
            """one pass over the members: a free scan with the uniforms of scan `scan_t`, or forced to the labels `forced`;
            returns (factors, sum of dS, dead)"""
            factors, dsum = [], 0.0
            for i, v in enumerate(members):
                cur = int(lab[v])
                o = sg if cur == rg else rg
                free = int((lab == cur).sum()) > 1
                dS_o = helper.dS(lab, v, o - own0) if free else None
                info["evaluated"] += free
                if free:
                    blocks = set(lab[col[rowptr[v]:rowptr[v + 1]]].tolist())  # (of the other type: they never change in a move)
                    info["longest_list"] = max(info["longest_list"], len(blocks))
                    info["highest_t"] = max([info["highest_t"]] + [x - (0 if t else ka) for x in blocks])
                if forced is None:
                    U = _draw(seed, gid, j, 2 + W + scan_t * M + i)
                    to_r, f, dead = D.numpy_reshuffle_step(dS_o, cur == rg, free, beta, u=u53(U[0], U[1]), exp=exp)
                else:
                    to_r, f, dead = D.numpy_reshuffle_step(dS_o, cur == rg, free, beta, forced_to_r=int(forced[i]) == rg, exp=exp)
                if not free and not dead:
                    info["not_free_stayed"] += 1
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
        info["L"] = L
        deg = np.diff(rowptr)
        info["m_r"] = [int(deg[members][x == b].sum()) for x in (orig, L) for b in (rg, sg)]  # (of r and s, at the start and at L)
        f_rev, dS_rev, dead = scan(forced=orig)
        lab[members] = orig  # (the pass ends at the original state; a dead one in transit)
        q_rev = (0.0, 0) if dead else D.numpy_reshuffle_q(f_rev)
        info["dead"] = dead
        if dead:
            dS_fwd, q_fwd, A, acc = 0.0, (0.0, 0), 0.0, False
        else:
            lab[members] = L
            f_fwd, dS_fwd, _ = scan(scan_t=scans)
            q_fwd = D.numpy_reshuffle_q(f_fwd)
            A, acc = D.numpy_reshuffle_accept(dS_fwd, dS_rev, q_fwd, q_rev, beta, 0.0)
        U = _draw(seed, gid, j, 1)
        u_acc = u53(U[0], U[1])
        last = j == j0 + moves - 1
        if last:  # the device's record of this move
            assert (got["type"], got["r"], got["s"], got["M"]) == (t, rg, sg, M)
            assert got["u_acc"] == u_acc
            assert _bits(got["dS_fwd"]) == _bits(dS_fwd) and _bits(got["dS_rev"]) == _bits(dS_rev), (got, dS_fwd, dS_rev)
            assert got["q_fwd"][1] == q_fwd[1] and got["q_rev"][1] == q_rev[1], (got, q_fwd, q_rev)
            assert _bits(got["q_fwd"][0]) == _bits(q_fwd[0]) and _bits(got["q_rev"][0]) == _bits(q_rev[0]), (got, q_fwd, q_rev)
            assert got["A"] == A or abs(got["A"] - A) <= 1e-12 * abs(A), (got["A"], A)
            assert got["accepted"] == (u_acc < got["A"])
            acc = got["accepted"]  # (the device's A decides, should the two differ in the last bits right at u_acc)
        else:
            acc = u_acc < A
        if acc:
            cum = cum + (dS_fwd - dS_rev)
            total = total + (dS_fwd - dS_rev)
            n_acc += 1
        else:
            lab[members] = orig
        info["accepted"] = bool(acc)
        SEEN["accepted" if acc else "rejected"] += 1
        out.append(info)
    assert (m.get_memberships(c) == lab).all()
    assert int(accepted_gpu[c]) == n_acc
    assert int(m.reshuffles_total()[c]) == j0 + moves
    for got_x, want_x in zip((m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c)), helper.state(lab)):
        assert (got_x == want_x).all()
    assert _bits(m.get_entropy()[c]) == _bits(cum)
    S1 = m.entropy()[c]
    print("%s: %d move(s), %d scan(s): pairs %s, M %s, accepted %d, sum dS %.6f, S %.6f -> %.6f"
          % (name, moves, scans, [x["pair"] for x in out], [x["M"] for x in out], n_acc, total, S0, S1))
    assert abs((S1 - S0) - total) <= 1e-9 * abs(S0)
    helper.m.close()
    return out


def _replay(name, moves, scans, beta=1.0, sweeps=3, labels=None, first=FIRST_ID, wants=None):
    """the last chain of a three-chain handle with a non-zero first chain id; wants(labels of that chain): whether the start
    serves the caller's edge (None is returned when it does not)"""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    chains = 3
    m = _model(name, chains, first_chain_id=first, labels=labels)
    if labels is None:
        m.shuffle_bisbm()
        m.run_sweeps(sweeps)
    else:
        m.init_bisbm()
    if wants is not None and not wants(m.get_memberships(chains - 1)):
        m.close()
        return None
    out = _replay_moves(m, chains - 1, first + chains - 1, name, moves, scans, beta)
    for other in range(chains - 1):  # (the other chains ran too, and are consistent)
        _assert_state_is_a_rebuild(m, rowptr, col, other)
    m.close()
    return out


# ------------------------------------------------------------------------------------------------------- 1. exact replay
@pytest.mark.parametrize("scans", [0, 2])
def test_three_moves_on_the_tiny_graph_are_the_host_replay(scans):
    _replay("tiny", 3, scans)


def test_a_second_chunk_of_members_hubs_and_isolated_nodes_are_the_host_replay():
    """5 + 7 blocks over 300 + 200 nodes: a pair of type a has about 120 members -- a second chunk of 64 --, the hubs' rows run
    past the 64 neighbour labels a header parks, the isolated nodes have empty lists"""
    out = _replay("hubs_isolated", 2, 1)
    assert max(x["M"] for x in out) > 64, [x["M"] for x in out]


def test_eta_in_hbm_is_the_host_replay():
    _replay("hb_eta_in_hbm", 2, 1)


def test_a_list_longer_than_one_wave_is_the_host_replay():
    """100 blocks of type b and a type-a hub of some 610 neighbours: the list of a type-a member runs into a second chunk of
    lanes.  3 of the 4953 pairs are of type a and two of those hold the hub (node 0): the first chain id is chosen so that the
    chain's move 0 is such a pair (the pair is a function of seed, chain id and move alone)."""
    name = "hb_long_list"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    out = None
    for first in range(1, 40000):
        t, rg, sg = _pair_of_move(SEED, first + 2, 0, ka, kb)
        if t == 0:
            out = _replay(name, 1, 1, first=first, wants=lambda lab: lab[0] in (rg, sg))
            if out is not None:
                break
    assert out is not None and out[0]["pair"][0] == 0 and out[0]["longest_list"] > 64, out and (out[0]["pair"], out[0]["longest_list"])


def test_a_type_b_pair_against_70_type_a_blocks_is_the_host_replay():
    """wideK: 70 + 3 blocks; the histogram and the list of a type-b member run over 70 blocks of the other type, a second chunk of
    lanes.  3 of the 2418 pairs are of type b: the first chain id is chosen so that the chain's move 0 is one"""
    name = "wideK"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    first = next(f for f in range(1, 40000) if _pair_of_move(SEED, f + 2, 0, ka, kb)[0] == 1)
    out = _replay(name, 1, 1, first=first)
    assert out[0]["pair"][0] == 1 and out[0]["highest_t"] >= 64, (out[0]["pair"], out[0]["highest_t"])


def test_one_move_past_the_log_q_table_is_the_host_replay():
    """mid_tier_low: 2 + 2 blocks of about 1200 nodes with m_r past the q table; one move with scans = 0 over all 2400 nodes of
    a type"""
    name = "mid_tier_low"
    out = _replay(name, 1, 0)[0]
    assert out["M"] == 2400 and not out["dead"] and out["evaluated"] >= 2 * 2400 - 2
    assert min(out["m_r"]) > 10000, out["m_r"]  # (log_q past the q table at both ends of the reverse pass)


def test_a_block_of_one_node_the_member_that_is_not_free_and_the_certain_rejection():
    """A start built by hand for the pair each move selects: block s holds the last node of the type alone.  With scans = 0 the
    launch bit of that node decides: set, it sits alone in s when the reverse pass reaches it and stays with the factor 1.0 (not
    free); clear, the last other member of s is forced out of a block it is alone in, Q_rev = 0 and the move is rejected for
    certain."""
    name = "tiny"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    chains, c = 3, 2
    gid = FIRST_ID + c
    m = _model(name, chains, first_chain_id=FIRST_ID)
    m.shuffle_bisbm()
    stayed = died = 0
    for j in range(8):
        assert int(m.reshuffles_total()[c]) == j
        t, rg, sg = _pair_of_move(SEED, gid, j, ka, kb)
        lab = O.contiguous_labels(na, nb, ka, kb).astype(np.int64)
        lo, hi = (na, na + nb) if t else (0, na)
        own = np.arange(lo, hi)
        lab[own[lab[own] == sg]] = rg
        lab[hi - 1] = sg
        for x in range(chains):
            m.set_memberships(lab.astype(np.uint32), chain=x)
        m.init_bisbm()
        out = _replay_moves(m, c, gid, name, 1, 0, 1.0)[0]
        stayed += out["not_free_stayed"] > 0
        died += out["dead"]
        assert not (out["dead"] and out["accepted"])
    assert stayed > 0 and died > 0, (stayed, died)
    m.close()


def test_the_replays_saw_both_outcomes():
    """a module that passed on rejections alone would have checked no accepted state (run on its own, this test replays the tiny
    graph first, where both come up)"""
    if not (SEEN["accepted"] and SEEN["rejected"]):
        _replay("tiny", 3, 2)
    assert SEEN["accepted"] > 0 and SEEN["rejected"] > 0, SEEN


# ------------------------------------------------------------------------------------- 2. a rejection restores everything
def test_a_rejected_move_restores_everything_and_an_accepted_one_is_a_rebuild():
    name, chains = "hubs_isolated", 8
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    m = _model(name, chains)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    o = O.OracleModel(rowptr, col, na, nb, ka, kb, eps, O.contiguous_labels(na, nb, ka, kb))

    def snapshot():
        return [(m.get_memberships(c), m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c)) for c in range(chains)], m.get_entropy(), m.entropy()
    n_acc = n_rej = 0
    for move in range(6):
        before, cum0, S0 = snapshot()
        acc = m.reshuffle(1, 1, 1.0)
        rec = m.reshuffle_last()
        after, cum1, S1 = snapshot()
        for c in range(chains):
            assert bool(acc[c]) == rec[c]["accepted"]
            if not rec[c]["accepted"]:
                n_rej += 1
                assert all((x == y).all() for x, y in zip(before[c], after[c])), (move, c)
                assert _bits(cum0[c]) == _bits(cum1[c])
            else:
                n_acc += 1
                o.set_memberships(after[c][0])
                o.init_bisbm()
                K = ka + kb
                assert (after[c][1] == o.m()).all() and (after[c][2] == o.m_r()).all() and (after[c][3] == o.n_r()).all()
                assert (after[c][4] == o.eta()[:, :after[c][4].shape[1]]).all()
                assert int((after[c][0] != before[c][0]).sum()) <= rec[c]["M"]
                dS = rec[c]["dS_fwd"] - rec[c]["dS_rev"]
                assert _bits(cum1[c]) == _bits(cum0[c] + dS)
                assert abs((S1[c] - S0[c]) - dS) <= 1e-9 * abs(S0[c]), (S1[c] - S0[c], dS)
    print("rejection restores: %d accepted, %d rejected" % (n_acc, n_rej))
    assert n_acc > 0 and n_rej > 0
    m.close()


# ------------------------------------------------------------------------------------------- 3. stationary distribution
@pytest.mark.parametrize("beta", [1.0, 5.0 / 3.0])
def test_reshuffles_alone_sample_exp_minus_beta_S(beta):
    """32768 chains on the enumerable 6 + 6 graph, one sample each after 400 reshuffle moves with scans = 1 and no sweep in
    between, against exp(-beta (S - S_min)) over the 3844 admissible states (the set-up of
    test_gpu_heatbath.py::test_heat_bath_chains_sample_exp_minus_beta_S; a state with an empty block makes chi_square raise).  A
    wrong Q ratio or a wrong sign in the acceptance cannot pass this."""
    rowptr, col = cases.enumerable_graph()
    na, nb = cases.ENUM_NA, cases.ENUM_NB
    chains, moves = 32768, 400
    g = B.BlockModel(O.contiguous_labels(na, nb, 2, 2), syn.types_vector(na, nb), 4, 2, 2, cases.ENUM_EPS, (rowptr, col),
                     n_chains=chains, rng="philox", seed=4242)
    g.shuffle_bisbm()
    accepted = g.reshuffle(moves, 1, beta)
    rate = float(accepted.sum()) / (chains * moves)
    codes = np.array([cases.state_code(g.get_memberships(c)) for c in range(chains)])
    g.close()
    states, _, S = cases.enumerable_states()
    target = np.exp(-beta * (S - S.min()))
    stat, dof, p = cases.chi_square(codes, states, target / target.sum())
    flat = np.exp(-beta * (S - S.min()) / 1.25)
    p_flat = cases.chi_square(codes, states, flat / flat.sum())[2]
    print("reshuffles, beta = %g: acceptance %.3f; chi2 = %.1f on %d dof, p = %.3g; flattened target p = %.3g" % (beta, rate, stat, dof, p, p_flat))
    assert rate >= 0.1, "400 moves are too few at this acceptance: raise the count"
    assert p > 1e-3, (stat, dof, p)
    assert p_flat < 1e-6


# ----------------------------------------------------------------------------------------- 4. independence of the split
def test_the_launch_state_does_not_depend_on_how_the_members_were_divided():
    """two one-chain handles with the same seed and chain id whose labels differ only in how the nodes of r and s -- the pair of
    move 0 -- are divided: the host replay of each (which the device is held to) must reach the same L"""
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    gid = 9
    t, rg, sg = _pair_of_move(SEED, gid, 0, ka, kb)
    a = _model(name, 1, first_chain_id=gid)
    a.shuffle_bisbm()
    a.run_sweeps(3)
    lab = a.get_memberships(0).astype(np.int64)
    members = np.flatnonzero((lab == rg) | (lab == sg))
    other = lab.copy()
    rng = np.random.default_rng(3)
    other[members] = np.where(rng.random(len(members)) < 0.5, rg, sg)
    assert (other[members] != lab[members]).any() and {rg, sg} <= set(other[members].tolist())
    b = _model(name, 1, first_chain_id=gid, labels=other.astype(np.uint32))
    b.init_bisbm()
    ra = _replay_moves(a, 0, gid, name, 1, 2, 1.0)[0]
    rb = _replay_moves(b, 0, gid, name, 1, 2, 1.0)[0]
    assert ra["pair"] == rb["pair"] == (t, rg, sg) and ra["M"] == rb["M"] == len(members)
    assert (ra["L"] == rb["L"]).all()
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------ 5. dispatch
def _run(m):
    m.shuffle_bisbm()
    acc = m.reshuffle(4, 1, 1.0)
    return [m.get_memberships(c) for c in range(m.n_chains)], acc, m.get_entropy(), m.reshuffle_last()


def test_device_entries_behind_one_handle_give_one_handles_labels_and_records():
    name = "hubs_isolated"
    one = _model(name, 6, first_chain_id=3)
    labels, acc, cum, rec = _run(one)
    for entries in (2, 3):
        many = _model(name, 6, first_chain_id=3, devices=[0] * entries)
        l2, a2, c2, r2 = _run(many)
        assert all((x == y).all() for x, y in zip(labels, l2)) and (acc == a2).all() and (_bits(cum) == _bits(c2)).all(), entries
        for x, y in zip(rec, r2):
            assert {k: (_bits(v).tolist() if isinstance(v, float) else v) for k, v in x.items()} == \
                   {k: (_bits(v).tolist() if isinstance(v, float) else v) for k, v in y.items()}
        assert (one.reshuffles_total() == many.reshuffles_total()).all()
        many.close()
    one.close()


def test_chains_grouped_by_shape_are_served():
    g, deg, na, nb = _mixed_shapes_model()
    _merge_until_mixed(g)
    rowptr, col, _, _ = O.load_graph("n_1000")
    assert len({g.ka_kb(c) for c in range(g.n_chains)}) > 1
    S0, cum0 = g.entropy(), g.get_entropy()
    acc = g.reshuffle(6, 1, 1.0)
    rec = g.reshuffle_last()
    S1, cum1 = g.entropy(), g.get_entropy()
    assert acc.sum() > 0 and (g.reshuffles_total() == 6).all()
    for c in range(g.n_chains):
        _assert_state_is_a_rebuild(g, rowptr, col, c)
        ka, kb = g.ka_kb(c)
        assert rec[c]["r"] < rec[c]["s"] < ka + kb and (rec[c]["s"] < ka) == (rec[c]["type"] == 0)
    assert (np.abs((S1 - S0) - (cum1 - cum0)) <= 1e-9 * np.abs(S0)).all()
    g.close()


def test_refusals():
    name = "tiny"
    m = _model(name, 4)
    assert "bisbm_init" in _refused(lambda: m.reshuffle(1), B.BISBM_ERR_STATE)  # (labels set, block state not built)
    m.shuffle_bisbm()
    _refused(lambda: m.reshuffle_last(), B.BISBM_ERR_STATE)  # (no move on record yet)
    state = [m.get_memberships(c) for c in range(4)], m.get_entropy(), m.reshuffles_total()
    for beta in (float("nan"), 0.0, -1.0, float("inf"), -float("inf")):
        assert "beta" in _refused(lambda: m.reshuffle(1, 1, beta), B.BISBM_ERR_INVALID_ARG)
    m.set_tempering([1.0, 2.0])
    assert "replica exchange" in _refused(lambda: m.reshuffle(1), B.BISBM_ERR_STATE)
    m.set_tempering(None)
    assert (m.reshuffle(0) == 0).all()  # moves = 0: a no-op that returns OK
    after = [m.get_memberships(c) for c in range(4)], m.get_entropy(), m.reshuffles_total()
    assert all((x == y).all() for x, y in zip(state[0], after[0])) and (_bits(state[1]) == _bits(after[1])).all()
    assert (state[2] == after[2]).all() and (after[2] == 0).all()
    assert B.lib().bisbm_reshuffle_run(m._h, 1, 1, 1.0, None) == B.BISBM_OK  # (the output may be NULL)
    m.close()
    compat = _model(name, 2, rng="mt19937-compat")
    compat.shuffle_bisbm()
    before = [compat.get_memberships(c) for c in range(2)]
    assert "MT19937" in _refused(lambda: compat.reshuffle(1), B.BISBM_ERR_UNSUPPORTED)
    assert all((x == compat.get_memberships(c)).all() for c, x in enumerate(before))
    compat.close()
    wide = _model("wide_labels", 2)
    wide.init_bisbm()
    assert "byte labels" in _refused(lambda: wide.reshuffle(1), B.BISBM_ERR_UNSUPPORTED)
    wide.close()
    one = _model("ka1", 2)  # 1 + 4 blocks: type a has no pair, type b has six
    one.shuffle_bisbm()
    one.reshuffle(3)
    assert all(r["type"] == 1 for r in one.reshuffle_last())
    one.close()


# ------------------------------------------------------------------------------------------------------------ 6. counters
def test_counters_and_what_a_call_leaves_alone():
    name, chains = "hubs_isolated", 4
    m = _model(name, chains)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    counts = m.last_counts()
    labels = [m.get_memberships(c) for c in range(chains)]
    assert (m.reshuffles_total() == 0).all()
    m.reshuffle(1, 0, 1.0)  # (accepted or not: the labels are put back below)
    first = m.reshuffle_last()
    assert (m.reshuffles_total() == 1).all()
    for c in range(chains):
        m.set_memberships(labels[c], chain=c)
    m.init_bisbm()
    m.reshuffle(1, 0, 1.0)
    second = m.reshuffle_last()
    assert (m.reshuffles_total() == 2).all()
    # the same state, another move: the second call does not replay the draws of the first
    assert all(a["u_acc"] != b["u_acc"] for a, b in zip(first, second))
    m.reshuffle(5, 1, 1.0)
    assert (m.reshuffles_total() == 7).all()
    assert all((x == y).all() for x, y in zip(counts, m.last_counts()))  # (last_counts are the MH sweeps' still)
    # sweeps_total has not moved: the next MH sweeps are those of a fresh handle that ran two sweeps and took these labels
    labels = [m.get_memberships(c) for c in range(chains)]
    m.run_sweeps(2)
    for c in (0, chains - 1):
        f = _model(name, 1, labels=labels[c], first_chain_id=c)
        f.init_bisbm()
        f.run_sweeps(2)
        f.set_memberships(labels[c])
        f.init_bisbm()
        f.run_sweeps(2)
        assert (f.get_memberships(0) == m.get_memberships(c)).all(), c
        f.close()
    m.close()


def test_marginalize_and_the_cli_run_reshuffles_and_report_the_acceptance():
    rowptr, col, na, nb = O.load_graph("n_1000")
    n, chains, seed = na + nb, 8, 5
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    labels0 = O.contiguous_labels(na, nb, 3, 3)

    def model():
        m = B.BlockModel(labels0, syn.types_vector(na, nb), 6, 3, 3, 1.0, (rowptr, col), n_chains=chains, seed=seed)
        m.shuffle_bisbm()
        return m
    m = model()
    labels, counts = B.marginalize(m, 10, 3, 2, align=True, reshuffles=2)
    assert m.reshuffle_stats["proposed"] == 2 * 4 * chains and 0 <= m.reshuffle_stats["accepted"] <= m.reshuffle_stats["proposed"]
    assert (m.reshuffles_total() == 8).all() and counts.sum() == 3 * chains * n
    m2 = model()  # ... which is the Python calls
    m2.run_sweeps(10)
    m2.reshuffle(2, 3, 1.0)
    m2.marginals_reset()
    m2.marginals_set_alignment(True)
    for _ in range(3):
        m2.run_sweeps(2)
        m2.reshuffle(2, 3, 1.0)
        m2.marginals_accumulate(None)
    assert (counts == m2.marginals_get()).all()
    with pytest.raises(ValueError):
        B.marginalize(m2, 1, 1, 1, tempering=[1.0, 2.0], reshuffles=2)
    sizes = [str(x) for x in np.bincount(labels0)]
    base = [cli, "-e", el, "-y", str(na), str(nb), "-z", "3", "3", "-n", *sizes, "-r", "-d", str(seed), "--rng", "philox", "--chains", str(chains)]
    r = subprocess.run(base + ["-b", str(10 * n), "-t", str(6 * n), "-f", str(2 * n), "--marginalize", "--align", "--reshuffle", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout == B.output_vec(labels, stream=open(os.devnull, "w"))
    assert "reshuffle: %d of %d pair reshuffle(s) accepted (3 scan(s))" % (m.reshuffle_stats["accepted"], m.reshuffle_stats["proposed"]) in r.stderr
    for x in (m, m2):
        x.close()


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "reshuffle.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "the running sum tracks the description length through every move" in r.stdout, r.stdout + r.stderr
