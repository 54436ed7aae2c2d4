"""GPU tests of the split and merge moves (include/bisbm.h, "Split and merge moves").

The replay walks the moves of one chain on the host, one call per move: kind, block or pair, the launch bits and every uniform
from the oracle's Philox with purpose 11; every evaluated step's dS from a one-chain helper handle of the shape the division has
(bisbm_conditionals_accumulate with KEEP_LAST: the device's own rows); merge_dS from that helper's block state through
distributed.numpy_split_merge_dS with the oracle's lgamma, the device's log_q and the library's shape term; exp and log from the
device's probes; the choice, the factors and the acceptance from distributed.numpy_split_merge_* (tests/test_split_merge.py ties
those to literal loops and to exact detailed balance).  Labels, shapes and the block state are integers; Q, dS and the running
sum of dS are compared on bit patterns."""
import importlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_gpu_heatbath import _GRAPHS, _assert_state_is_a_rebuild, _bits, _case, _model, _refused
from test_tempering import philox, u53

B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SEED = 21
FIRST_ID = 5
PURPOSE = B.PHILOX_PURPOSE_SPLIT_MERGE
SEEN = {(k, a): 0 for k in (B.SM_SPLIT, B.SM_MERGE) for a in (True, False)}  # evaluated moves over all replays: (kind, accepted)


@pytest.fixture(autouse=True)
def _every_launch_keeps_its_own_sum(monkeypatch):
    """the MH sweeps of these tests keep the sum of their own dS values (tests/test_gpu_heatbath.py does the same)"""
    monkeypatch.setenv("BISBM_KEEP_SUM", "1")


def _draw(seed, gid, j, k):
    return philox(seed, gid, PURPOSE, (j << 32) | k)


def _lgamma(i):
    return float(O.lib().orc_lgamma_fast(int(i)))


class _Helpers:
    """one-chain handles, one per shape, that return the device's conditional rows and block state of given labels"""

    def __init__(self, name, beta):
        self.name, self.beta, self.by_shape = name, beta, {}

    def at(self, ka, kb, lab):
        (rowptr, col), na, nb, _, _, eps = _case(self.name)
        if (ka, kb) not in self.by_shape:
            m = B.BlockModel(lab.astype(np.uint32), syn.types_vector(na, nb), ka + kb, ka, kb, eps, (rowptr, col), n_chains=1, seed=SEED)
            m.conditionals_set(None, self.beta, keep_last=True)
            self.by_shape[(ka, kb)] = [m, None]
        return self.by_shape[(ka, kb)]

    def dS(self, ka, kb, lab, v, o_loc):
        h = self.at(ka, kb, lab)
        if h[1] is None or not (h[1] == lab).all():
            h[0].set_memberships(lab.astype(np.uint32))
            h[0].init_bisbm()
            h[0].conditionals_accumulate()
            h[1] = lab.copy()
        return float(h[0].conditionals_last(v)[0][0][o_loc])

    def state(self, ka, kb, lab):
        h = self.at(ka, kb, lab)
        h[0].set_memberships(lab.astype(np.uint32))
        h[0].init_bisbm()
        h[1] = None
        return h[0].get_m(0), h[0].get_m_r(0), h[0].get_n_r(0), h[0].get_eta_rk_(0)

    def close(self):
        for m, _ in self.by_shape.values():
            m.close()


def _merge_dS(m, helpers, ka, kb, lab, h, a, t):
    """merge_dS of blocks h and a of the division `lab` of shape (ka, kb) through the host model, on the device's numbers"""
    M_, m_r, n_r, eta = helpers.state(ka, kb, lab)
    oth = slice(0, ka) if t else slice(ka, ka + kb)
    T_div, T_mer = m.split_merge_shape_term(ka, kb), m.split_merge_shape_term(ka - (1 - t), kb - t)
    log_q = lambda n, k: float(m.debug_log_q([n], [k])[0])
    return D.numpy_split_merge_dS(M_[h, oth], M_[a, oth], eta[h], eta[a], m_r[h], m_r[a], n_r[h], n_r[a], T_mer, T_div, _lgamma, log_q)


def _replay_move(m, c, gid, name, helpers, scans, beta, k_min=(1, 1), k_max=None, seed=SEED):
    """One move of every chain on the device, chain c replayed on the host; asserts everything the two share and returns what the
    callers assert their edge on."""
    (rowptr, col), na, nb, _, _, eps = _case(name)
    ka, kb = m.ka_kb(c)
    K = ka + kb
    lab = m.get_memberships(c).astype(np.int64)
    cum, S0 = m.get_entropy()[c], m.entropy()[c]
    tot0 = m.split_merge_total()[c].astype(np.int64)
    j = int(tot0[0] + tot0[2])
    before = (lab.copy(), m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c))
    exp = lambda x: m.debug_exp([float(x)])[0]
    log = lambda x: m.debug_log([float(x)])[0]
    kmax_eff = k_max if k_max is not None else (min(na, 127), min(nb, 127))
    accepted_gpu = m.split_merge(1, scans, beta, k_min, k_max)
    got = m.split_merge_last()[c]
    X0, U = _draw(seed, gid, j, 0), _draw(seed, gid, j, 1)
    u_acc = u53(U[0], U[1])
    kind, t, r, s, refused = D.numpy_split_merge_choice(X0[0], X0[1], ka, kb, k_min, kmax_eff, size_of=lambda g: int((lab == g).sum()))
    info = {"kind": kind, "type": t, "r": r, "s": s, "refused": refused, "accepted": False, "dead": False, "not_free_stayed": 0, "M": 0}
    assert (got["kind"], got["type"], got["r"], got["s"], got["refused"]) == (kind, t, r, s, refused), (got, kind, t, r, s, refused)
    assert got["u_acc"] == u_acc and got["before"] == (ka, kb)
    tot1 = m.split_merge_total()[c].astype(np.int64)
    assert (tot1 - tot0).tolist() == [kind == 0, got["accepted"] and kind == 0, kind == 1, got["accepted"] and kind == 1]
    if refused:
        assert not got["accepted"] and got["after"] == (ka, kb) and got["A"] == 0.0 and got["lnA"] == -np.inf and got["dS"] == 0.0
        assert got["M"] == (int((lab == r).sum()) if refused == B.SM_SINGLETON else 0)
        new_lab, ka2, kb2, dS = lab, ka, kb, 0.0
    else:
        own0 = t * ka
        if kind == B.SM_SPLIT:
            # the division lives in the numbering of the accepted split: the spare is label s, type-b labels one up for type a
            members = np.flatnonzero(lab == r)
            work, _, _ = D.numpy_split_merge_renumber(lab, 0, t, r, s, ka, kb, away_nodes=[])
            wka, wkb, home, away_l = ka + (1 - t), kb + t, r, s
        else:
            members = np.flatnonzero((lab == r) | (lab == s))
            work, wka, wkb = lab.copy(), ka, kb
            home, away_mask = D.numpy_split_merge_roles(lab[members])
            away_l = s if home == r else r
            mdS = _merge_dS(m, helpers, ka, kb, lab, home, away_l, t)
        M, W = len(members), (len(members) + 127) >> 7
        info["M"] = M
        assert got["M"] == M and M >= 2
        bits = [(_draw(seed, gid, j, 2 + (i >> 7))[(i >> 5) & 3] >> (i & 31)) & 1 for i in range(M)]
        away = D.numpy_split_merge_launch(bits)
        work[members] = np.where(away, away_l, home)

        def scan(scan_t=None, forced=None):
            factors = []
            for i in range(1, M):
                v = members[i]
                cur = int(work[v])
                o = away_l if cur == home else home
                free = int((work == cur).sum()) > 1
                dS_o = helpers.dS(wka, wkb, work, v, o - t * wka) if free else None
                if forced is None:
                    X = _draw(seed, gid, j, 2 + W + scan_t * M + i)
                    to_home, f, dead = D.numpy_split_merge_step(dS_o, cur == home, free, beta, u=u53(X[0], X[1]), exp=exp)
                else:
                    to_home, f, dead = D.numpy_split_merge_step(dS_o, cur == home, free, beta, forced_home=int(forced[i]) == home, exp=exp)
                if not free and not dead:
                    info["not_free_stayed"] += 1
                if dead:
                    return factors, True
                factors.append(f)
                work[v] = home if to_home else away_l
            return factors, False
        for s_t in range(scans):
            scan(scan_t=s_t)
        info["L"] = work[members].copy()
        if kind == B.SM_SPLIT:
            f, _ = scan(scan_t=scans)
            q = D.numpy_reshuffle_q(f)
            mdS = _merge_dS(m, helpers, wka, wkb, work, home, away_l, t)
        else:
            f, dead = scan(forced=lab[members])
            q = (0.0, 0) if dead else D.numpy_reshuffle_q(f)
            info["dead"] = dead
        dS, lnA, A, _ = D.numpy_split_merge_accept(kind, mdS, q, beta, 0.0, ka, kb, t, exp=exp, log=log)
        assert got["q"][1] == q[1] and _bits(got["q"][0]) == _bits(q[0]), (got, q)
        assert _bits(got["dS"]) == _bits(dS), (got, dS)
        assert got["lnA"] == lnA or abs(got["lnA"] - lnA) <= 1e-12 * max(1.0, abs(lnA)), (got["lnA"], lnA)
        assert got["A"] == A or abs(got["A"] - A) <= 1e-12 * abs(A), (got["A"], A)
        assert got["accepted"] == (u_acc < got["A"])
        if got["accepted"]:
            if kind == B.SM_SPLIT:
                new_lab, ka2, kb2 = work, wka, wkb
            else:
                new_lab, ka2, kb2 = D.numpy_split_merge_renumber(lab, 1, t, r, s, ka, kb)
        else:
            new_lab, ka2, kb2, dS = lab, ka, kb, 0.0
        info["accepted"] = got["accepted"]
        SEEN[(kind, bool(got["accepted"]))] += 1
    assert got["after"] == (ka2, kb2) == m.ka_kb(c)
    assert (m.get_memberships(c) == new_lab).all()
    assert int(accepted_gpu[c]) == int(info["accepted"])
    if info["accepted"]:
        assert _bits(m.get_entropy()[c]) == _bits(cum + dS)
        for got_x, want_x in zip((m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c)), helpers.state(ka2, kb2, new_lab)):
            assert (got_x == want_x).all()
        S1 = m.entropy()[c]
        assert abs((S1 - S0) - dS) <= 1e-9 * abs(S0), (S1 - S0, dS)
    else:  # a rejection, or a refusal: everything to the bit
        assert _bits(m.get_entropy()[c]) == _bits(cum)
        for x, y in zip(before, (m.get_memberships(c), m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c))):
            assert (x == y).all()
    return info


def _replay(name, moves, scans, beta=1.0, sweeps=3, labels=None, first=FIRST_ID, k_min=(1, 1), k_max=None):
    """the last chain of a three-chain handle with a non-zero first chain id"""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    chains = 3
    m = _model(name, chains, first_chain_id=first, labels=labels)
    if labels is None:
        m.shuffle_bisbm()
        m.run_sweeps(sweeps)
    else:
        m.init_bisbm()
    helpers = _Helpers(name, beta)
    out = [_replay_move(m, chains - 1, first + chains - 1, name, helpers, scans, beta, k_min, k_max) for _ in range(moves)]
    for other in range(chains - 1):  # (the other chains ran too, and are consistent)
        _assert_state_is_a_rebuild(m, rowptr, col, other)
    print("%s: %d move(s), %d scan(s): %s" % (name, moves, scans, [(x["kind"], x["type"], x["r"], x["s"], x["M"], x["refused"], x["accepted"]) for x in out]))
    helpers.close()
    m.close()
    return out


# ------------------------------------------------------------------------------------------------------- 1. exact replay
@pytest.mark.parametrize("scans", [0, 2])
def test_moves_on_the_tiny_graph_are_the_host_replay(scans):
    """3 + 2 blocks over 12 + 9 nodes at beta = 0.3, where both kinds are accepted often: ten moves through several shapes"""
    out = _replay("tiny", 10, scans, beta=0.3)
    assert any(x["accepted"] for x in out)


def test_a_second_chunk_of_members_hubs_and_isolated_nodes_are_the_host_replay():
    """5 + 7 blocks over 300 + 200 nodes: a merge of type a has about 120 members -- a second chunk of 64 --, the hubs' rows run
    past the 64 neighbour labels a header parks, the isolated nodes have empty lists, eta rows of 150 degrees enter merge_dS"""
    out = _replay("hubs_isolated", 4, 1)
    assert max(x["M"] for x in out) > 64, [x["M"] for x in out]


def test_a_list_longer_than_one_wave_is_the_host_replay():
    """3 + 100 blocks and a type-a hub of some 610 neighbours: merge_dS walks 100 (and one spare) blocks of the other type in two
    chunks of lanes and 611 degrees in ten.  The first chain id is chosen so that the chain's move 0 is of type a."""
    name = "hb_long_list"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    first = next(f for f in range(1, 4000) if D.numpy_split_merge_choice(*_draw(SEED, f + 2, 0, 0)[:2], ka, kb)[1] == 0)
    out = _replay(name, 1, 1, first=first)
    assert out[0]["type"] == 0 and not out[0]["refused"] and out[0]["M"] > 64


def test_a_block_of_one_node_the_member_that_is_not_free_and_the_certain_rejection():
    """A start built by hand on the tiny graph: the last node of each type sits alone in the last block of its type.  A split of
    that block is refused as a singleton; a merge with it whose launch puts another member away alone either keeps a member that
    is not free (factor 1.0) or forces one out of a block it is alone in (Q_rev = 0, a certain rejection)."""
    name = "tiny"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    lab = O.contiguous_labels(na, nb, ka, kb).astype(np.int64)
    lab[:na][lab[:na] == ka - 1] = ka - 2
    lab[na - 1] = ka - 1
    lab[na:][lab[na:] == ka + kb - 1] = ka + kb - 2
    lab[na + nb - 1] = ka + kb - 1
    singleton = stayed = died = 0
    for first in range(1, 60):
        kind, t, r, s, _ = D.numpy_split_merge_choice(*_draw(SEED, first + 2, 0, 0)[:2], ka, kb)
        last = (ka - 1, ka + kb - 1)[t]
        if not ((kind == B.SM_SPLIT and r == last) or (kind == B.SM_MERGE and s == last)):
            continue
        out = _replay(name, 1, 0, labels=lab.astype(np.uint32), first=first)[0]
        singleton += out["refused"] == B.SM_SINGLETON
        stayed += out["not_free_stayed"] > 0
        died += out["dead"]
        assert not (out["dead"] and out["accepted"])
        if singleton and stayed and died:
            break
    assert singleton > 0 and stayed > 0 and died > 0, (singleton, stayed, died)


def test_refusals_at_k_max_and_k_min_leave_everything_alone():
    name = "tiny"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    out = _replay(name, 6, 1, k_min=(ka, kb), k_max=(ka, kb))
    assert all(x["refused"] in (B.SM_AT_K_MAX, B.SM_AT_K_MIN) for x in out)
    assert {x["refused"] for x in out} == {B.SM_AT_K_MAX, B.SM_AT_K_MIN}, [x["refused"] for x in out]


def test_the_replays_saw_accepted_and_rejected_splits_and_merges():
    """a module that passed on rejections alone would have checked no accepted state (run on its own, this test replays the tiny
    graph first)"""
    if not all(SEEN.values()):
        _replay("tiny", 16, 1, beta=0.3)
    assert all(v > 0 for v in SEEN.values()), SEEN


# ------------------------------------------------------------------------------------------- 1b. the byte-label edge
EDGE_NA, EDGE_NB = 262, 264
EDGE_K_MAX = (127, 127)


def _edge_case(ka, kb):
    """262 + 264 nodes, 2400 edges and a hub of some 600 (node 0), known to _case under a name per creation shape; the start by
    hand: block 0 of each type holds the type's first nodes (12 at 126 + 127 blocks), every other block two nodes in id order"""
    name = "sm_byte_edge_%d_%d" % (ka, kb)
    if name not in _GRAPHS:
        graph = next((g[0] for k, g in _GRAPHS.items() if k.startswith("sm_byte_edge_")), None)
        _GRAPHS[name] = (graph or cases.random_graph(11, EDGE_NA, EDGE_NB, 2400, 126, 127, 1, 0), EDGE_NA, EDGE_NB, ka, kb, 1.0)
    la = np.repeat(np.arange(ka), [EDGE_NA - 2 * (ka - 1)] + [2] * (ka - 1))
    lb = ka + np.repeat(np.arange(kb), [EDGE_NB - 2 * (kb - 1)] + [2] * (kb - 1))
    return name, np.concatenate([la, lb]).astype(np.uint32)


def _edge_first(ka, kb, lab, want, u_below=0.25):
    """the lowest first chain id at which move 0 of the replayed chain (the last of three) is the wanted kind and choice, with
    a u_acc below u_below; the kind and the choice from the oracle's Philox, as the device draws them"""
    size_of = lambda g: int((lab == g).sum())
    for first in range(1, 1 << 20):
        x = _draw(SEED, first + 2, 0, 0)
        if want(*D.numpy_split_merge_choice(x[0], x[1], ka, kb, (1, 1), EDGE_K_MAX, size_of=size_of)) and u53(*_draw(SEED, first + 2, 0, 1)[:2]) < u_below:
            return first
    raise AssertionError("no chain id draws the wanted move")


def _replay_edge(ka, kb, want, beta, scans=1):
    """one move of three chains from the start by hand, the last chain replayed on the host; afterwards every chain's state is a
    rebuild from its labels and its labels are contiguous per type"""
    name, lab = _edge_case(ka, kb)
    (rowptr, col), na, nb, _, _, eps = _case(name)
    # the padded launch holds (ka + 1) x (kb + 1) blocks: its quadrant fits the LDS, its eta (K + 2 rows of max_degree + 1 words)
    # is past what the plan keeps there, so the kernel's instantiation with eta in HBM runs (as test_eta_outside_the_lds asserts)
    deg_max = int(np.diff(rowptr.astype(np.int64)).max())
    assert 4 * (ka + 1) * (kb + 2) <= 160 * 1024 and 4 * (ka + kb + 2) * (deg_max + 1) > 40 * 1024
    first = _edge_first(ka, kb, lab, want)
    chains = 3
    m = _model(name, chains, first_chain_id=first, labels=lab)
    m.init_bisbm()
    helpers = _Helpers(name, beta)
    out = _replay_move(m, chains - 1, first + chains - 1, name, helpers, scans, beta, (1, 1), EDGE_K_MAX)
    print("%s: first chain id %d: %s; all chains: %s" % (name, first, out, [(r["kind"], r["type"], r["r"], r["s"], r["M"], r["refused"], r["accepted"]) for r in m.split_merge_last()]))
    for c in range(chains):
        _assert_state_is_a_rebuild(m, rowptr, col, c)
        a, b = m.ka_kb(c)
        got = m.get_memberships(c)
        assert sorted(set(got[:na].tolist())) == list(range(a)) and sorted(set(got[na:].tolist())) == list(range(a, a + b)), c
        assert a <= 127 and b <= 127 and int(got.max()) == a + b - 1
    helpers.close()
    m.close()
    return out


def test_a_split_to_127_plus_127_blocks_is_the_host_replay():
    """126 + 127 blocks, a split of the 12 nodes of type-a block 0 at beta = 0.05: with K = 253 the move carries
    log(K / N(shape after)) = log(253 / 16002) = -4.1 and -ln Q_fwd of 11 free members is about +7, so it is accepted.  The
    chain ends at 127 + 127 blocks with labels up to 253.  Observed on an MI355X: first chain id 3294, u_acc = 0.138, the split of 12 members accepted (the two
    other chains proposed merges of four members at K = 253: one accepted, one rejected)."""
    out = _replay_edge(126, 127, lambda kind, t, r, s, refused: kind == B.SM_SPLIT and r == 0 and not refused, 0.05)
    assert out["accepted"] and out["M"] == 12 and out["type"] == 0


def test_a_merge_into_the_last_label_at_127_plus_127_blocks_is_the_host_replay():
    """127 + 127 blocks: the padded launch has 128 + 128, the spare of type b is label 255.  A type-b merge whose s is the last
    label, 253 -- label 254 of the launch, the upper of the two labels the regrouping takes out -- of two blocks of two nodes.
    Observed on an MI355X: first chain id 1134, blocks 238 and 253, accepted, as were the type-b merges of the two other chains."""
    out = _replay_edge(127, 127, lambda kind, t, r, s, refused: kind == B.SM_MERGE and t == 1 and s == 253 and r > 127 and not refused, 0.05)
    assert out["accepted"] and out["M"] == 4 and (out["type"], out["s"]) == (1, 253)


def test_a_type_a_merge_at_127_plus_127_blocks_is_the_host_replay():
    """every type-b label moves down with the merged type-a block's.  Observed on an MI355X: first chain id 33, blocks 7 and 89, accepted."""
    out = _replay_edge(127, 127, lambda kind, t, r, s, refused: kind == B.SM_MERGE and t == 0 and r > 0 and not refused, 0.05)
    assert out["accepted"] and out["M"] == 4 and out["type"] == 0


def test_a_split_at_127_plus_127_blocks_is_refused_at_k_max():
    out = _replay_edge(127, 127, lambda kind, t, r, s, refused: kind == B.SM_SPLIT, 0.05)
    assert out["refused"] == B.SM_AT_K_MAX and not out["accepted"]


# --------------------------------------------------------------------------------------------------------- 2. regrouping
def _run(m, rounds=5):
    m.shuffle_bisbm()
    acc = np.zeros(m.n_chains, dtype=np.uint64)
    recs = []
    for _ in range(rounds):
        acc += m.split_merge(2, 1, 0.3, (1, 1), (4, 4))
        recs.append(m.split_merge_last())
        m.run_sweeps(1)
    return [m.get_memberships(c) for c in range(m.n_chains)], [m.ka_kb(c) for c in range(m.n_chains)], acc, m.get_entropy(), recs, m.split_merge_total()


def _same_records(a, b):
    norm = lambda x: {k: (_bits(v).tolist() if isinstance(v, float) else v) for k, v in x.items()}
    return all(norm(x) == norm(y) for x, y in zip(a, b))


def test_chains_that_reach_a_shape_join_its_group_and_every_state_is_a_rebuild():
    name, chains = "tiny", 48
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    m = _model(name, chains, first_chain_id=3)
    labels, shapes, acc, cum, recs, tot = _run(m)
    assert acc.sum() > 0 and len(set(shapes)) > 1
    groups = m.chain_groups()
    by_shape = {}
    for c in range(chains):
        by_shape.setdefault(shapes[c], set()).add(int(groups[c]))
        _assert_state_is_a_rebuild(m, rowptr, col, c)
        lab = labels[c]
        assert sorted(set(lab[:na].tolist())) == list(range(shapes[c][0]))  # no block empty, labels contiguous per type
        assert sorted(set(lab[na:].tolist())) == list(range(shapes[c][0], sum(shapes[c])))
    assert all(len(g) == 1 for g in by_shape.values()), by_shape  # one group per shape
    assert len({next(iter(g)) for g in by_shape.values()}) == len(by_shape)
    assert (tot[:, 0] + tot[:, 2] == 10).all() and (tot[:, 1] + tot[:, 3] == acc).all()
    # the description length follows the running sum through moves and sweeps, across all regroupings
    o_S = m.entropy()
    for c in (0, chains - 1):
        o = O.OracleModel(rowptr, col, na, nb, shapes[c][0], shapes[c][1], eps, labels[c])
        o.init_bisbm()
        assert abs(o.entropy() - o_S[c]) <= 1e-9 * abs(o_S[c])
    m.close()


def test_device_entries_behind_one_handle_give_one_handles_bits():
    name = "tiny"
    one = _model(name, 6, first_chain_id=3)
    labels, shapes, acc, cum, recs, tot = _run(one)
    for entries in (2, 3):
        many = _model(name, 6, first_chain_id=3, devices=[0] * entries)
        l2, s2, a2, c2, r2, t2 = _run(many)
        assert all((x == y).all() for x, y in zip(labels, l2)) and shapes == s2 and (acc == a2).all() and (_bits(cum) == _bits(c2)).all(), entries
        assert all(_same_records(x, y) for x, y in zip(recs, r2)) and (tot == t2).all()
        many.close()
    one.close()


# ------------------------------------------------------------------------------------------------ 3. refusals, counters
def test_refusals():
    name = "tiny"
    m = _model(name, 4)
    assert "bisbm_init" in _refused(lambda: m.split_merge(1), B.BISBM_ERR_STATE)  # (labels set, block state not built)
    m.shuffle_bisbm()
    _refused(lambda: m.split_merge_last(), B.BISBM_ERR_STATE)  # (no move on record yet)
    assert (m.split_merge_total() == 0).all()
    state = [m.get_memberships(c) for c in range(4)], m.get_entropy()
    for beta in (float("nan"), 0.0, -1.0, float("inf")):
        assert "beta" in _refused(lambda: m.split_merge(1, 1, beta), B.BISBM_ERR_INVALID_ARG)
    assert "k_min" in _refused(lambda: m.split_merge(1, k_min=(0, 1)), B.BISBM_ERR_INVALID_ARG)
    assert "k_min" in _refused(lambda: m.split_merge(1, k_min=(3, 1), k_max=(2, 5)), B.BISBM_ERR_INVALID_ARG)
    assert "254" in _refused(lambda: m.split_merge(1, k_max=(200, 100)), B.BISBM_ERR_INVALID_ARG)
    m.set_tempering([1.0, 2.0])
    assert "replica exchange" in _refused(lambda: m.split_merge(1), B.BISBM_ERR_STATE)
    m.set_tempering(None)
    m.clamp([0, 1])
    assert "clamped" in _refused(lambda: m.split_merge(1), B.BISBM_ERR_STATE)
    m.unclamp()
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    m.set_fields(np.zeros(na + nb, dtype=np.uint8), np.ones((1, ka + kb)))
    assert "fields" in _refused(lambda: m.split_merge(1), B.BISBM_ERR_STATE)
    m.clear_fields()
    held = _model(name, 2)  # (contiguous labels in both chains: node 0 sits in block 0, and its class allows nothing else of type a)
    held.init_bisbm()
    cls = np.zeros(na + nb, dtype=np.uint8)
    cls[0] = 1
    allowed = np.ones((2, ka + kb), dtype=np.uint8)
    allowed[1, 1:ka] = 0
    held.constrain(cls, allowed)
    assert "constraints" in _refused(lambda: held.split_merge(1), B.BISBM_ERR_STATE)
    held.close()
    m.population_run([1.0, 0.9], 1)
    assert "population" in _refused(lambda: m.split_merge(1), B.BISBM_ERR_STATE)
    m.population_reset()
    state = [m.get_memberships(c) for c in range(4)], m.get_entropy()
    assert (m.split_merge(0) == 0).all()  # moves = 0: a no-op that returns OK
    after = [m.get_memberships(c) for c in range(4)], m.get_entropy()
    assert all((x == y).all() for x, y in zip(state[0], after[0])) and (_bits(state[1]) == _bits(after[1])).all()
    assert (m.split_merge_total() == 0).all()
    assert B.lib().bisbm_split_merge_run(m._h, 1, 1, 1.0, None, None, None) == B.BISBM_OK  # (every pointer may be NULL)
    assert (m.split_merge_total()[:, [0, 2]].sum(axis=1) == 1).all()
    m.close()
    compat = _model(name, 2, rng="mt19937-compat")
    compat.shuffle_bisbm()
    assert "MT19937" in _refused(lambda: compat.split_merge(1), B.BISBM_ERR_UNSUPPORTED)
    compat.close()
    wide = _model("wide_labels", 2)
    wide.init_bisbm()
    assert "byte labels" in _refused(lambda: wide.split_merge(1), B.BISBM_ERR_UNSUPPORTED)
    wide.close()


def test_counters_and_what_a_call_leaves_alone():
    name, chains = "hubs_isolated", 4
    m = _model(name, chains)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    counts = m.last_counts()
    labels = [m.get_memberships(c) for c in range(chains)]
    m.split_merge(1, 0, 1.0, (5, 7), (5, 7))  # (every proposal refused: the labels stay)
    first = m.split_merge_last()
    assert all(r["refused"] in (B.SM_AT_K_MAX, B.SM_AT_K_MIN) for r in first)
    m.split_merge(1, 0, 1.0, (5, 7), (5, 7))
    second = m.split_merge_last()
    tot = m.split_merge_total()
    assert (tot[:, 0] + tot[:, 2] == 2).all() and (tot[:, 1] + tot[:, 3] == 0).all()
    # the same state, another move: the second call does not replay the draws of the first
    assert all(a["u_acc"] != b["u_acc"] for a, b in zip(first, second))
    assert all((x == y).all() for x, y in zip(counts, m.last_counts()))  # (last_counts are the MH sweeps' still)
    assert (m.reshuffles_total() == 0).all()
    # sweeps_total has not moved: the next MH sweeps are those of a fresh handle that ran two sweeps and took these labels
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


def test_a_moved_chain_keeps_its_scalars_the_next_sweeps_are_a_fresh_handles():
    """after accepted moves -- the chain has been copied into another group, some chains more than once -- sweeps_total and the
    chain's global id are what they were: the next two MH sweeps equal those of a fresh one-chain handle of the chain's new shape
    that ran two sweeps and then took these labels; the running sum has followed the description length all the way"""
    name, chains = "tiny", 6
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    m = _model(name, chains, first_chain_id=3)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    S0, cum0 = m.entropy(), m.get_entropy()
    acc = np.zeros(chains, dtype=np.uint64)
    for _ in range(6):
        acc += m.split_merge(1, 1, 0.3, (1, 1), (4, 4))
    moved = [c for c in range(chains) if acc[c] > 0]
    assert moved
    S1, cum1 = m.entropy(), m.get_entropy()
    assert (np.abs((S1 - S0) - (cum1 - cum0)) <= 1e-9 * np.abs(S0)).all()
    assert (m.last_counts()[1] == 2).all()  # (last_counts are the MH sweeps' still)
    labels = [m.get_memberships(c) for c in range(chains)]
    shapes = [m.ka_kb(c) for c in range(chains)]
    m.run_sweeps(2)
    for c in moved[:2] + [c for c in range(chains) if c not in moved][:1]:
        a, b = shapes[c]
        f = B.BlockModel(labels[c], syn.types_vector(na, nb), a + b, a, b, eps, (rowptr, col), n_chains=1, seed=SEED, first_chain_id=3 + c)
        f.init_bisbm()
        f.run_sweeps(2)
        f.set_memberships(labels[c])
        f.init_bisbm()
        f.run_sweeps(2)
        assert (f.get_memberships(0) == m.get_memberships(c)).all(), c
        f.close()
    m.close()


def test_the_cli_counts_the_shapes_as_marginalize_does(tmp_path):
    rowptr, col, na, nb = O.load_graph("n_1000")
    n, chains, seed = na + nb, 8, 5
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    labels0 = O.contiguous_labels(na, nb, 3, 3)
    m = B.BlockModel(labels0, syn.types_vector(na, nb), 6, 3, 3, 1.0, (rowptr, col), n_chains=chains, seed=seed)
    m.shuffle_bisbm()
    shape_counts, best = B.marginalize(m, 4, 3, 2, split_merges=3, split_merge_scans=2, k_min=(1, 2), k_max=(8, 8))
    out = str(tmp_path / "shapes.txt")
    sizes = [str(x) for x in np.bincount(labels0)]
    r = subprocess.run([cli, "-e", el, "-y", str(na), str(nb), "-z", "3", "3", "-n", *sizes, "-r", "-d", str(seed), "--rng", "philox", "--chains", str(chains),
                        "-b", str(4 * n), "-t", str(6 * n), "-f", str(2 * n), "--marginalize", "--split_merge", "3", "--split_merge_scans", "2",
                        "--k_min", "1", "2", "--k_max", "8", "8", "--shape_counts", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rows = [line.split() for line in open(out).read().splitlines()]
    got = {(int(a), int(b)): (int(v), float(S)) for a, b, v, S in rows}
    assert [(int(a), int(b)) for a, b, _, _ in rows] == sorted(got)
    assert got == {shape: (shape_counts[shape], best[shape][0]) for shape in shape_counts}
    lowest = min(sorted(best), key=lambda shape: best[shape][0])
    assert r.stdout == B.output_vec(best[lowest][1], stream=open(os.devnull, "w"))
    assert "split_merge: %d of %d split / merge move(s) accepted (2 scan(s))" % (m.split_merge_stats["accepted"], m.split_merge_stats["proposed"]) in r.stderr
    m.close()


def test_marginalize_counts_the_shapes_and_keeps_the_numbering_free_sums():
    rowptr, col, na, nb = O.load_graph("n_1000")
    chains, seed = 8, 5

    def model():
        m = B.BlockModel(O.contiguous_labels(na, nb, 3, 3), syn.types_vector(na, nb), 6, 3, 3, 1.0, (rowptr, col), n_chains=chains, seed=seed)
        m.shuffle_bisbm()
        return m
    m = model()
    rng = np.random.default_rng(2)
    pairs = np.stack([rng.integers(0, na, 50), na + rng.integers(0, nb, 50)], axis=1)
    shape_counts, best, similar = B.marginalize(m, 4, 3, 2, split_merges=3, k_max=(8, 8), score_pairs=pairs, similar=([0, na], 5))
    assert sum(shape_counts.values()) == 3 * chains and set(best) == set(shape_counts)
    assert m.split_merge_stats["proposed"] == 3 * 4 * chains and 0 <= m.split_merge_stats["accepted"] <= m.split_merge_stats["proposed"]
    tot = m.split_merge_total()
    assert (tot[:, 0] + tot[:, 2] == 12).all() and tot[:, [1, 3]].sum() == m.split_merge_stats["accepted"]
    for (ka, kb), (S, lab) in best.items():
        o = O.OracleModel(rowptr, col, na, nb, ka, kb, 1.0, lab)
        o.init_bisbm()
        assert abs(o.entropy() - S) <= 1e-9 * abs(S)
    assert m.pair_scores()[1] == 3 * chains and similar[2] == 3 * chains
    m2 = model()  # ... which is the Python calls
    m2.run_sweeps(4)
    m2.split_merge(3, 3, 1.0, (1, 1), (8, 8))
    for _ in range(3):
        m2.run_sweeps(2)
        m2.split_merge(3, 3, 1.0, (1, 1), (8, 8))
    assert all((m.get_memberships(c) == m2.get_memberships(c)).all() and m.ka_kb(c) == m2.ka_kb(c) for c in range(chains))
    for kw in ({"align": True}, {"reshuffles": 2}, {"tempering": [1.0, 2.0]}, {"return_counts": True}):
        with pytest.raises(ValueError, match="split_merges"):
            B.marginalize(m2, 1, 1, 1, split_merges=2, **kw)
    for x in (m, m2):
        x.close()


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "block_counts.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "the running sum tracks the description length through every change of shape" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------- 4. stationary distribution
K_MAX = 3
_TARGET = {}


def _growth_strings(n, kmax):
    """every partition of n items into at most kmax blocks, as labels by first occurrence"""
    out = [[0]]
    for _ in range(n - 1):
        out = [p + [x] for p in out for x in range(min(max(p) + 1, kmax - 1) + 1)]
    return out


def _code(lab_a, lab_b):
    """canonical labels (by first occurrence within each type, local) -> integer"""
    code, seen = 0, {}
    for i, x in enumerate(lab_a):
        code += seen.setdefault(int(x), len(seen)) * 3 ** i
    seen = {}
    for i, x in enumerate(lab_b):
        code += seen.setdefault(int(x), len(seen)) * 3 ** (len(lab_a) + i)
    return code


def _exact_target():
    """the 14 884 partitions of the enumerable graph with at most three blocks per type: codes, shapes, S from the oracle, T"""
    if not _TARGET:
        rowptr, col = cases.enumerable_graph()
        na, nb, E = cases.ENUM_NA, cases.ENUM_NB, len(cases.ENUM_EDGES)
        parts = _growth_strings(na, K_MAX)
        assert len(parts) == 122
        lb = O.lib().orc_lbinom_fast
        models, codes, shapes, S, T = {}, [], [], [], []
        for pa in parts:
            ka = max(pa) + 1
            for pb in parts:
                kb = max(pb) + 1
                lab = np.array(pa + [ka + x for x in pb], dtype=np.uint32)
                if (ka, kb) not in models:
                    models[(ka, kb)] = O.OracleModel(rowptr, col, na, nb, ka, kb, cases.ENUM_EPS, lab)
                o = models[(ka, kb)]
                o.set_memberships(lab)
                o.init_bisbm()
                codes.append(_code(pa, pb))
                shapes.append((ka, kb))
                S.append(o.entropy())
                T.append((float(lb(ka * kb + E - 1, E)) + float(lb(na - 1, ka - 1))) + float(lb(nb - 1, kb - 1)))
        _TARGET.update(codes=np.array(codes), shapes=shapes, S=np.array(S), T=np.array(T))
        assert len(set(codes)) == 14884
    return _TARGET


def _shape_probs(weights, shapes):
    p = np.zeros((K_MAX, K_MAX))
    for w, (ka, kb) in zip(weights, shapes):
        p[ka - 1, kb - 1] += w
    return p / p.sum()


def _chi2_shapes(counts, probs):
    from scipy import stats
    e = probs * counts.sum()
    stat = float(((counts - e) ** 2 / e).sum())
    return stat, float(stats.chi2.sf(stat, counts.size - 1))


ISSUE_TABLE = np.array([[0.6589, 0.1792, 0.0420], [0.0776, 0.0216, 0.0061], [0.0101, 0.0034, 0.0011]])
ROUNDS = {1.0: 24, 0.6: 24}


@pytest.mark.parametrize("beta", [1.0, 0.6])
def test_chains_sample_the_block_counts_with_the_partition(beta):
    """32768 chains on the enumerable 6 + 6 graph from the shuffled 2 + 2 start (2.2 % of the target mass at beta = 1: chains that
    never leave it fail on their own), rounds of {one MH sweep, two moves with scans = 1}, k_min = (1, 1), k_max = (3, 3), against
    exp(-beta S) over the 14 884 unlabelled partitions from the oracle.  The shapes also against the target without the three
    shape terms and against the labelled target (an extra Ka! Kb!), which must both fail; at beta = 1 the partitions themselves.
    Rounds: 24 at both beta, chosen for at least 10 accepted shape changes per chain.  Observed on an MI355X with these 24 rounds:
    beta = 1: 15.4 accepted shape changes per chain (splits 227460 of 786107 proposed, 28.9 %; merges 278581 of 786757, 35.4 %;
    refused proposals count as proposed), shapes chi2 = 10.0 on 8 dof (p = 0.27), partitions chi2 = 108.3 on 145 dof (p = 0.99);
    beta = 0.6: 22.5 per chain (splits 366765 of 786107, 46.7 %; merges 370778 of 786757, 47.1 %), shapes chi2 = 11.6 (p = 0.17)."""
    tg = _exact_target()
    S, T, shapes = tg["S"], tg["T"], tg["shapes"]
    w = np.exp(-beta * (S - S.min()))
    prob = w / w.sum()
    exact = _shape_probs(w, shapes)
    if beta == 1.0:
        assert np.abs(exact - ISSUE_TABLE).max() < 6e-5, exact  # (the table of the issue, four decimals)
        start = sum(p for p, s in zip(prob, shapes) if s == (2, 2))
        assert 0.02 < start < 0.024
    else:
        assert abs(exact.min() - 0.049) < 5e-4 and abs(exact.max() - 0.179) < 5e-4, exact  # (the issue's figures, three decimals)
    S_no = S - T
    no_shape = _shape_probs(np.exp(-beta * (S_no - S_no.min())), shapes)
    labelled = _shape_probs(w * np.array([math.factorial(a) * math.factorial(b) for a, b in shapes]), shapes)
    if beta == 1.0:
        assert abs(no_shape[2, 2] - 0.90) < 0.01 and abs(labelled[0, 0] - 0.38) < 0.01, (no_shape, labelled)

    rowptr, col = cases.enumerable_graph()
    na, nb = cases.ENUM_NA, cases.ENUM_NB
    chains, rounds = 32768, ROUNDS[beta]
    g = B.BlockModel(O.contiguous_labels(na, nb, 2, 2), syn.types_vector(na, nb), 4, 2, 2, cases.ENUM_EPS, (rowptr, col),
                     n_chains=chains, rng="philox", seed=4242)
    g.shuffle_bisbm()
    accepted = np.zeros(chains, dtype=np.uint64)
    for _ in range(rounds):
        g.run_sweeps(1, temperature=1.0 / beta)
        accepted += g.split_merge(2, 1, beta, (1, 1), (K_MAX, K_MAX))
    tot = g.split_merge_total().sum(axis=0)
    per_chain = float(accepted.sum()) / chains
    got_shapes = [g.ka_kb(c) for c in range(chains)]
    counts = np.zeros((K_MAX, K_MAX))
    for ka, kb in got_shapes:
        counts[ka - 1, kb - 1] += 1
    groups = g.chain_groups()
    assert len(set(groups.tolist())) == len(set(got_shapes)) <= 9
    stat, p = _chi2_shapes(counts, exact)
    p_no, p_lab = _chi2_shapes(counts, no_shape)[1], _chi2_shapes(counts, labelled)[1]
    print("split/merge, beta = %g: %d rounds, %.1f accepted shape changes per chain (splits %d of %d, merges %d of %d); shapes: chi2 = %.1f on 8 dof, "
          "p = %.3g; without the shape terms p = %.3g; labelled target p = %.3g" % (beta, rounds, per_chain, tot[1], tot[0], tot[3], tot[2], stat, p, p_no, p_lab))
    print(np.round(counts / chains, 4))
    assert per_chain >= 10.0, "too few accepted shape changes per chain: raise the rounds"
    assert p > 1e-3, (stat, p)
    assert p_no < 1e-6 and p_lab < 1e-6
    if beta == 1.0:
        big = prob * chains >= 8.0
        assert prob[~big].sum() <= 0.06  # (from the exact distribution: the share of the pooled bin)
        codes = np.array([_code(lab[:na], lab[na:]) for lab in (g.get_memberships(c) for c in range(chains))])
        stat2, dof2, p2 = cases.chi_square(codes, tg["codes"], prob, min_expected=8.0)
        print("partitions: %d states above the threshold, %.1f %% pooled; chi2 = %.1f on %d dof, p = %.3g" % (big.sum(), 100 * prob[~big].sum(), stat2, dof2, p2))
        assert p2 > 1e-3, (stat2, dof2, p2)
    g.close()
