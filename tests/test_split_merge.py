"""Split and merge moves (include/bisbm.h, "Split and merge moves") without a device: the host model
(distributed.numpy_split_merge_*, which the GPU tests hold the kernel to) against literal loops on hand-made inputs, merge_dS with
the shape terms against the oracle's description length at the two shapes, the exact detailed balance of the host model over all
25 partitions of a 3 + 3-node graph, and the binding."""
import ctypes as C
import importlib
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
W32 = 2 ** 32


def _lgamma(i):
    return float(O.lib().orc_lgamma_fast(int(i)))


def _log_q(n, k):
    return float(O.lib().orc_log_q(int(n), int(k)))


def _shape_term(E, na, nb, ka, kb):
    """T(ka, kb) of step 5 from the oracle's lbinom"""
    lb = O.lib().orc_lbinom_fast
    return (float(lb(ka * kb + E - 1, E)) + float(lb(na - 1, ka - 1))) + float(lb(nb - 1, kb - 1))


# ------------------------------------------------------------------------------------------------ kind, block and pair
def _word_for(index, count):
    """a 32-bit word y with (y * count) >> 32 == index"""
    return (index * W32 + count - 1) // count


@pytest.mark.parametrize("ka,kb", [(3, 2), (1, 4), (4, 1), (2, 2), (1, 1), (70, 3)])
def test_kind_block_and_pair_are_the_literal_enumeration(ka, kb):
    K = ka + kb
    pairs = [(t, r + t * ka, s + t * ka) for t, k in ((0, ka), (1, kb)) for r in range(k) for s in range(r + 1, k)]
    assert len(pairs) == D.numpy_split_merge_pairs(ka, kb)
    for b in range(K):  # an even first word: a split of block (y * K) >> 32
        for y in {_word_for(b, K), (_word_for(b + 1, K) - 1) % W32 if b + 1 < K else W32 - 1}:
            kind, t, r, s, refused = D.numpy_split_merge_choice(2 * 77, y, ka, kb)
            assert (kind, t, r, refused) == (0, int(b >= ka), b, 0) and s == (K if b >= ka else ka), (b, y)
    for i, (t, r, s) in enumerate(pairs):  # an odd first word: a merge of pair (y * N) >> 32
        assert D.numpy_split_merge_choice(2 * 77 + 1, _word_for(i, len(pairs)), ka, kb) == (1, t, r, s, 0)
    if not pairs:
        assert D.numpy_split_merge_choice(1, 12345, ka, kb) == (1, 0, 0, 0, B.SM_NO_PAIR)
    # only bit 0 of the first word is looked at
    assert D.numpy_split_merge_choice(0xfffffffe, 0, ka, kb)[0] == 0 and D.numpy_split_merge_choice(0x80000001, 0, ka, kb)[0] == 1


def test_refusals_at_k_min_and_k_max_and_of_a_singleton():
    ka, kb = 3, 2
    # a merge of a type at k_min is refused, the other type's is not; the pair is still the enumeration's
    assert D.numpy_split_merge_choice(1, 0, ka, kb, k_min=(3, 1)) == (1, 0, 0, 1, B.SM_AT_K_MIN)
    assert D.numpy_split_merge_choice(1, W32 - 1, ka, kb, k_min=(3, 1)) == (1, 1, 3, 4, 0)
    assert D.numpy_split_merge_choice(1, W32 - 1, ka, kb, k_min=(1, 2))[4] == B.SM_AT_K_MIN
    assert D.numpy_split_merge_choice(1, W32 - 1, ka, kb, k_min=(1, 3))[4] == B.SM_AT_K_MIN  # (a chain below k_min merges no further)
    # a split of a type at k_max
    assert D.numpy_split_merge_choice(0, 0, ka, kb, k_max=(3, 3)) == (0, 0, 0, 3, B.SM_AT_K_MAX)
    assert D.numpy_split_merge_choice(0, W32 - 1, ka, kb, k_max=(3, 3)) == (0, 1, 4, 5, 0)
    assert D.numpy_split_merge_choice(0, W32 - 1, ka, kb, k_max=(4, 2))[4] == B.SM_AT_K_MAX
    # a block of fewer than two nodes, tested after k_max
    sizes = {0: 1, 1: 5, 2: 2, 3: 1, 4: 7}
    assert D.numpy_split_merge_choice(0, 0, ka, kb, k_max=(4, 4), size_of=sizes.get)[4] == B.SM_SINGLETON
    assert D.numpy_split_merge_choice(0, 0, ka, kb, k_max=(3, 4), size_of=sizes.get)[4] == B.SM_AT_K_MAX
    assert D.numpy_split_merge_choice(0, _word_for(1, 5), ka, kb, k_max=(4, 4), size_of=sizes.get)[4] == 0
    assert D.numpy_split_merge_choice(0, _word_for(3, 5), ka, kb, k_max=(4, 4), size_of=sizes.get)[1:] == (1, 3, 5, B.SM_SINGLETON)
    # a merge with N = 0 is a refusal whatever k_min says
    assert D.numpy_split_merge_choice(1, 99, 1, 1, k_min=(1, 1))[4] == B.SM_NO_PAIR


# ------------------------------------------------------------------------------------------------------ roles and launch
def test_roles_go_by_the_lowest_member():
    assert D.numpy_split_merge_roles([4, 2, 4, 2, 2]) == (4, [False, True, False, True, True])
    assert D.numpy_split_merge_roles([2, 4, 2, 4, 4]) == (2, [False, True, False, True, True])  # (the same division, other labels)
    # every unordered division of M members into two non-empty parts has exactly one description with member 0 at home
    M = 5
    seen = set()
    for lab in itertools.product((7, 9), repeat=M):
        if len(set(lab)) == 2:
            seen.add(tuple(D.numpy_split_merge_roles(lab)[1]))
    assert len(seen) == 2 ** (M - 1) - 1 and all(not a[0] for a in seen)


def _literal_launch(bits):
    away = [False] * len(bits)
    for i in range(1, len(bits)):
        if bits[i]:
            away[i] = True
    if not any(away):
        away[len(bits) - 1] = True
    return away


def test_the_launch_fix_up():
    assert D.numpy_split_merge_launch([0, 0, 0, 0]) == [False, False, False, True]  # nobody away: the last member goes
    assert D.numpy_split_merge_launch([1, 0, 0, 0]) == [False, False, False, True]  # (member 0's bit is not looked at)
    assert D.numpy_split_merge_launch([1, 1, 1]) == [False, True, True]
    assert D.numpy_split_merge_launch([0, 0]) == [False, True] and D.numpy_split_merge_launch([1, 1]) == [False, True]
    rng = np.random.default_rng(5)
    for _ in range(200):
        bits = (rng.random(int(rng.integers(2, 12))) < rng.random()).astype(int).tolist()
        got = D.numpy_split_merge_launch(bits)
        assert got == _literal_launch(bits) and not got[0] and any(got)


# ---------------------------------------------------------------------------------------------------------------- the step
def _literal_step(dS_o, in_home, beta, u):
    mn = min(dS_o, 0.0)
    w_c, w_o = math.exp(-(beta * (0.0 - mn))), math.exp(-(beta * (dS_o - mn)))
    w_h, w_a = (w_c, w_o) if in_home else (w_o, w_c)
    Z = w_h + w_a
    return (u < w_h / Z), (w_h / Z if u < w_h / Z else w_a / Z)


def test_a_free_step_is_the_literal_step():
    rng = np.random.default_rng(7)
    for _ in range(300):
        dS_o, in_home, beta, u = float(rng.normal(0, 5)), bool(rng.integers(2)), float(rng.choice([1.0, 0.6])), float(rng.random())
        home, f, dead = D.numpy_split_merge_step(dS_o, in_home, True, beta, u=u, exp=lambda x: math.exp(float(x)))
        want = _literal_step(dS_o, in_home, beta, u)
        assert (home, dead) == (want[0], False) and f == want[1]
        # a forced step takes the factor of where it is sent
        for forced in (True, False):
            h2, f2, dead2 = D.numpy_split_merge_step(dS_o, in_home, True, beta, forced_home=forced, exp=lambda x: math.exp(float(x)))
            P_home = want[1] if want[0] else 1.0 - want[1]
            assert h2 == forced and not dead2 and abs(f2 - (P_home if forced else 1.0 - P_home)) <= 1e-15


def test_the_sole_member_of_away_is_not_free_and_forcing_it_home_kills_the_pass():
    assert D.numpy_split_merge_step(None, False, False, 1.0, u=0.3) == (False, 1.0, False)  # stays away, factor 1, no draw
    assert D.numpy_split_merge_step(None, False, False, 1.0, forced_home=False) == (False, 1.0, False)
    home, f, dead = D.numpy_split_merge_step(None, False, False, 1.0, forced_home=True)
    assert (home, f, dead) == (True, 0.0, True)
    assert D.numpy_reshuffle_q([0.5, f, 0.25]) == (0.0, 0)  # Q = 0: the merge is rejected for certain
    assert D.numpy_split_merge_accept(1, -50.0, (0.0, 0), 1.0, 0.0, 2, 2, 0) == (-50.0, -np.inf, 0.0, False)


def test_a_zero_factor_kills_a_forced_pass():
    # dS_o = +800 at beta = 1: the weight of the other block is cut to exactly 0.0, and a member forced there has the factor 0.0
    home, f, dead = D.numpy_split_merge_step(800.0, True, True, 1.0, forced_home=False)
    assert (home, f, dead) == (False, 0.0, True)
    home, f, dead = D.numpy_split_merge_step(800.0, True, True, 1.0, forced_home=True)
    assert (home, f, dead) == (True, 1.0, False)
    assert D.numpy_split_merge_step(800.0, True, True, 1.0, u=0.999999) == (True, 1.0, False)  # (a free scan never goes there)


# ------------------------------------------------------------------------------------------------------- the acceptance
def test_both_acceptance_formulas_are_the_literal_ones():
    rng = np.random.default_rng(11)
    for _ in range(300):
        ka, kb, t = int(rng.integers(1, 6)), int(rng.integers(1, 6)), int(rng.integers(2))
        mdS, beta, u = float(rng.normal(0, 20)), float(rng.choice([1.0, 0.6])), float(rng.random())
        q = (float(rng.uniform(0.5, 1)), int(rng.integers(-60, 2)))
        K, lnQ = ka + kb, math.log(q[0]) + q[1] * math.log(2.0)
        # split: dS = -merge_dS(D'); ln A = -beta dS + ln K - ln N(shape after) - ln Q_fwd
        ka2, kb2 = ka + (1 - t), kb + t
        N2 = ka2 * (ka2 - 1) // 2 + kb2 * (kb2 - 1) // 2
        dS, lnA, A, acc = D.numpy_split_merge_accept(0, mdS, q, beta, u, ka, kb, t)
        want = -beta * (-mdS) + math.log(K) - math.log(N2) - lnQ
        assert dS == -mdS and abs(lnA - want) <= 1e-12 * max(1.0, abs(want)) and acc == (u < A)
        assert A == math.exp(lnA) or abs(A - math.exp(lnA)) <= 1e-12 * A
        # merge: dS = merge_dS(D); ln A = -beta dS + ln N(shape now) - ln(K - 1) + ln Q_rev
        N = ka * (ka - 1) // 2 + kb * (kb - 1) // 2
        if N == 0:
            continue
        dS, lnA, A, acc = D.numpy_split_merge_accept(1, mdS, q, beta, u, ka, kb, t)
        want = -beta * mdS + math.log(N) - math.log(K - 1) + lnQ
        assert dS == mdS and abs(lnA - want) <= 1e-12 * max(1.0, abs(want)) and acc == (u < A)
    # a split and the merge that undoes it: the two A are reciprocal (same division, same Q, the shapes swapped)
    for ka, kb, t in ((2, 2, 0), (1, 3, 1), (1, 1, 0)):
        q, mdS = (0.7, -3), 4.25
        lnA_s = D.numpy_split_merge_accept(0, mdS, q, 0.6, 0.5, ka, kb, t)[1]
        lnA_m = D.numpy_split_merge_accept(1, mdS, q, 0.6, 0.5, ka + (1 - t), kb + t, t)[1]
        assert abs(lnA_s + lnA_m) <= 1e-13


def test_the_numbering_after_an_accepted_move():
    lab = np.array([0, 1, 1, 2, 0, 3, 4, 4, 3], dtype=np.int64)  # 3 + 2 blocks over 5 + 4 nodes
    out, ka, kb = D.numpy_split_merge_renumber(lab, 0, 0, 1, 3, 3, 2, away_nodes=[2])
    assert (ka, kb) == (4, 2) and out.tolist() == [0, 1, 3, 2, 0, 4, 5, 5, 4]  # away is label ka, type b one up
    out, ka, kb = D.numpy_split_merge_renumber(lab, 0, 1, 4, 5, 3, 2, away_nodes=[7])
    assert (ka, kb) == (3, 3) and out.tolist() == [0, 1, 1, 2, 0, 3, 4, 5, 3]  # away is label K
    out, ka, kb = D.numpy_split_merge_renumber(lab, 1, 0, 0, 1, 3, 2)
    assert (ka, kb) == (2, 2) and out.tolist() == [0, 0, 0, 1, 0, 2, 3, 3, 2]  # r keeps its label, everything above s one down
    out, ka, kb = D.numpy_split_merge_renumber(lab, 1, 1, 3, 4, 3, 2)
    assert (ka, kb) == (3, 1) and out.tolist() == [0, 1, 1, 2, 0, 3, 3, 3, 3]


# ------------------------------------------------------------------------------------- merge_dS against the oracle
def _graph(name):
    _, na, nb, ne, ka, kb, eps, hubs, iso = cases.CASE[name]
    return cases.random_graph(11, na, nb, ne, ka, kb, hubs, iso), na, nb, ka, kb, eps


def _oracle_S(graph, na, nb, ka, kb, eps, lab):
    o = O.OracleModel(graph[0], graph[1], na, nb, ka, kb, eps, lab.astype(np.uint32))
    o.init_bisbm()
    return o, o.entropy()


def _model_merge_dS(o, h, a, t, E, na, nb):
    """merge_dS of blocks h and a (global labels, type t) of the oracle's state through the host model"""
    ka, kb = o.ka, o.kb
    m, m_r, n_r, eta = o.m(), o.m_r(), o.n_r(), o.eta()
    oth = slice(0, ka) if t else slice(ka, ka + kb)
    T_div = _shape_term(E, na, nb, ka, kb)
    T_mer = _shape_term(E, na, nb, ka - (1 - t), kb - t)
    return D.numpy_split_merge_dS(m[h, oth], m[a, oth], eta[h], eta[a], m_r[h], m_r[a], n_r[h], n_r[a], T_mer, T_div, _lgamma, _log_q)


@pytest.mark.parametrize("name", ["tiny", "hubs_isolated"])
def test_merge_dS_with_the_shape_terms_is_the_oracles_change_of_description_length(name):
    """random divisions of both types: S at the shape after against S at the shape before, to 1e-9 |S| -- merges of a random
    pair of a random state, down to ONE block of a type, and the same numbers read as splits (a split's dS is -merge_dS(D'))"""
    graph, na, nb, ka0, kb0, eps = _graph(name)
    rng = np.random.default_rng(3)
    worst, down_to_one = 0.0, 0
    for trial in range(12):
        ka, kb = (ka0, kb0) if trial < 4 else ((2, kb0) if trial < 8 else (ka0, 2))
        lab = np.concatenate([rng.integers(0, ka, na), ka + rng.integers(0, kb, nb)])
        lab[:ka], lab[na:na + kb] = np.arange(ka), ka + np.arange(kb)  # (no block empty)
        o, S_div = _oracle_S(graph, na, nb, ka, kb, eps, lab)
        E = o.num_edges
        for t in (0, 1):
            k, lo = (kb, ka) if t else (ka, 0)
            if k < 2:
                continue
            r, s = sorted(rng.choice(k, 2, replace=False).tolist())
            got = _model_merge_dS(o, lo + r, lo + s, t, E, na, nb)
            assert got == _model_merge_dS(o, lo + s, lo + r, t, E, na, nb) or abs(got - _model_merge_dS(o, lo + s, lo + r, t, E, na, nb)) <= 1e-12 * abs(S_div)
            merged, ka2, kb2 = D.numpy_split_merge_renumber(lab, 1, t, lo + r, lo + s, ka, kb)
            _, S_mer = _oracle_S(graph, na, nb, ka2, kb2, eps, merged)
            err = abs((S_mer - S_div) - got) / abs(S_div)
            worst = max(worst, err)
            down_to_one += (ka2 if t == 0 else kb2) == 1
            assert err <= 1e-9, (name, trial, t, S_mer - S_div, got)
            # the split that undoes it: numbering of the split, the same unlabelled partition, the same S
            away = np.flatnonzero(lab == lo + s)
            back, ka3, kb3 = D.numpy_split_merge_renumber(merged, 0, t, lo + r, None, ka2, kb2, away_nodes=away)
            assert (ka3, kb3) == (ka, kb)
            _, S_back = _oracle_S(graph, na, nb, ka3, kb3, eps, back)
            assert abs(S_back - S_div) <= 1e-12 * abs(S_div)
    print("%s: merge_dS against the oracle: worst relative error %.3g; %d merge(s) down to one block of a type" % (name, worst, down_to_one))
    assert down_to_one >= 2


# --------------------------------------------------------------------------- exact detailed balance of the host model
DB_NA = DB_NB = 3
DB_EDGES = [(0, 3), (0, 4), (1, 3), (1, 4), (2, 5), (2, 5), (1, 5), (0, 3)]


def _canonical(lab):
    """relabel by first occurrence within each type: (labels tuple, ka, kb)"""
    lab, out, seen = list(lab), [], {}
    for x in lab[:DB_NA]:
        out.append(seen.setdefault(x, len(seen)))
    ka, seen = len(seen), {}
    for x in lab[DB_NA:]:
        out.append(seen.setdefault(x, ka + len(seen)))
    return tuple(out), ka, len(seen)


class _Enumerated:
    """the 25 partitions of the 3 + 3-node graph with the oracle's S, and the oracle's block state of any labelled state"""

    def __init__(self):
        a = np.array([e[0] for e in DB_EDGES], dtype=np.uint64)
        b = np.array([e[1] for e in DB_EDGES], dtype=np.uint64)
        self.graph = O.edge_to_csr(a, b, DB_NA + DB_NB)
        self.E = len(DB_EDGES)
        self.cache = {}
        parts = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (0, 1, 2)]
        self.states = []
        for pa in parts:
            for pb in parts:
                ka = max(pa) + 1
                self.states.append(_canonical(list(pa) + [ka + x for x in pb])[0])
        assert len(set(self.states)) == 25

    def oracle(self, lab):
        """(oracle model, S) of a labelled state without an empty block"""
        key = tuple(lab)
        if key not in self.cache:
            ka = len(set(lab[:DB_NA]))
            kb = len(set(lab[DB_NA:]))
            assert sorted(set(lab)) == list(range(ka + kb))
            self.cache[key] = _oracle_S(self.graph, DB_NA, DB_NB, ka, kb, 1.0, np.array(lab))
        return self.cache[key]

    def S(self, lab):
        return self.oracle(_canonical(list(lab))[0])[1]


def _scan_tree(en, lab, members, home, away, beta, forced=None):
    """Every outcome of one restricted scan over members 1 .. M - 1 from the labelled state `lab` (home and away both occupied):
    [(probability of the branch, product of the factors, labels at the end)].  forced: the labels the members are sent to --
    one branch, probability 1, with the product Q (0.0 when the pass dies)."""
    out = [(1.0, 1.0, list(lab))]
    for i in range(1, len(members)):
        v = members[i]
        nxt = []
        for p, q, cur in out:
            if q == 0.0:
                nxt.append((p, q, cur))
                continue
            c = cur[v]
            o = away if c == home else home
            free = sum(1 for x in cur if x == c) > 1
            dS_o = None
            if free:
                moved = list(cur)
                moved[v] = o
                dS_o = en.S(moved) - en.S(cur)
            if forced is not None:
                to_home, f, dead = D.numpy_split_merge_step(dS_o, c == home, free, beta, forced_home=forced[v] == home)
                end = list(cur)
                end[v] = home if to_home else away
                nxt.append((p, 0.0 if dead else q * f, end))
                continue
            if not free:
                nxt.append((p, q, cur))
                continue
            for u, to in ((0.0, True), (1.0 - 2.0 ** -53, False)):  # the two ends of u: home, away
                to_home, f, dead = D.numpy_split_merge_step(dS_o, c == home, True, beta, u=u)
                if to_home != to or f == 0.0:
                    continue  # (a branch of probability 0)
                end = list(cur)
                end[v] = home if to_home else away
                nxt.append((p * f, q * f, end))
        out = nxt
    return out


def _transition_matrix(en, beta, k_min=(1, 1), k_max=(3, 3)):
    """the exact kernel of one move with scans = 0: every kind, block or pair, launch-bit pattern and branch of the one scan"""
    index = {s: i for i, s in enumerate(en.states)}
    T = np.zeros((25, 25))
    for x in en.states:
        ix = index[x]
        o, _ = en.oracle(x)
        ka, kb = o.ka, o.kb
        K, N = ka + kb, D.numpy_split_merge_pairs(ka, kb)
        stay = 0.0
        # ---- splits: probability 1/2 * 1/K each
        for b in range(K):
            kind, t, r, s_new, refused = D.numpy_split_merge_choice(0, _word_for(b, K), ka, kb, k_min, k_max, size_of=lambda g: x.count(g))
            assert (kind, r) == (0, b)
            if refused:
                stay += 0.5 / K
                continue
            members = [v for v in range(len(x)) if x[v] == b]
            M = len(members)
            # the spare block: label s_new in the numbering of the split; type-b labels move up for a type-a split
            base = [l + 1 if (t == 0 and l >= ka) else l for l in x]
            for bits in itertools.product((0, 1), repeat=M - 1):
                p_L = 0.5 ** (M - 1)
                away = D.numpy_split_merge_launch([0] + list(bits))
                L = list(base)
                for i, v in enumerate(members):
                    if away[i]:
                        L[v] = s_new
                for p_branch, Q, end in _scan_tree(en, L, members, b, s_new, beta):
                    y = _canonical(end)[0]
                    oy, _ = en.oracle(tuple(end))
                    mdS = _model_merge_dS(oy, b, s_new, t, en.E, DB_NA, DB_NB)
                    _, lnA, A, _ = D.numpy_split_merge_accept(0, mdS, math.frexp(Q), beta, 0.0, ka, kb, t)
                    a = min(1.0, A)
                    T[ix, index[y]] += 0.5 / K * p_L * p_branch * a
                    stay += 0.5 / K * p_L * p_branch * (1.0 - a)
        # ---- merges: probability 1/2 * 1/N each
        if N == 0:
            stay += 0.5
        for i in range(N):
            kind, t, r, s, refused = D.numpy_split_merge_choice(1, _word_for(i, N), ka, kb, k_min, k_max)
            if refused:
                stay += 0.5 / N
                continue
            members = [v for v in range(len(x)) if x[v] in (r, s)]
            M = len(members)
            home, away_mask = D.numpy_split_merge_roles([x[v] for v in members])
            away_l = s if home == r else r
            mdS = _model_merge_dS(o, home, away_l, t, en.E, DB_NA, DB_NB)
            y = _canonical(D.numpy_split_merge_renumber(x, 1, t, r, s, ka, kb)[0].tolist())[0]
            for bits in itertools.product((0, 1), repeat=M - 1):
                p_L = 0.5 ** (M - 1)
                away = D.numpy_split_merge_launch([0] + list(bits))
                L = list(x)
                for j, v in enumerate(members):
                    L[v] = away_l if away[j] else home
                (_, Q, end), = _scan_tree(en, L, members, home, away_l, beta, forced=list(x))
                assert Q == 0.0 or end == list(x)
                _, lnA, A, _ = D.numpy_split_merge_accept(1, mdS, math.frexp(Q) if Q else (0.0, 0), beta, 0.0, ka, kb, t)
                a = min(1.0, A)
                T[ix, index[y]] += 0.5 / N * p_L * a
                stay += 0.5 / N * p_L * (1.0 - a)
        T[ix, ix] += stay
    return T


@pytest.fixture(scope="module")
def enumerated():
    return _Enumerated()


@pytest.mark.parametrize("beta", [1.0, 0.6])
def test_the_host_model_is_in_exact_detailed_balance_over_all_25_partitions(enumerated, beta):
    """3 + 3 nodes, shapes up to 3 + 3, scans = 0: every random choice of a move enumerated gives the exact kernel T; with pi =
    exp(-beta S) from the oracle, pi(x) T(x, y) = pi(y) T(y, x) to 1e-12 relative for all x != y"""
    en = enumerated
    T = _transition_matrix(en, beta)
    assert np.abs(T.sum(axis=1) - 1.0).max() <= 1e-12
    S = np.array([en.oracle(s)[1] for s in en.states])
    pi = np.exp(-beta * (S - S.min()))
    flow = pi[:, None] * T
    pairs = worst = 0
    for i in range(25):
        for j in range(i + 1, 25):
            if flow[i, j] == 0.0 and flow[j, i] == 0.0:
                continue
            pairs += 1
            rel = abs(flow[i, j] - flow[j, i]) / max(flow[i, j], flow[j, i])
            worst = max(worst, rel)
            assert rel <= 1e-12, (en.states[i], en.states[j], flow[i, j], flow[j, i])
    shapes = {(len(set(s[:3])), len(set(s[3:]))) for s in en.states}
    print("beta = %g: %d connected pairs of 25 states over %d shapes, worst relative imbalance %.3g" % (beta, pairs, len(shapes), worst))
    assert len(shapes) == 9 and pairs >= 24  # (25 states in one connected component have at least 24 links)
    # ... and the chain is irreducible: some power of T is positive everywhere
    P = np.linalg.matrix_power(T, 12)
    assert (P > 0).all()
    # a target without the shape terms is NOT in balance with this kernel (the test can fail)
    E, na, nb = en.E, DB_NA, DB_NB
    S_wrong = np.array([en.oracle(s)[1] - _shape_term(E, na, nb, len(set(s[:3])), len(set(s[3:]))) for s in en.states])
    flow_w = np.exp(-beta * (S_wrong - S_wrong.min()))[:, None] * T
    assert max(abs(flow_w[i, j] - flow_w[j, i]) / max(flow_w[i, j], flow_w[j, i]) for i in range(25) for j in range(25) if i != j and flow_w[i, j] > 0) > 1e-3


# ------------------------------------------------------------------------------------------------------------ the binding
def test_the_calls_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "bisbm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+bisbm_split_merge_run\s*\(\s*bisbm_handle\s+h\s*,\s*uint64_t\s+moves\s*,\s*uint32_t\s+scans\s*,\s*double\s+beta\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*k_min\s*,\s*const\s+uint32_t\s*\*\s*k_max\s*,\s*uint64_t\s*\*\s*accepted_out", code)
    assert re.search(r"\bint\s+bisbm_split_merge_get_last\s*\(\s*bisbm_handle\s+h\s*,\s*bisbm_split_merge_record\s*\*\s*out", code)
    assert re.search(r"\bint\s+bisbm_split_merge_get_total\s*\(\s*bisbm_handle\s+h\s*,\s*uint64_t\s*\*\s*out", code)
    assert re.search(r"#define\s+BISBM_ABI_VERSION\s+3\b", code)  # (additions only)
    assert "Split and merge moves" in text
    assert B.ABI["bisbm_split_merge_run"][1][1:4] == [C.c_uint64, C.c_uint32, C.c_double]
    if not os.path.exists(B.LIB_PATH):
        B.build()
    raw = C.CDLL(B.LIB_PATH)
    for fn in ("bisbm_split_merge_run", "bisbm_split_merge_get_last", "bisbm_split_merge_get_total", "bisbm_split_merge_shape_term"):
        assert hasattr(raw, fn), fn
    unit = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "csrc", "bisbm_split_merge.hip")).read()
    assert B.PHILOX_PURPOSE_SPLIT_MERGE == 11 and re.search(r"PHX_SPLIT_MERGE\s*=\s*11\b", unit)
    for name in ("SPLIT", "MERGE", "EVALUATED", "SINGLETON", "AT_K_MAX", "AT_K_MIN", "NO_PAIR"):
        assert int(re.search(r"#define\s+BISBM_SM_%s\s+(\d+)u" % name, code).group(1)) == getattr(B, "SM_" + name)
    # the record as Python reads it is the header's struct, field for field
    body = re.search(r"typedef struct bisbm_split_merge_record \{(.*?)\}", code, flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().split(" ", 1)[-1]) if decl.strip()]
    assert names == [f[0] for f in B.SplitMergeRecord._fields_], names
    assert C.sizeof(B.SplitMergeRecord) == 88
    for method in ("split_merge", "split_merge_last", "split_merge_total"):
        assert callable(getattr(B.BlockModel, method))
    for fn in ("numpy_split_merge_choice", "numpy_split_merge_launch", "numpy_split_merge_step", "numpy_split_merge_dS", "numpy_split_merge_accept",
               "numpy_split_merge_renumber", "numpy_split_merge_roles"):
        assert getattr(B, fn) is getattr(D, fn)
    hpp = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "host", "bisbm.hpp")).read()
    assert "bisbm_split_merge_run" in hpp and "bisbm_split_merge_get_last" in hpp and "bisbm_split_merge_get_total" in hpp
    assert "bisbm_split_merge.hip" in open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "build.py")).read()


def test_a_null_handle_is_an_invalid_argument():
    L = B.lib()
    assert L.bisbm_split_merge_run(None, 1, 3, 1.0, None, None, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_split_merge_get_last(None, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_split_merge_get_total(None, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_split_merge_shape_term(None, 1, 1, None) == B.BISBM_ERR_INVALID_ARG


def test_without_a_device_there_is_no_handle_to_split():
    """the new calls need a handle, and without a HIP device there is none: create fails loudly, as for every other call"""
    import torch
    if torch.cuda.is_available():
        return  # (tests/test_gpu_split_merge.py runs the calls)
    rowptr = np.array([0, 1, 2], dtype=np.uint64)
    col = np.array([1, 0], dtype=np.uint32)
    with pytest.raises(B.BisbmError) as e:
        B.BlockModel([0, 1], [0, 1], 2, 1, 1, 1.0, (rowptr, col)).split_merge(1)
    assert e.value.code == B.BISBM_ERR_NO_DEVICE


class _NoSweeps:
    """a model that must not be asked to run anything"""
    n, shard = 10, None

    def __getattr__(self, name):
        raise AssertionError("the model was touched: " + name)


def test_marginalize_refuses_what_needs_one_block_numbering_before_anything_runs():
    for kw in ({"align": True}, {"blocks": True, "align": True}, {"tempering": [1.0, 2.0]}, {"reshuffles": 2}, {"return_counts": True},
               {"clamp": [0]}, {"trace": 4}, {"recommend": ([0], 3)}):
        with pytest.raises(ValueError, match="split_merges"):
            B.marginalize(_NoSweeps(), 1, 1, 1, split_merges=2, **kw)
    with pytest.raises(ValueError, match="negative"):
        B.marginalize(_NoSweeps(), 1, 1, 1, split_merges=-1)
    with pytest.raises(ValueError, match="negative"):
        B.marginalize(_NoSweeps(), 1, 1, 1, split_merges=1, split_merge_scans=-1)


CLI = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
EL = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
BASE = ["-e", EL, "-y", "500", "500", "-z", "3", "3", "-n", "167", "167", "166", "167", "167", "166"]
SM = ["--marginalize", "--split_merge", "2", "--shape_counts", "shapes.txt", "--rng", "philox"]
CLI_REFUSALS = [
    (["--split_merge", "2", "--shape_counts", "x", "--rng", "philox"], "--split_merge", "--marginalize"),
    (["--marginalize", "--split_merge", "2", "--rng", "philox"], "--split_merge", "--shape_counts"),
    (["--marginalize", "--split_merge_scans", "2", "--rng", "philox"], "--split_merge_scans", "--split_merge"),
    (["--marginalize", "--k_min", "1", "1", "--rng", "philox"], "--k_min", "--split_merge"),
    (["--marginalize", "--k_max", "4", "4", "--rng", "philox"], "--k_max", "--split_merge"),
    (["--marginalize", "--shape_counts", "x", "--rng", "philox"], "--shape_counts", "--split_merge"),
    (SM + ["--tempering", "1", "2", "--chains", "2"], "--split_merge", "--tempering"),
    (SM + ["--align"], "--split_merge", "--align"),
    (SM + ["--reshuffle", "2"], "--split_merge", "--reshuffle"),
    (["--marginalize", "--split_merge", "2", "--shape_counts", "x", "--rng", "mt19937-compat"], "--split_merge", "Philox"),
    (["--marginalize", "--split_merge", "0", "--shape_counts", "x", "--rng", "philox"], "Invalid --split_merge", ">= 1"),
    (["--marginalize", "--split_merge", "some", "--shape_counts", "x", "--rng", "philox"], "Invalid --split_merge", ">= 1"),
    (SM + ["--split_merge_scans", "-1"], "Invalid --split_merge_scans", ">= 0"),
    (SM + ["--k_min", "0", "1"], "Invalid --k_min", ">= 1"),
    (SM + ["--k_min", "2"], "Invalid --k_min", "Two integers"),
    (SM + ["--k_min", "3", "1", "--k_max", "2", "5"], "Invalid --k_max", "--k_min"),
    (SM + ["--k_max", "200", "100"], "Invalid --k_max", "254"),
]


@pytest.mark.parametrize("extra,flag,word", CLI_REFUSALS, ids=[" ".join(c[0]) for c in CLI_REFUSALS])
def test_the_command_line_refuses_before_anything_runs(extra, flag, word):
    if not os.path.exists(CLI):
        B.build()
    r = subprocess.run([CLI] + BASE + extra, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stdout == "", (r.returncode, r.stdout, r.stderr)
    assert flag in r.stderr and word in r.stderr, r.stderr
    assert not os.path.exists("shapes.txt")


def test_help_lists_the_flags():
    if not os.path.exists(CLI):
        B.build()
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=120)
    for flag in ("--split_merge M", "--split_merge_scans", "--k_min A B", "--k_max A B", "--shape_counts OUT"):
        assert flag in r.stdout + r.stderr, flag
