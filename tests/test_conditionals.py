"""CPU checks of the node conditionals (include/bisbm.h, "Node conditionals"): the numpy model of steps 3 and 4 against a literal
double loop on bit patterns, the definition tied to the description length on the oracle (dS of a move = the change of
entropy(), and the softmax of the dS rows = the exact conditional of the enumerable graph's stationary distribution), and the
drop-in boundary (header, ctypes table, BlockModel)."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import cases
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed

TOL_DS_REL_S = 1e-9  # tests/test_cross_mode.py: |dS - (S1 - S0)| <= 1e-9 |S|
CALLS = ["bisbm_conditionals_set", "bisbm_conditionals_set_reference", "bisbm_conditionals_accumulate", "bisbm_conditionals_reset",
         "bisbm_conditionals_get_stats", "bisbm_conditionals_get_marginals", "bisbm_conditionals_get_last"]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _literal(dS, r, free, beta):
    """steps 3 and 4 of the header, one scalar operation after the other"""
    K = len(dS)
    if not free:
        P = [1.0 if s == r else 0.0 for s in range(K)]
        margin = None
    else:
        mn = dS[0]
        for x in dS[1:]:
            mn = x if x < mn else mn
        w = []
        for s in range(K):
            x = beta * (dS[s] - mn)
            w.append(0.0 if x > 700.0 else float(np.exp(-x)))
        Z = w[0]
        for y in w[1:]:
            Z = Z + y
        P = [y / Z for y in w]
        margin = min(dS[s] for s in range(K) if s != r)
    acc = 0.0
    for y in P:
        if y != 0.0:
            acc = acc + y * float(np.log(y))
    return P, P[r], 0.0 - acc, margin


ROWS = [
    # name, dS row, r, free, beta
    ("plain", [0.0, 1.5, -0.25, 3.0, 7.75], 0, True, 1.0),
    ("beta", [2.0, 0.0, -1.0, 0.5], 1, True, 0.37),
    ("beyond_700", [0.0, 800.0, 700.0, 700.0000001, -3.0, 1e6], 0, True, 1.0),  # x_s > 700 -> exactly 0.0; 703 > 700 too
    ("beyond_700_beta", [0.0, 350.1, 349.9], 0, True, 2.0),
    ("not_free", [0.0, -5.0, 2.0], 0, False, 1.0),       # a node alone in its block: the point mass, whatever dS says
    ("k_own_1", [0.0], 0, False, 1.0),
    ("ties_in_min", [0.0, -2.0, -2.0, 1.0, -2.0], 0, True, 1.0),
    ("tie_with_r", [0.0, 0.0, 0.0], 1, True, 3.0),
    ("r_last", [4.0, 0.125, 0.0], 2, True, 1.0),
]


@pytest.mark.parametrize("name,dS,r,free,beta", ROWS, ids=[c[0] for c in ROWS])
def test_numpy_model_is_the_literal_loop(name, dS, r, free, beta):
    P, stay, ent, margin = D.numpy_conditional_row(np.array(dS), r, free, beta)
    Pl, stay_l, ent_l, margin_l = _literal(dS, r, free, beta)
    assert (_bits(P) == _bits(Pl)).all()
    assert _bits([stay])[0] == _bits([stay_l])[0] and _bits([ent])[0] == _bits([ent_l])[0]
    assert margin == margin_l if free else margin is None
    assert abs(sum(Pl) - 1.0) <= (len(dS) + 4) * 2.0 ** -52
    assert ent >= 0.0
    if name.startswith("beyond_700"):
        assert (np.array(P)[1:4 if name == "beyond_700" else 2] == 0.0).all()
    if not free:
        assert P[r] == 1.0 and sum(P) == 1.0 and ent == 0.0 and not math.copysign(1.0, ent) < 0


def _oracle_rows(rowptr, col, na, nb, ka, kb, eps, labels):
    """dS rows from transition_ratio in Philox mode, and the worst |dS - (S(moved) - S)| over every node and target"""
    o = O.OracleModel(rowptr, col, na, nb, ka, kb, eps, labels)
    o.seed_philox(99, 0)
    o.init_bisbm()
    o2 = O.OracleModel(rowptr, col, na, nb, ka, kb, eps, labels)
    o2.init_bisbm()
    S0 = o.entropy()
    n_r = o.n_r()
    rows, worst = [], 0.0
    for v in range(na + nb):
        lo, hi = (0, ka) if v < na else (ka, ka + kb)
        row = np.zeros(hi - lo)
        for s in range(lo, hi):
            row[s - lo] = o.transition_ratio(v, s)[0]
            if s == labels[v]:
                assert row[s - lo] == 0.0
                continue
            moved = labels.copy()
            moved[v] = s
            o2.set_memberships(moved)
            o2.init_bisbm()
            worst = max(worst, abs(row[s - lo] - (o2.entropy() - S0)))
        rows.append(row)
    return rows, worst, abs(S0), n_r


def test_dS_is_the_change_of_the_description_length_hubs_isolated(record_property):
    _, na, nb, ne, ka, kb, eps, hubs, iso = cases.CASE["hubs_isolated"]
    rowptr, col = cases.random_graph(11, na, nb, ne, ka, kb, hubs, iso)
    o = O.OracleModel(rowptr, col, na, nb, ka, kb, eps, O.contiguous_labels(na, nb, ka, kb))
    o.seed_philox(5, 0)
    o.shuffle_bisbm()
    o.anneal("constant", [1.0], 2 * (na + nb), 1 << 60)
    _, worst, S, _ = _oracle_rows(rowptr, col, na, nb, ka, kb, eps, o.memberships().astype(np.uint32))
    record_property("worst_abs", worst)
    record_property("S", S)
    assert worst <= TOL_DS_REL_S * S


def test_softmax_of_the_rows_is_the_exact_conditional_on_the_enumerable_graph(record_property):
    """P(b_v = s | rest) of the stationary distribution exp(-S) over the states without an empty block, against the softmax of the
    oracle's dS rows.  A dS within e = 1e-9 |S| of the true difference moves exp(-dS) by e relative and Z by at most e relative:
    |P - P_exact| <= 2 e P (+ rounding, far below)."""
    rowptr, col = cases.enumerable_graph()
    na = nb = cases.ENUM_NA
    states, prob, _ = cases.enumerable_states()
    index = {int(c): i for i, c in enumerate(states)}
    rng = np.random.default_rng(3)
    worst_dS = worst_P = 0.0
    for pick in rng.choice(len(states), 40, replace=False):
        code = int(states[pick])
        bits = [(code >> i) & 1 for i in range(na + nb)]
        labels = np.array(bits[:na] + [2 + b for b in bits[na:]], dtype=np.uint32)
        rows, worst, S, n_r = _oracle_rows(rowptr, col, na, nb, 2, 2, cases.ENUM_EPS, labels)
        worst_dS = max(worst_dS, worst / S)
        assert worst <= TOL_DS_REL_S * S
        for v in range(na + nb):
            r = int(labels[v]) - (0 if v < na else 2)
            free = n_r[labels[v]] > 1
            P, stay, ent, margin = D.numpy_conditional_row(rows[v], r, free, 1.0)
            other = code ^ (1 << v)
            if free:
                assert other in index
                p_here, p_there = prob[pick], prob[index[other]]
                exact = np.zeros(2)
                exact[r], exact[1 - r] = p_here / (p_here + p_there), p_there / (p_here + p_there)
                assert margin == rows[v][1 - r]
            else:
                assert other not in index  # (the other state has an empty block)
                exact = np.zeros(2)
                exact[r] = 1.0
                assert margin is None
            err = np.abs(P - exact)
            assert (err <= 2 * TOL_DS_REL_S * S * exact + 1e-15).all(), (code, v, P, exact)
            worst_P = max(worst_P, float(err.max()))
            assert stay == P[r]
    record_property("worst_dS_rel_S", worst_dS)
    record_property("worst_P_abs", worst_P)


def test_the_calls_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "bisbm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bisbm_conditionals_[a-z_]+)\s*\(", code))
    assert declared == set(CALLS)
    assert re.search(r"#define\s+BISBM_COND_KEEP_LAST\s+1u", code) and B.COND_KEEP_LAST == 1
    assert "node conditionals (bisbm_conditionals_*)" in re.sub(r"\s*\n \*\s*", " ", text)
    assert re.search(r"#define\s+BISBM_ABI_VERSION\s+3\b", code)
    if not os.path.exists(B.LIB_PATH):
        B.build()
    raw = C.CDLL(B.LIB_PATH)
    for name in CALLS:
        assert hasattr(raw, name), "libbisbm_hip.so does not export %s" % name
        assert name in B.ABI
    for method in ("conditionals_set", "conditionals_set_reference", "conditionals_accumulate", "conditionals_reset", "conditionals_stats",
                   "conditionals_marginals", "conditionals_last"):
        assert callable(getattr(B.BlockModel, method))
    assert B.numpy_conditional_row is D.numpy_conditional_row
    mirror = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "host", "bisbm.hpp")).read()
    for name in CALLS:
        assert name in mirror, "host/bisbm.hpp does not wrap %s" % name
