"""Held conditionals and the least-settled ranking on the device (include/bisbm.h, "Held conditionals", "Least settled").  The held
rows of every (chain, node) against numpy_held_conditional_row fed the PLAIN rows of the same state and the device's exp, bit
for bit; heat-bath and greedy sweeps replayed from the held rows alone; the switch; the plain calls untouched by holds; soft
marginals, replica exchange and device entries fed held rows; bisbm_least_settled_topk against a lexsort of the stats; and the
plumbing: marginalize, the command line, the example.

Graphs: `tiny`, `hubs_isolated` and cases.random_graph at 300 + 200 nodes (300 + 260 for 1 + 255 blocks: 255 blocks need 255
nodes).  Three chains from first chain id 5, every node a query, last rows kept."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_align import overlap_tables
from test_gpu_constraints import _one_start, _state
from test_gpu_fields import _visit
from test_tempering import philox, u53

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu

SEED = 21
FIRST_ID = 5
CHAINS = 3
INF = float("inf")
ALL = ("clamp", "table", "field")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


_GRAPHS = {}


def _graph(key):
    """key: a name of cases.CASE, or (ka, kb) for a graph of 300 + 200 nodes"""
    if key not in _GRAPHS:
        if isinstance(key, str):
            _, na, nb, ne, ka, kb, eps, hubs, iso = cases.CASE[key]
            _GRAPHS[key] = (cases.random_graph(11, na, nb, ne, ka, kb, hubs, iso), na, nb, ka, kb, eps)
        else:
            ka, kb = key
            na, nb = 300, 260 if kb > 200 else 200
            _GRAPHS[key] = (cases.random_graph(11, na, nb, 3000, 5, 7), na, nb, ka, kb, 1.0)
    return _GRAPHS[key]


def _model(key, chains=CHAINS, labels=None, **kw):
    (rowptr, col), na, nb, ka, kb, eps = _graph(key)
    lab = O.contiguous_labels(na, nb, ka, kb) if labels is None else labels
    kw.setdefault("first_chain_id", FIRST_ID)
    return B.BlockModel(lab, syn.types_vector(na, nb), ka + kb, ka, kb, eps, (rowptr, col), n_chains=chains, seed=SEED, **kw)


def _own(v, na, ka, kb):
    return (ka, 0) if v < na else (kb, ka)  # K_own, first label of the type


def _make_holds(key, lab, which, seed):
    """mask: a random 30 % of the nodes.  table (256 classes): class 0 allows everything, class 1 one block per type (its members
    sit there), class 255 and the others random half-lists, every node's own block added to its class.  field (256 classes):
    N(0, 3^2) nats, class 255 included.  Holds not in `which` are None."""
    (_, _), na, nb, ka, kb, _ = _graph(key)
    n, K = na + nb, ka + kb
    rng = np.random.default_rng(seed)
    mask = table = field = None
    if "clamp" in which:
        mask = rng.random(n) < 0.3
    if "table" in which:
        allowed = rng.random((256, K)) < 0.5
        allowed[0] = True
        allowed[1] = False
        allowed[1, [int(lab[0]), int(lab[na])]] = True
        cls = rng.choice([0, 255] + list(range(2, 255)), size=n, p=[0.2, 0.2] + [0.6 / 253] * 253)
        members = np.flatnonzero((lab == lab[0]) | (lab == lab[na]))
        cls[members[::2]] = 1
        allowed[cls, lab] = True
        table = (cls.astype(np.uint8), allowed)
    if "field" in which:
        field = (rng.integers(0, 256, n).astype(np.uint8), rng.normal(scale=3.0, size=(256, K)))
        field[0][::7] = 255
    return mask, table, field


def _set_holds(m, holds):
    mask, table, field = holds
    if table is not None:
        m.constrain(*table)
    if mask is not None and mask.any():
        m.clamp(mask)
    if field is not None:
        m.set_fields(*field)


def _sync(p, m, chains):
    """the handle `p` (no holds) takes the labels of the chains of `m`"""
    for i, c in enumerate(chains):
        p.set_memberships(m.get_memberships(c), chain=i)
    p.init_bisbm()


def _model_rows(key, labs, n_r, plain, holds, beta, exp_dev, log_dev, nodes=None):
    """{(chain index, query index): (dE, P, stay, entropy, margin)} of numpy_held_conditional_row from the plain rows
    plain[i][0][chain], with the device's exp and log taken in one call each: a first pass records the arguments of exp, a second
    is served its values and records those of log, a third is served both"""
    (_, _), na, nb, ka, kb, _ = _graph(key)
    mask, table, field = holds
    nodes = range(na + nb) if nodes is None else nodes

    def run(exp, log):
        out = {}
        for c in range(len(labs)):
            for i, v in enumerate(nodes):
                v = int(v)
                k_own, lo = _own(v, na, ka, kb)
                r = int(labs[c][v]) - lo
                free = k_own > 1 and int(n_r[c][lo + r]) > 1
                out[c, i] = D.numpy_held_conditional_row(
                    plain[i][0][c][:k_own], r, free, beta, clamped=bool(mask is not None and mask[v]),
                    allowed_own=None if table is None else table[1][table[0][v], lo:lo + k_own],
                    f_own=None if field is None else field[1][field[0][v], lo:lo + k_own], exp=exp, log=log)
        return out

    def recorder(fn):
        rec = []

        def record(x):
            rec.append(np.array(x, dtype=np.float64))
            return fn(x)
        return rec, record

    def server(dev, rec):
        flat, pos = (dev(np.concatenate(rec)) if rec else np.zeros(0)), [0]

        def served(x):
            y = flat[pos[0]:pos[0] + len(x)]
            pos[0] += len(x)
            return y
        return served
    exp_args, exp_rec = recorder(np.exp)
    run(exp_rec, np.log)
    log_args, log_rec = recorder(np.log)
    run(server(exp_dev, exp_args), log_rec)
    return run(server(exp_dev, exp_args), server(log_dev, log_args))


def _zero(Q):
    return {"stay": np.zeros(Q), "entropy": np.zeros(Q), "margin": np.zeros(Q), "free": np.zeros(Q, dtype=np.uint64)}


def _add(total, rows, chains, Q):
    """the host's chain-ordered adds of the model's terms"""
    for c in chains:
        for i in range(Q):
            _, _, stay, ent, margin = rows[c, i]
            total["stay"][i] = total["stay"][i] + stay
            total["entropy"][i] = total["entropy"][i] + ent
            if margin is not None:
                total["margin"][i] = total["margin"][i] + margin
                total["free"][i] += 1


def _check_stats(st, total, terms):
    assert st["terms"] == terms
    for key in ("stay", "entropy", "margin"):
        assert _same(st[key], total[key]), (key, int((_bits(st[key]) != _bits(total[key])).sum()), np.abs(st[key] - total[key]).max())
    assert (st["free"] == total["free"]).all()


def _held_pair(key, which, seed=1, beta=1.0, sweeps_before=1):
    """m: three chains under the holds `which` with the switch on; p: three chains without holds (the plain rows).  Every chain of m
    starts from chain 2's labels after a shuffle and three sweeps (one table then admits all of them), and `sweeps_before` held
    sweeps take the chains apart again."""
    m, p = _model(key), _model(key)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    lab = _one_start(m, CHAINS - 1)
    holds = _make_holds(key, lab, which, seed)
    _set_holds(m, holds)
    if sweeps_before:
        m.run_sweeps(sweeps_before)
    m.conditionals_set(None, beta, keep_last=True)
    m.conditionals_held(True)
    assert m.conditionals_is_held()
    p.conditionals_set(None, beta, keep_last=True)
    assert not p.conditionals_is_held()
    return m, p, holds


def _check_sample(key, m, p, holds, beta, total, seen, chains=None):
    """one sample of both handles at the state of m: the held rows of m against the model on the plain rows of p"""
    (_, _), na, nb, ka, kb, _ = _graph(key)
    n = na + nb
    chains = list(range(m.n_chains)) if chains is None else chains
    _sync(p, m, chains)
    p.conditionals_accumulate()
    m.conditionals_accumulate()
    labs = [m.get_memberships(c).astype(np.int64) for c in chains]
    n_r = [m.get_n_r(c) for c in chains]
    plain = [p.conditionals_last(i) for i in range(n)]
    held = [m.conditionals_last(i) for i in range(n)]
    rows = _model_rows(key, labs, n_r, plain, holds, beta, m.debug_exp, m.debug_log)
    mask, table, field = holds
    for j, c in enumerate(chains):
        for v in range(n):
            k_own, lo = _own(v, na, ka, kb)
            r = int(labs[j][v]) - lo
            dE, P, stay, ent, margin = rows[j, v]
            dE_dev, P_dev = held[v][0][c][:k_own], held[v][1][c][:k_own]
            want = plain[v][0][j][:k_own] if field is None else B.numpy_field_row(plain[v][0][j][:k_own], r, field[1][field[0][v], lo:lo + k_own])
            assert _same(dE_dev, want) and _same(dE_dev, dE), (c, v)
            assert _same(P_dev, P), (c, v, np.abs(P_dev - P).max())
            A = np.ones(k_own, dtype=bool) if table is None else table[1][table[0][v], lo:lo + k_own]
            assert (P_dev[~A] == 0.0).all()
            seen["open"] += margin is not None
            seen["clamped"] += bool(mask is not None and mask[v])
            seen["one_block"] += bool(A.sum() == 1 and k_own > 1)
            seen["barred_min"] += bool(margin is not None and (dE[~A] < dE[A].min()).any())
            seen["zero_weight_inside"] += bool(margin is not None and (P[A] == 0.0).any())
            seen["second_word"] += bool(margin is not None and lo + k_own > 32 and not A[max(32 - lo, 0):].all())
    _add(total, rows, range(len(chains)), n)
    return rows


def _new_seen():
    return {"open": 0, "clamped": 0, "one_block": 0, "barred_min": 0, "zero_weight_inside": 0, "second_word": 0}


# (6, 5): one wave; (64, 65): one type on each kernel width; (70, 3); (1, 255): a one-block type and the longest row of lanes;
# (31, 4), (32, 4), (33, 4): the type-b window of cn_bits ends in, at the end of and behind the first 32-bit word
SHAPES = [(6, 5), (64, 65), (70, 3), (1, 255), (31, 4), (32, 4), (33, 4)]
CASES = [(key, ALL) for key in ["tiny", "hubs_isolated"] + SHAPES] + [(key, (one,)) for key in [(6, 5), (64, 65)] for one in ALL]


@pytest.mark.parametrize("key,which", CASES, ids=["%s-%s" % (k if isinstance(k, str) else "%d+%d" % k, "+".join(w)) for k, w in CASES])
def test_held_rows_and_their_sums_are_the_numpy_model_bit_for_bit(key, which):
    beta = 1.0 if key != (6, 5) else 0.8
    m, p, holds = _held_pair(key, which, beta=beta)
    (_, _), na, nb, ka, kb, _ = _graph(key)
    n = na + nb
    total, seen = _zero(n), _new_seen()
    for sample in range(3):
        if sample:
            m.run_sweeps(1)
        _check_sample(key, m, p, holds, beta, total, seen)
    _check_stats(m.conditionals_stats(), total, 3 * CHAINS)
    print(key, which, seen)
    assert seen["open"] > 0
    if "clamp" in which:
        assert seen["clamped"] > 0
    if "table" in which:
        assert seen["one_block"] > 0
        if key != "tiny":  # (3 + 2 blocks: a list of two blocks seldom bars the cheaper one)
            assert seen["barred_min"] > 0
        if key in SHAPES and ka + kb > 32:
            assert seen["second_word"] > 0
    m.close()
    p.close()


def test_a_barred_minimum_and_weights_that_underflow_to_exact_zeros():
    """every open node's cheapest other block is struck from its list (its class: one per node), and a field row holds +800 and
    -800 nats: the minimum, the margin and the weights leave the barred block out, x > 700 gives exact zeros inside A_v"""
    key = (6, 5)
    (_, _), na, nb, ka, kb, _ = _graph(key)
    n, K = na + nb, ka + kb
    m, p = _model(key), _model(key)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    lab = _one_start(m, CHAINS - 1)
    p.conditionals_set(None, 1.0, keep_last=True)
    _sync(p, m, range(CHAINS))
    p.conditionals_accumulate()
    nodes = np.arange(0, n, 2)[:250]  # (at most 255 classes of their own beside class 0)
    allowed = np.ones((1 + len(nodes), K), dtype=bool)
    cls = np.zeros(n, dtype=np.uint8)
    struck = {}
    for j, v in enumerate(nodes):
        k_own, lo = _own(int(v), na, ka, kb)
        row = p.conditionals_last(int(v))[0][0][:k_own].copy()
        row[int(lab[v]) - lo] = INF
        s = int(np.argmin(row))
        cls[v] = 1 + j
        allowed[1 + j, lo + s] = False
        struck[int(v)] = s
    fcls = (np.arange(n) % 3).astype(np.uint8)
    field = np.zeros((3, K))
    field[1, [1, ka + 1]] = 800.0
    field[2, [2, ka + 2]] = -800.0
    holds = (None, (cls, allowed), (fcls, field))
    _set_holds(m, holds)
    m.conditionals_set(None, 1.0, keep_last=True)
    m.conditionals_held(True)
    total, seen = _zero(n), _new_seen()
    rows = _check_sample(key, m, p, holds, 1.0, total, seen)
    _check_stats(m.conditionals_stats(), total, CHAINS)
    assert seen["barred_min"] > 20 and seen["zero_weight_inside"] > 20, seen
    for v, s in struck.items():
        dE, P, stay, ent, margin = rows[0, v]
        if margin is not None:
            assert P[s] == 0.0 and np.isfinite(dE[s])
    m.close()
    p.close()


# ------------------------------------------------------------------------------------------------------- the heat-bath tie
@pytest.mark.parametrize("key,beta", [("tiny", 1.0), ("tiny", INF), ("hubs_isolated", 1.0), ("hubs_isolated", INF)])
def test_a_sweep_replayed_from_the_held_rows_alone(key, beta):
    """tests/test_gpu_fields.py::_heatbath_replay with all three holds on, but the helper's held P rows go straight into
    numpy_heatbath_choice: no restriction, no field add and no exponential on the host"""
    (rowptr, col), na, nb, ka, kb, eps = _graph(key)
    n, greedy = na + nb, beta == INF
    m = _model(key)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    c, gid, sweep0 = CHAINS - 1, FIRST_ID + CHAINS - 1, 3
    lab = _one_start(m, c)
    holds = _make_holds(key, lab, ALL, 2)
    mask, table, field = holds
    _set_holds(m, holds)
    helper = _model(key, 1, labels=lab.astype(np.uint32))
    helper.init_bisbm()
    _set_holds(helper, holds)
    helper.conditionals_set(None, 1.0, keep_last=True)
    helper.conditionals_held(True)

    def sync():
        helper.set_memberships(lab.astype(np.uint32))
        helper.init_bisbm()
        helper.conditionals_accumulate()
    sync()
    moved_gpu = m.polish(1)[0] if greedy else m.heatbath_sweeps(1, beta)
    moved, opened = 0, 0
    for pos, v in enumerate(_visit(gid, sweep0, na, nb)):
        k_own, lo = _own(v, na, ka, kb)
        r = int(lab[v]) - lo
        dE, P = (x[0][:k_own] for x in helper.conditionals_last(v))
        o = philox(SEED, gid, B.PHILOX_PURPOSE_HEATBATH, sweep0 * n + pos)
        if greedy:  # (the greedy choice reads dE, not P: whether the node is open and its A_v are the host's)
            A = table[1][table[0][v], lo:lo + k_own]
            is_open = k_own > 1 and int((lab == lab[v]).sum()) > 1 and not mask[v] and A.sum() > 1
            assert is_open or P[r] == 1.0
            s = D.numpy_heatbath_choice(dE, P, r, is_open, 0.0, True, allowed=A)
        else:
            s = D.numpy_heatbath_choice(dE, P, r, True, u53(o[0], o[1]), False)
        opened += P[r] != 1.0
        if s != r:
            assert not mask[v] and table[1][table[0][v], lo + s]
            lab[v] = lo + s
            moved += 1
            sync()
    assert moved > 0 and opened > 0
    assert (m.get_memberships(c) == lab).all(), np.flatnonzero(m.get_memberships(c) != lab)
    assert int(moved_gpu[c]) == moved
    for x, y in zip(_state(m, c)[1:], _state(helper, 0)[1:]):
        assert (x == y).all()
    m.close()
    helper.close()


# ------------------------------------------------------------------------------------------------------------- the switch
def _everything(m, n, ref):
    out = {"stats": m.conditionals_stats(), "last": [m.conditionals_last(i) for i in range(0, n, 7)]}
    if ref:
        out["prob"] = m.conditionals_marginals()
    return out


def _same_everything(a, b):
    ok = a["stats"]["terms"] == b["stats"]["terms"] and (a["stats"]["free"] == b["stats"]["free"]).all()
    ok = ok and all(_same(a["stats"][k], b["stats"][k]) for k in ("stay", "entropy", "margin"))
    ok = ok and all(_same(x[0], y[0]) and _same(x[1], y[1]) for x, y in zip(a["last"], b["last"]))
    if "prob" in a:
        ok = ok and a["prob"][1] == b["prob"][1] and _same(a["prob"][0], b["prob"][0])
    return ok


def test_the_switch():
    key = "hubs_isolated"
    (_, _), na, nb, ka, kb, _ = _graph(key)
    n = na + nb
    a, b = _model(key), _model(key)
    for m in (a, b):
        m.shuffle_bisbm()
        m.run_sweeps(3)
        m.conditionals_set(None, 1.3, keep_last=True)
        m.conditionals_set_reference(a.get_memberships(0))
    # on with nothing held is off, bit for bit, in every output
    b.conditionals_held(True)
    assert b.conditionals_is_held() and not a.conditionals_is_held()
    for m in (a, b):
        m.conditionals_accumulate()
    assert _same_everything(_everything(a, n, True), _everything(b, n, True))
    # a call that does not change the switch changes nothing
    b.conditionals_held(True)
    assert b.conditionals_stats()["terms"] == CHAINS
    # on, then holds set and cleared again, is the same
    lab = _one_start(b, 0)
    _one_start(a, 0)
    holds = _make_holds(key, lab, ALL, 3)
    _set_holds(b, holds)
    b.conditionals_accumulate()
    a.conditionals_accumulate()
    assert not _same(a.conditionals_stats()["entropy"], b.conditionals_stats()["entropy"])  # (held rows now)
    b.unclamp(), b.unconstrain(), b.clear_fields()
    for m in (a, b):
        m.conditionals_reset()
        m.conditionals_accumulate()
    assert _same_everything(_everything(a, n, True), _everything(b, n, True))
    # switching, in either direction, zeroes the sums and prob and forgets the last rows; queries, beta and the reference stay
    for on in (False, True):
        b.conditionals_held(on)
        assert b.conditionals_is_held() == on
        st = b.conditionals_stats()
        assert st["terms"] == 0 and not st["stay"].any() and not st["entropy"].any() and not st["margin"].any() and not st["free"].any()
        prob, terms = b.conditionals_marginals()
        assert terms == 0 and not prob.any()
        with pytest.raises(B.BisbmError) as e:
            b.conditionals_last(0)
        assert e.value.code == B.BISBM_ERR_STATE
        b.conditionals_accumulate()
        a.conditionals_reset()
        a.conditionals_accumulate()
        assert _same_everything(_everything(a, n, True), _everything(b, n, True))  # (beta 1.3 and the reference are still there)
    # conditionals_set turns it off
    b.conditionals_set(None, 1.0)
    assert not b.conditionals_is_held()
    a.close()
    b.close()


def test_with_the_switch_off_the_holds_move_nothing():
    """all three holds set and the switch off: rows, stats and soft marginals of a handle with the same labels and no holds"""
    key = (64, 65)
    (_, _), na, nb, ka, kb, _ = _graph(key)
    n = na + nb
    m, p = _model(key), _model(key)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    lab = _one_start(m, CHAINS - 1)
    _set_holds(m, _make_holds(key, lab, ALL, 4))
    m.run_sweeps(1)
    ref = m.get_memberships(1)
    for h in (m, p):
        h.conditionals_set(None, 1.0, keep_last=True)
        h.conditionals_set_reference(ref)
    for _ in range(2):
        m.run_sweeps(1)
        _sync(p, m, range(CHAINS))
        m.conditionals_accumulate()
        p.conditionals_accumulate()
    assert not m.conditionals_is_held()
    assert _same_everything(_everything(m, n, True), _everything(p, n, True))
    m.close()
    p.close()


# ------------------------------------------------------------------------------------ downstream: fed the held rows
def test_soft_marginals_from_held_rows_are_the_hosts_scatter():
    key = (6, 5)
    (_, _), na, nb, ka, kb, _ = _graph(key)
    n = na + nb
    m, p, holds = _held_pair(key, ALL, seed=5)
    ref = m.get_memberships(0)
    m.conditionals_set_reference(ref)
    prob = np.zeros((n, max(ka, kb)))
    for _ in range(2):
        m.run_sweeps(1)
        m.conditionals_accumulate()
        perms = []
        for c in range(CHAINS):
            ca, cb = overlap_tables(m.get_memberships(c), ref, na, ka, kb)
            perms.append((B.align_assignment(ca)[0].astype(np.int64), B.align_assignment(cb)[0].astype(np.int64)))
        for v in range(n):
            k_own, lo = _own(v, na, ka, kb)
            P = m.conditionals_last(v)[1]
            for c in range(CHAINS):
                perm = perms[c][1 if v >= na else 0]
                for s in range(k_own):
                    prob[v, perm[s]] = prob[v, perm[s]] + P[c, s]
    got, terms = m.conditionals_marginals()
    assert terms == 2 * CHAINS and _same(got, prob)
    mask, table, _ = holds
    clamped_everywhere = mask & (m.get_memberships(0) == ref) & (m.get_memberships(1) == ref) & (m.get_memberships(2) == ref)
    assert clamped_everywhere.any() and ((got[clamped_everywhere] == 0) | (got[clamped_everywhere] == terms)).all()  # point masses
    m.close()
    p.close()


def test_replica_exchange_counts_held_rows_on_rung_0_and_leaves_nan_rows_elsewhere():
    key, chains, ladder = "hubs_isolated", 6, [1.0, 1.5, 2.2]
    (_, _), na, nb, ka, kb, _ = _graph(key)
    n = na + nb
    m, p = _model(key, chains, first_chain_id=6), _model(key, 2)  # (ensembles are global ids [3 g, 3 g + 3))
    m.shuffle_bisbm()
    m.run_sweeps(3)
    lab = _one_start(m, 0)
    holds = _make_holds(key, lab, ALL, 6)
    _set_holds(m, holds)
    m.set_tempering(ladder)
    m.tempering_run(2, 1)
    m.conditionals_set(None, 1.0, keep_last=True)
    m.conditionals_held(True)
    p.conditionals_set(None, 1.0, keep_last=True)
    total, seen = _zero(n), _new_seen()
    for sample in range(1, 3):
        m.tempering_run(2, 1)
        cold = [int(c) for c in np.flatnonzero(m.tempering_state()[0] == 0)]
        assert len(cold) == 2
        _check_sample(key, m, p, holds, 1.0, total, seen, chains=cold)
        assert m.conditionals_stats()["terms"] == 2 * sample
        for v in range(0, n, 11):
            dE, P = m.conditionals_last(v)
            for c in range(chains):
                assert np.isnan(dE[c]).all() == np.isnan(P[c]).all() == (c not in cold)
    _check_stats(m.conditionals_stats(), total, 4)
    assert seen["open"] > 0 and seen["clamped"] > 0
    m.close()
    p.close()


def _run_both(key, which, seed, queries=None, samples=1, **kw):
    """a handle and one of three device entries of the same device, through the same calls"""
    one, many = _model(key), _model(key, devices=[0, 0, 0], **kw)
    holds = None
    for m in (one, many):
        m.shuffle_bisbm()
        m.run_sweeps(3)
        lab = _one_start(m, CHAINS - 1)
        holds = _make_holds(key, lab, which, seed)
        _set_holds(m, holds)
        m.conditionals_set(queries, 1.0, keep_last=True)
        m.conditionals_held(True)
        m.conditionals_set_reference(lab.astype(np.uint32))
        for _ in range(samples):
            m.run_sweeps(1)
            m.conditionals_accumulate()
    return one, many, holds


def test_three_device_entries_give_the_bits_of_one_handle():
    key = (6, 5)
    (_, _), na, nb, ka, kb, _ = _graph(key)
    n = na + nb
    one, many, _ = _run_both(key, ALL, 7)  # (one sample: an entry's own sum over samples is added as a whole when it is read)
    assert many.conditionals_is_held()
    for c in range(CHAINS):
        assert (one.get_memberships(c) == many.get_memberships(c)).all()
    for i in range(0, n, 5):
        a, b = one.conditionals_last(i), many.conditionals_last(i)
        assert _same(a[0], b[0]) and _same(a[1], b[1]), i
    # one chain per entry: the entries' sums added in device order are the one handle's chain-ordered sums
    a, b = one.conditionals_stats(), many.conditionals_stats()
    assert a["terms"] == b["terms"] == CHAINS and (a["free"] == b["free"]).all()
    assert all(_same(a[k], b[k]) for k in ("stay", "entropy", "margin"))
    pa, pb = one.conditionals_marginals(), many.conditionals_marginals()
    assert pa[1] == pb[1] == CHAINS and _same(pa[0], pb[0])
    many.run_sweeps(1)
    many.conditionals_accumulate()
    b = many.conditionals_stats()
    for by in ("entropy", "stay"):
        idx, nodes, val, terms = many.least_settled(40, by)
        want_idx, want_val = D.numpy_least_settled(b[by], 40, by)
        assert terms == 2 * CHAINS and (idx == want_idx).all() and _same(val, want_val) and (nodes == idx).all()
        assert _same(val, b[by][idx])
    many.conditionals_held(False)
    st = many.conditionals_stats()
    assert not many.conditionals_is_held() and st["terms"] == 0 and not st["stay"].any()
    one.close()
    many.close()


# ------------------------------------------------------------------------------------------------------------------ top-k
def _check_topk(m, nq, ks):
    st = m.conditionals_stats()
    q = m.conditional_queries.astype(np.int64)
    for by in ("entropy", "stay"):
        v = st[by]
        assert len(v) == nq
        for k in ks:
            idx, nodes, val, terms = m.least_settled(k, by)
            want_idx, want_val = D.numpy_least_settled(v, k, by)
            assert terms == st["terms"] and len(idx) == k
            assert (idx == want_idx).all(), (by, nq, k, np.flatnonzero(idx != want_idx)[:5])
            assert _same(val, want_val)
            some = idx != B.QUERY_NONE
            assert some.sum() == min(k, nq) and _same(val[some], v[idx[some]]) and (nodes[some] == q[idx[some]]).all() and (nodes[~some] == -1).all()
    return st


@pytest.mark.parametrize("nq", [1, 255, 256, 257, 1604])
def test_least_settled_is_the_lexsort_of_the_stats(nq):
    """queries that repeat (1604 over 500 nodes) and clamped nodes, all at entropy +0.0 and stay = terms, give the ties; k runs past
    the entries and past the non-zero entries"""
    key = "hubs_isolated"
    (_, _), na, nb, ka, kb, _ = _graph(key)
    n = na + nb
    m = _model(key)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    lab = _one_start(m, 0)
    holds = _make_holds(key, lab, ALL, 8)
    _set_holds(m, holds)
    q = ((np.arange(nq) * 7 + 3) % n).astype(np.uint32)
    m.conditionals_set(q, 1.0)
    m.conditionals_held(True)
    for _ in range(2):
        m.run_sweeps(1)
        m.conditionals_accumulate()
    st = _check_topk(m, nq, sorted({1, min(nq, 1024), 1024}))
    if nq >= 255:
        settled = (st["entropy"] == 0.0).sum()
        assert settled >= 0.3 * nq - 40 and (st["stay"] == st["terms"]).sum() >= settled > 0  # (the clamped ones among others)
    # plain rows are ranked alike
    m.conditionals_held(False)
    m.conditionals_accumulate()
    _check_topk(m, nq, [min(nq, 1024)])
    m.close()


def test_refusals():
    key = "tiny"
    (_, _), na, nb, ka, kb, _ = _graph(key)
    m = _model(key)
    m.shuffle_bisbm()
    L = B.lib()
    import ctypes as C

    def code(fn, *args):
        with pytest.raises(B.BisbmError) as e:
            fn(*args)
        assert str(e.value)
        return e.value.code
    # without queries
    assert code(m.conditionals_held, True) == B.BISBM_ERR_STATE
    assert code(m.conditionals_is_held) == B.BISBM_ERR_STATE
    assert code(m.least_settled, 3) == B.BISBM_ERR_STATE
    m.conditionals_set(None, 1.0)
    # before the first sample; k; by; NULL
    assert code(m.least_settled, 3) == B.BISBM_ERR_STATE
    m.conditionals_accumulate()
    assert code(m.least_settled, 0) == B.BISBM_ERR_INVALID_ARG
    assert code(m.least_settled, B.QUERY_MAX_K + 1) == B.BISBM_ERR_UNSUPPORTED
    assert len(m.least_settled(B.QUERY_MAX_K)[0]) == B.QUERY_MAX_K
    with pytest.raises(ValueError):
        m.least_settled(3, "margin")
    idx = np.zeros(3, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    assert L.bisbm_least_settled_topk(m._h, 2, 3, idx.ctypes.data_as(u32p), None, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_least_settled_topk(m._h, 1, 3, None, None, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_least_settled_topk(m._h, 1, 3, idx.ctypes.data_as(u32p), None, None) == B.BISBM_OK  # (values and terms may be NULL)
    assert L.bisbm_held_conditionals_get(m._h, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_held_conditionals_set(None, 1) == B.BISBM_ERR_INVALID_ARG and L.bisbm_least_settled_topk(None, 0, 1, None, None, None) == B.BISBM_ERR_INVALID_ARG
    # a reset forgets the samples again
    m.conditionals_reset()
    assert code(m.least_settled, 3) == B.BISBM_ERR_STATE
    m.close()
    # a compat handle has no conditionals, so it has no switch
    (rowptr, col), na, nb, ka, kb, eps = _graph(key)
    w = B.BlockModel(O.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, eps, (rowptr, col), rng="compat", seed=1, gen_seed=2)
    assert code(w.conditionals_held, True) == B.BISBM_ERR_STATE
    w.close()


# --------------------------------------------------------------------------------------------------------------- upwards
def test_marginalize_and_the_cli_reproduce_the_python_calls(tmp_path):
    rowptr, col, na, nb = O.load_graph("n_1000")
    n, chains, seed, beta, k = na + nb, 4, 5, 0.7, 12
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    planted = O.contiguous_labels(na, nb, 4, 6)
    clamped = np.arange(0, n, 3)
    q = np.concatenate([np.arange(0, n, 7), [0, 4, na + 1]]).astype(np.uint32)  # (a third of them clamped, node 0 twice)

    def model():
        m = B.BlockModel(planted, syn.types_vector(na, nb), 10, 4, 6, 1.0, (rowptr, col), n_chains=chains, seed=seed)
        m.init_bisbm()
        return m
    m = model()
    labels, _, st, ranked = B.marginalize(m, 3, 2, 2, clamp=clamped, conditionals=(q, beta), conditionals_held=True, least_settled=(k, "stay"))
    assert m.conditionals_is_held() and st["terms"] == 2 * chains
    m2 = model()
    m2.clamp(clamped)
    m2.run_sweeps(3)
    m2.marginals_reset()
    m2.conditionals_set(q, beta)
    m2.conditionals_held(True)
    for _ in range(2):
        m2.run_sweeps(2)
        m2.marginals_accumulate(None)
        m2.conditionals_accumulate()
    st2, ranked2 = m2.conditionals_stats(), m2.least_settled(k, "stay")
    assert all(_same(st[key], st2[key]) for key in ("stay", "entropy", "margin")) and (st["free"] == st2["free"]).all()
    assert (ranked[0] == ranked2[0]).all() and (ranked[1] == ranked2[1]).all() and _same(ranked[2], ranked2[2]) and ranked[3] == ranked2[3] == 2 * chains
    held = np.isin(q, clamped)
    assert (st["stay"][held] == st["terms"]).all() and (st["entropy"][held] == 0.0).all() and (st["free"][held] == 0).all()
    assert not np.isin(ranked[1], clamped).any()  # (a clamped query stays in every chain: the largest stay sum there is)
    m3 = model()
    out = B.marginalize_modes(m3, 1, 2, 1, threshold=0.5, clamp=clamped, conditionals=(q, beta), conditionals_held=True, least_settled=(k,))
    assert out["conditionals"]["terms"] > 0 and len(out["least_settled"][0]) == k
    assert _same(out["least_settled"][2], D.numpy_least_settled(out["conditionals"]["entropy"], k)[1])
    for h in (m, m2, m3):
        h.close()
    # the command line: the same run
    mb, cl, qin, qout, rout = (tmp_path / x for x in ("labels.txt", "clamp.txt", "nodes.txt", "out.txt", "ranked.txt"))
    mb.write_text("".join("%d\n" % x for x in planted))
    cl.write_text(" ".join(str(v) for v in clamped) + "\n")
    qin.write_text("".join("%d\n" % v for v in q))
    base = [cli, "-e", el, "-y", str(na), str(nb), "-z", "4", "6", "--membership_path", str(mb), "-d", str(seed), "--rng", "philox", "--chains",
            str(chains), "-b", str(3 * n), "-t", str(4 * n), "-f", str(2 * n), "--marginalize", "--clamp", str(cl), "--conditionals", str(qin),
            str(qout), "--conditionals_beta", str(beta), "--conditionals_held"]
    for by in ("stay", "entropy", None):
        r = subprocess.run(base + ["--least_settled", str(rout), str(k)] + ([by] if by else []), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert "held rows" in r.stderr and "least_settled: %d of %d" % (k, len(q)) in r.stderr
        lines = [line.split() for line in qout.read_text().splitlines()]
        assert len(lines) == len(q)
        got = np.array([[float(t) for t in tok[1:3]] for tok in lines])
        assert _same(got[:, 0], st["stay"] / st["terms"]) and _same(got[:, 1], st["entropy"] / st["terms"])
        by = by or "entropy"
        want_idx, want_val = D.numpy_least_settled(st[by], k, by)
        tok = [line.split() for line in rout.read_text().splitlines()]
        assert [int(t[0]) for t in tok] == want_idx.tolist() and [int(t[1]) for t in tok] == q[want_idx].tolist()
        assert _same(np.array([float(t[2]) for t in tok]), want_val / st["terms"])


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "active_learning.py"), "--rounds", "2", "--per_round", "20", "--sweeps", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "uncertainty" in r.stdout and "random" in r.stdout
