"""GPU tests of the node conditionals (include/bisbm.h, "Node conditionals").

dS rows are compared with the oracle's Philox-mode transition_ratio (the sweep's own evaluator restated on the CPU; the
summation order differs, so to rounding: 1e-9 |dS| + 1e-12 |S|, the tolerance of sum_dS_close in tests/test_gpu_parity.py) and
with differences of the handle's own description length.  Everything after dS is checked against
distributed.numpy_conditional_row fed with the device's OWN dS rows (tests/test_conditionals.py ties that model to the literal
loop), and the pooled sums against per-chain terms added one chain at a time on the host: the order of the additions is part of
the definition, so those comparisons are on bit patterns.

The bound on P.  With x_s = beta (dS_s - dS_min) evaluated with the same two roundings on both sides (no FMA), the device's
w_s = exp(-x_s) differs from numpy's only through the two exponentials: each within 1 ulp of the true value, the device's
allowed 2, so |w_gpu - w_np| <= 3 * 2^-53 w <= 2 * 2^-52 w -- and were x_s itself one rounding apart, that would add
x_s 2^-53 relative; Z is K_own - 1 adds of non-negative terms, each term off by the above and each add rounding once:
(K_own - 1 + 2) 2^-52 relative; the divide rounds once more.  In all (K_own + 8 + x_s) 2^-52 P is a safe bound.  The entropy
adds, per non-zero P, P ln P with the device's ln (within 2 ulp) in K_own - 1 adds of terms of one sign:
(K_own + 8) 2^-52 relative, plus 2^-52 absolute for P so close to 1 that ln P is a few ulps of 1."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_align import overlap_tables
from test_gpu_pair_scores import _merge_until_mixed, _mixed_shapes_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
NA, NB = 903, 701
SEED = 9
SHAPES = [(4, 4), (6, 5), (32, 32), (64, 64), (200, 56), (1, 255)]
TIER_CASES = ["dense_low_tier", "mid_tier_low", "closed2_tier", "mid_tier", "direct_tier", "big_m_r"]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


_GRAPHS = {}


def _graph(hub):
    """the graph of test_gpu_foldin.py (903 + 701 nodes, about 9000 edges, the last two nodes of each type isolated); hub: node 0
    has 600 more entries (a row longer than 256)"""
    if hub not in _GRAPHS:
        _GRAPHS[hub] = cases.random_graph(5, NA, NB, 9000, 4, 4, 1 if hub else 0, 2)
    return _GRAPHS[hub]


ALONE_A, ALONE_B = 11, NA + 13


def _queries(rowptr, col):
    """both types: a repeated node, the isolated nodes, the node of the highest degree (the hub where there is one) and one of
    its neighbours, the two nodes that _make_alone leaves alone in their blocks, and a few more"""
    deg = np.diff(rowptr.astype(np.int64))
    top = int(np.argmax(deg))
    q = [5, NA + 7, 5, NA - 1, NA + NB - 1, top, int(col[rowptr[top]]), ALONE_A, ALONE_B, 17, NA + 100, NA - 3, NA + NB - 3, 400]
    return np.array(q, dtype=np.uint32)


def _model(rowptr, col, ka, kb, chains, seed=SEED, **kw):
    return B.BlockModel(O.contiguous_labels(NA, NB, ka, kb), syn.types_vector(NA, NB), ka + kb, ka, kb, 1.0, (rowptr, col),
                        n_chains=chains, seed=seed, **kw)


def _make_alone(m, ka, kb, chains):
    """every chain: the other nodes of the blocks of ALONE_A and ALONE_B move to the next block of their type (where the type
    has one), then the block state is rebuilt"""
    for c in chains:
        lab = m.get_memberships(c).astype(np.int64)
        for v, lo, k in ((ALONE_A, 0, ka), (ALONE_B, ka, kb)):
            if k < 2:
                continue
            r = lab[v]
            others = np.flatnonzero(lab == r)
            lab[others[others != v]] = lo + (r - lo + 1) % k
        m.set_memberships(lab.astype(np.uint32), chain=c)
    m.init_bisbm()


def _own(v, ka, kb, na=NA):
    return (ka, kb, 0) if v < na else (kb, ka, ka)  # K_own, K_oth, first label of the type


def _oracle(rowptr, col, na, nb, ka, kb, labels, seed):
    o = O.OracleModel(rowptr, col, na, nb, ka, kb, 1.0, np.asarray(labels, dtype=np.uint32))
    o.seed_philox(seed, 0)
    o.init_bisbm()
    return o


def _check_dS_against_oracle(m, o, queries, na, ka, kb, record_property):
    S = abs(o.entropy())
    lab = o.memberships()
    worst = 0.0
    for i, v in enumerate(queries):
        v = int(v)
        k_own, _, lo = _own(v, ka, kb, na)
        dS, _ = m.conditionals_last(i)
        assert dS.shape == (1, k_own)
        for s in range(k_own):
            want = o.transition_ratio(v, lo + s)[0]
            err = abs(dS[0, s] - want)
            worst = max(worst, err)
            assert err <= 1e-9 * abs(want) + 1e-12 * S, (i, v, s, dS[0, s], want)
        assert dS[0, int(lab[v]) - lo] == 0.0 and not np.signbit(dS[0, int(lab[v]) - lo])
    record_property("worst_abs_error", worst)
    record_property("S", S)
    print("worst |dS_gpu - dS_oracle| = %.3g, |S| = %.6g" % (worst, S))


@pytest.fixture(scope="module", params=[(ka, kb, False) for ka, kb in SHAPES] + [(6, 5, True), (200, 56, True)],
                ids=lambda p: "%d+%d%s" % (p[0], p[1], "-hub" if p[2] else ""))
def one_chain(request):
    """one chain after shuffle_bisbm and 3 sweeps, two nodes made alone in their blocks, one sample with the last rows kept:
    everything the tests below need, read once"""
    ka, kb, hub = request.param
    rowptr, col = _graph(hub)
    q = _queries(rowptr, col)
    m = _model(rowptr, col, ka, kb, 1)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    _make_alone(m, ka, kb, [0])
    m.conditionals_set(q, beta=1.0, keep_last=True)
    m.conditionals_accumulate()
    out = dict(ka=ka, kb=kb, hub=hub, rowptr=rowptr, col=col, q=q, m=m, labels=m.get_memberships(0), n_r=m.get_n_r(0),
               stats=m.conditionals_stats(), rows=[m.conditionals_last(i) for i in range(len(q))])
    yield out
    m.close()


def test_dS_is_the_oracles_transition_ratio(one_chain, record_property):
    d = one_chain
    o = _oracle(d["rowptr"], d["col"], NA, NB, d["ka"], d["kb"], d["labels"], SEED)
    deg = np.diff(d["rowptr"].astype(np.int64))
    assert deg[d["q"][3]] == 0 and deg[d["q"][4]] == 0 and d["q"][0] == d["q"][2]
    assert deg[d["q"][5]] > (256 if d["hub"] else 1)
    _check_dS_against_oracle(d["m"], o, d["q"], NA, d["ka"], d["kb"], record_property)
    assert _same(d["rows"][0][0], d["rows"][2][0]) and _same(d["rows"][0][1], d["rows"][2][1])  # the repeated node


def test_P_and_the_terms_are_the_numpy_model_of_the_devices_own_rows(one_chain):
    d = one_chain
    ka, kb, st = d["ka"], d["kb"], d["stats"]
    assert st["terms"] == 1
    not_free = set()
    for i, v in enumerate(d["q"]):
        v = int(v)
        k_own, _, lo = _own(v, ka, kb)
        r = int(d["labels"][v]) - lo
        free = k_own > 1 and d["n_r"][lo + r] > 1
        dS, P = d["rows"][i][0][0], d["rows"][i][1][0]
        Pn, stay, ent, margin = D.numpy_conditional_row(dS, r, free, 1.0)
        x = 1.0 * (dS - dS.min())
        assert (np.abs(P - Pn) <= (k_own + 8 + np.minimum(x, 700.0)) * EPS * Pn).all(), (i, v, np.abs(P - Pn).max())
        assert (P[Pn == 0.0] == 0.0).all()
        assert abs(P.sum() - 1.0) <= (k_own + 4) * EPS
        # the chain's terms from the device's own rows (one chain, one sample: 0.0 + term keeps the term's bits)
        assert _same(st["stay"][i], P[r])
        ent_np = 0.0 - float(sum(p * np.log(p) for p in P if p != 0.0))
        assert abs(st["entropy"][i] - ent_np) <= (k_own + 8) * EPS * abs(ent_np) + EPS, (i, st["entropy"][i], ent_np)
        if free:
            assert st["free"][i] == 1 and _same(st["margin"][i], np.delete(dS, r).min())
        else:
            not_free.add(v)
            assert st["free"][i] == 0 and st["margin"][i] == 0.0
            assert P[r] == 1.0 and P.sum() == 1.0 and st["stay"][i] == 1.0 and st["entropy"][i] == 0.0
    # the nodes made alone (where their type has two blocks) and every node of a one-block type are not free
    # (with many blocks a queried node may be alone in its block by itself)
    want = {int(v) for v in d["q"] if (_own(int(v), ka, kb)[0] < 2) or int(v) in (ALONE_A, ALONE_B)}
    assert want and want <= not_free


@pytest.mark.parametrize("name", TIER_CASES)
def test_dS_through_the_log_q_tiers(name, record_property):
    _, na, nb, ne, ka, kb, eps, hubs, iso = cases.CASE[name]
    rowptr, col = cases.random_graph(11, na, nb, ne, ka, kb, hubs, iso)
    m = B.BlockModel(O.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, eps, (rowptr, col), n_chains=1, seed=SEED)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    q = np.random.default_rng(4).choice(na + nb, 200, replace=False).astype(np.uint32)
    m.conditionals_set(q, keep_last=True)
    m.conditionals_accumulate()
    o = _oracle(rowptr, col, na, nb, ka, kb, m.get_memberships(0), SEED)
    tiers = cases.tier_counts(o.m_r(), o.n_r())
    assert tiers[cases.CASE_TIERS[name]] >= 1, tiers
    _check_dS_against_oracle(m, o, q, na, ka, kb, record_property)
    m.close()


def test_dS_is_the_change_of_the_handles_own_description_length(record_property):
    ka, kb = 6, 5
    rowptr, col = _graph(True)
    q = _queries(rowptr, col)
    m = _model(rowptr, col, ka, kb, 1)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    m.conditionals_set(q, keep_last=True)
    m.conditionals_accumulate()
    lab = m.get_memberships(0)
    S0 = float(m.entropy()[0])
    rows = [m.conditionals_last(i)[0][0] for i in range(len(q))]
    rng = np.random.default_rng(8)
    worst, pairs = 0.0, 0
    for _ in range(20):
        i = int(rng.integers(len(q)))
        v = int(q[i])
        k_own, _, lo = _own(v, ka, kb)
        s = int(rng.integers(k_own - 1))
        s += s >= int(lab[v]) - lo  # (a target other than r)
        moved = lab.copy()
        moved[v] = lo + s
        m.set_memberships(moved)
        m.init_bisbm()
        err = abs(rows[i][s] - (float(m.entropy()[0]) - S0))
        worst = max(worst, err)
        assert err <= 1e-9 * abs(S0), (v, s, rows[i][s], float(m.entropy()[0]) - S0)
        pairs += 1
    record_property("worst_abs_error", worst)
    assert pairs == 20
    m.close()


def _chain_terms(helper, m, chains):
    """{chain: stats of the one-chain handle `helper` set to the chain's labels}: the device's own terms of every chain"""
    out = {}
    for c in chains:
        helper.set_memberships(m.get_memberships(c))
        helper.init_bisbm()
        helper.conditionals_reset()
        helper.conditionals_accumulate()
        out[c] = helper.conditionals_stats()
    return out


def _add_terms(total, terms, chains):
    for c in chains:
        t = terms[c]
        total["stay"] = total["stay"] + t["stay"]
        total["entropy"] = total["entropy"] + t["entropy"]
        total["margin"] = np.where(t["free"] > 0, total["margin"] + t["margin"], total["margin"])
        total["free"] = total["free"] + t["free"]


def _zero(Q):
    return {"stay": np.zeros(Q), "entropy": np.zeros(Q), "margin": np.zeros(Q), "free": np.zeros(Q, dtype=np.uint64)}


def _check_stats(st, total, terms):
    assert st["terms"] == terms
    for key in ("stay", "entropy", "margin"):
        assert _same(st[key], total[key]), (key, np.abs(st[key] - total[key]).max())
    assert (st["free"] == total["free"]).all()


def _check_last_against_terms(m, q, terms, ka, kb):
    """stay and margin of the per-chain terms are what the last rows hold; chains outside `terms` have NaN rows"""
    for i, v in enumerate(q):
        k_own, _, lo = _own(int(v), ka, kb)
        dS, P = m.conditionals_last(i)
        for c in range(m.n_chains):
            if c not in terms:
                assert np.isnan(dS[c]).all() and np.isnan(P[c]).all()
                continue
            r = int(m.get_memberships(c)[int(v)]) - lo
            assert _same(terms[c]["stay"][i], P[c, r]) and dS[c, r] == 0.0
            if terms[c]["free"][i]:
                assert _same(terms[c]["margin"][i], np.delete(dS[c], r).min())


def test_pooled_sums_six_chains_three_samples_reset_and_set():
    ka, kb, chains = 6, 5, 6
    rowptr, col = _graph(True)
    q = _queries(rowptr, col)
    m = _model(rowptr, col, ka, kb, chains)
    helper = _model(rowptr, col, ka, kb, 1)
    m.shuffle_bisbm()
    helper.shuffle_bisbm()
    m.conditionals_set(q, beta=0.8, keep_last=True)
    helper.conditionals_set(q, beta=0.8)
    with pytest.raises(B.BisbmError) as e:  # before the first sample
        m.conditionals_last(0)
    assert e.value.code == B.BISBM_ERR_STATE and "sample" in str(e.value)
    total = _zero(len(q))
    for sample in range(3):
        m.run_sweeps(2)
        if sample == 1:
            _make_alone(m, ka, kb, [1, 4])
        terms = _chain_terms(helper, m, range(chains))
        _add_terms(total, terms, range(chains))
        m.conditionals_accumulate()
        _check_last_against_terms(m, q, terms, ka, kb)
    st = m.conditionals_stats()
    _check_stats(st, total, 18)
    assert (st["free"] < 18).any() and (st["free"] == 18).any()
    # the sums survive a merge; the next sample adds the merged chains' terms
    m.agg_merge(1, 1)
    helper.agg_merge(1, 1)
    assert m.ka_kb(0) == (5, 4)
    _check_stats(m.conditionals_stats(), total, 18)
    m.run_sweeps(1)
    terms = _chain_terms(helper, m, range(chains))
    _add_terms(total, terms, range(chains))
    m.conditionals_accumulate()
    _check_stats(m.conditionals_stats(), total, 24)
    _check_last_against_terms(m, q, terms, 5, 4)
    # reset zeroes and keeps the queries
    m.conditionals_reset()
    _check_stats(m.conditionals_stats(), _zero(len(q)), 0)
    m.conditionals_accumulate()
    one = _zero(len(q))
    _add_terms(one, terms, range(chains))
    _check_stats(m.conditionals_stats(), one, chains)
    # set replaces; without keep_last the rows are refused
    m.conditionals_set(q[:3][::-1].copy(), beta=0.8)
    _check_stats(m.conditionals_stats(), _zero(3), 0)
    m.conditionals_accumulate()
    st = m.conditionals_stats()
    assert st["terms"] == chains and _same(st["stay"], one["stay"][:3][::-1]) and _same(st["entropy"], one["entropy"][:3][::-1])
    with pytest.raises(B.BisbmError) as e:
        m.conditionals_last(0)
    assert e.value.code == B.BISBM_ERR_STATE and "KEEP_LAST" in str(e.value)
    with pytest.raises(IndexError):
        m.conditionals_last(3)
    # every node
    m.conditionals_set(None)
    m.conditionals_accumulate()
    st = m.conditionals_stats()
    assert st["stay"].shape == (NA + NB,) and st["terms"] == chains and (st["stay"] > 0).all() and (st["stay"] <= chains * (1 + 16 * EPS)).all()
    # set([]) frees everything
    m.conditionals_set([])
    with pytest.raises(B.BisbmError) as e:
        m.conditionals_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "queries" in str(e.value)
    m.close()
    helper.close()


def test_refusals():
    rowptr, col = _graph(False)
    q = _queries(rowptr, col)
    m = _model(rowptr, col, 6, 5, 2)
    for call in (m.conditionals_accumulate, m.conditionals_stats, m.conditionals_marginals, lambda: m.conditionals_set_reference(m.get_memberships(0))):
        with pytest.raises(B.BisbmError) as e:  # no queries
            call()
        assert e.value.code == B.BISBM_ERR_STATE and "queries" in str(e.value)
    m.conditionals_set(q)
    with pytest.raises(B.BisbmError) as e:  # no block state yet
        m.conditionals_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "bisbm_init" in str(e.value)
    m.init_bisbm()
    m.conditionals_accumulate()
    before = m.conditionals_stats()
    bad = [(dict(nodes=[3, 5, NA + NB, 2]), "query 2"), (dict(nodes=[NA + NB + 7]), "query 0"),
           (dict(nodes=q, beta=0.0), "beta"), (dict(nodes=q, beta=-1.0), "beta"), (dict(nodes=q, beta=float("nan")), "beta"),
           (dict(nodes=q, beta=float("inf")), "beta")]
    for kw, names in bad:
        with pytest.raises(B.BisbmError) as e:
            m.conditionals_set(**kw)
        assert e.value.code == B.BISBM_ERR_INVALID_ARG and names in str(e.value), (kw, str(e.value))
        after = m.conditionals_stats()  # the earlier queries and their sums are intact
        assert after["terms"] == 2 and _same(after["stay"], before["stay"]) and _same(after["entropy"], before["entropy"])
    for what in (2, 3, 1 << 31):
        with pytest.raises(B.BisbmError) as e:
            m._check(m._L.bisbm_conditionals_set(m._h, len(q), B._p(q, B._u32p), 1.0, what))
        assert e.value.code == B.BISBM_ERR_INVALID_ARG and "what" in str(e.value)
    assert m.conditionals_stats()["terms"] == 2
    with pytest.raises(B.BisbmError) as e:  # no reference
        m.conditionals_marginals()
    assert e.value.code == B.BISBM_ERR_STATE and "reference" in str(e.value)
    with pytest.raises(B.BisbmError) as e:  # a reference label of the wrong type
        m.conditionals_set_reference(np.zeros(NA + NB, dtype=np.uint32))
    assert e.value.code == B.BISBM_ERR_INVALID_ARG
    m.close()
    # compat mode: refused at set
    c = _model(rowptr, col, 6, 5, 1, rng="mt19937-compat", gen_seed=10)
    c.shuffle_bisbm()
    with pytest.raises(B.BisbmError) as e:
        c.conditionals_set(q)
    assert e.value.code == B.BISBM_ERR_UNSUPPORTED and "COMPAT" in str(e.value)
    c.close()
    # a wide handle (two-byte labels): refused at accumulate
    name, na, nb, ne, ka, kb, eps, hubs, isolated = cases.CASE["wide_labels"]
    wr, wc = cases.random_graph(5, na, nb, ne, ka, kb, hubs, isolated)
    w = B.BlockModel(O.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, eps, (wr, wc), n_chains=1, seed=2)
    w.shuffle_bisbm()
    w.conditionals_set([0, na])
    with pytest.raises(B.BisbmError) as e:
        w.conditionals_accumulate()
    assert e.value.code == B.BISBM_ERR_UNSUPPORTED and "byte labels" in str(e.value)
    w.close()


def _soft_model(prob, m, q, ka, kb, chains):
    """prob[q][perm_c(s) - base] += P_c(s) for the given chains in order, perm_c from the host solver on the numpy overlap table,
    P from the last rows"""
    ref = m._soft_ref
    perms = {}
    for c in chains:
        ca, cb = overlap_tables(m.get_memberships(c), ref, NA, ka, kb)
        perms[c] = (B.align_assignment(ca)[0].astype(np.int64), B.align_assignment(cb)[0].astype(np.int64))
    for i, v in enumerate(q):
        k_own = _own(int(v), ka, kb)[0]
        P = m.conditionals_last(i)[1]
        for c in chains:
            perm = perms[c][1 if v >= NA else 0]
            for s in range(k_own):
                prob[i, perm[s]] = prob[i, perm[s]] + P[c, s]


def test_soft_marginals_against_the_alignment_model():
    ka, kb, chains = 6, 5, 6
    rowptr, col = _graph(True)
    q = _queries(rowptr, col)
    m = _model(rowptr, col, ka, kb, chains)
    m.shuffle_bisbm()
    m.run_sweeps(4)
    m.conditionals_set(q, keep_last=True)
    m._soft_ref = m.get_memberships(2)
    m.conditionals_set_reference(m._soft_ref)
    prob = np.zeros((len(q), max(ka, kb)))
    for _ in range(2):
        m.run_sweeps(2)
        m.conditionals_accumulate()
        _soft_model(prob, m, q, ka, kb, range(chains))
    got, terms = m.conditionals_marginals()
    assert terms == 12 and got.shape == prob.shape
    assert _same(got, prob), np.abs(got - prob).max()
    assert (np.abs(got.sum(axis=1) - terms) <= (max(ka, kb) + 4) * terms * EPS).all()
    for i, v in enumerate(q):
        assert (got[i, _own(int(v), ka, kb)[0]:] == 0).all()
    # reset zeroes prob and keeps the reference
    m.conditionals_reset()
    got, terms = m.conditionals_marginals()
    assert terms == 0 and (got == 0).all()
    m.conditionals_accumulate()
    assert m.conditionals_marginals()[1] == chains
    # a merge: the reference is stale until it is set again, and prob then starts afresh while the label-free sums go on
    m.agg_merge(1, 1)
    with pytest.raises(B.BisbmError) as e:
        m.conditionals_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "set it again" in str(e.value)
    assert m.conditionals_stats()["terms"] == chains
    m._soft_ref = m.get_memberships(0)
    m.conditionals_set_reference(m._soft_ref)
    m.run_sweeps(1)
    m.conditionals_accumulate()
    fresh = np.zeros((len(q), 5))
    _soft_model(fresh, m, q, 5, 4, range(chains))
    got, terms = m.conditionals_marginals()
    assert terms == chains and _same(got, fresh) and m.conditionals_stats()["terms"] == 2 * chains
    # clearing the reference
    m.conditionals_set_reference(None)
    with pytest.raises(B.BisbmError) as e:
        m.conditionals_marginals()
    assert e.value.code == B.BISBM_ERR_STATE and "reference" in str(e.value)
    m.conditionals_accumulate()  # (the label-free sums need none)
    assert m.conditionals_stats()["terms"] == 3 * chains
    m.close()


@pytest.mark.parametrize("entries", [2, 3])
def test_device_entries_of_one_device(entries):
    """every device entry keeps the sums of its own chains, and they are added in device order when read: the terms of the
    single handle's chains added entry by entry give the bits; the last rows are the single handle's"""
    ka, kb, chains = 5, 6, 6
    rowptr, col = _graph(True)
    q = _queries(rowptr, col)
    one = _model(rowptr, col, ka, kb, chains)
    many = _model(rowptr, col, ka, kb, chains, devices=[0] * entries)
    helper = _model(rowptr, col, ka, kb, 1)
    helper.shuffle_bisbm()
    helper.conditionals_set(q, beta=1.3)
    per = chains // entries
    parts = [_zero(len(q)) for _ in range(entries)]
    probs = [np.zeros((len(q), max(ka, kb))) for _ in range(entries)]
    for m in (one, many):
        m.shuffle_bisbm()
        m.conditionals_set(q, beta=1.3, keep_last=True)
    one._soft_ref = one.get_memberships(1)
    for m in (one, many):
        m.conditionals_set_reference(one._soft_ref)
    for _ in range(2):
        for m in (one, many):
            m.run_sweeps(2)
            m.conditionals_accumulate()
        terms = _chain_terms(helper, one, range(chains))
        for d in range(entries):
            _add_terms(parts[d], terms, range(d * per, (d + 1) * per))
            _soft_model(probs[d], one, q, ka, kb, range(d * per, (d + 1) * per))
    for c in range(chains):
        assert (one.get_memberships(c) == many.get_memberships(c)).all()
    for i in range(len(q)):
        a, b = one.conditionals_last(i), many.conditionals_last(i)
        assert _same(a[0], b[0]) and _same(a[1], b[1]), i
    total, prob = parts[0], probs[0]
    for d in range(1, entries):
        for key in ("stay", "entropy", "margin", "free"):
            total[key] = total[key] + parts[d][key]
        prob = prob + probs[d]
    _check_stats(many.conditionals_stats(), total, 2 * chains)
    got, terms = many.conditionals_marginals()
    assert terms == 2 * chains and _same(got, prob)
    many.conditionals_reset()
    _check_stats(many.conditionals_stats(), _zero(len(q)), 0)
    assert many.conditionals_marginals()[1] == 0
    for m in (one, many, helper):
        m.close()


def test_chains_grouped_by_shape_serve_stats_and_last_rows_and_refuse_a_reference():
    g, deg, na, nb = _mixed_shapes_model()
    q = np.array([3, na + 4, 3, na - 1, na + nb - 1, int(np.argmax(deg)), 77, na + 55], dtype=np.uint32)
    g.conditionals_set(q, keep_last=True)
    _merge_until_mixed(g)
    shapes = [g.ka_kb(c) for c in range(g.n_chains)]
    order = sorted(range(g.n_chains), key=lambda c: (shapes.index(shapes[c]), c))  # groups in order of first appearance
    assert len(set(shapes)) >= 2 and order != list(range(g.n_chains))
    g.run_sweeps(1)
    g.conditionals_accumulate()
    st = g.conditionals_stats()
    assert st["terms"] == g.n_chains
    stay, margin, free = np.zeros(len(q)), np.zeros(len(q)), np.zeros(len(q), dtype=np.uint64)
    ent_lo, ent_hi = np.zeros(len(q)), np.zeros(len(q))
    rows = [g.conditionals_last(i) for i in range(len(q))]
    for c in order:
        ka, kb = shapes[c]
        lab, n_r = g.get_memberships(c), g.get_n_r(c)
        for i, v in enumerate(q):
            k_own, _, lo = _own(int(v), ka, kb, na)
            r = int(lab[int(v)]) - lo
            dS, P = rows[i][0][c], rows[i][1][c]
            assert (dS[k_own:] == 0).all() and (P[k_own:] == 0).all() and abs(P[:k_own].sum() - 1) <= (k_own + 4) * EPS
            stay[i] = stay[i] + P[r]
            if k_own > 1 and n_r[lo + r] > 1:
                margin[i] = margin[i] + np.delete(dS[:k_own], r).min()
                free[i] += 1
            ent = 0.0 - float(sum(p * np.log(p) for p in P[:k_own] if p != 0.0))
            tol = (k_own + 8) * EPS * abs(ent) + EPS
            ent_lo[i], ent_hi[i] = ent_lo[i] + ent - tol, ent_hi[i] + ent + tol
    assert _same(st["stay"], stay) and _same(st["margin"], margin) and (st["free"] == free).all()
    slack = g.n_chains * EPS * np.abs(ent_hi)  # (the rounding of the adds themselves)
    assert (st["entropy"] >= ent_lo - slack).all() and (st["entropy"] <= ent_hi + slack).all()
    with pytest.raises(B.BisbmError) as e:
        g.conditionals_set_reference(g.get_memberships(0))
    assert e.value.code == B.BISBM_ERR_STATE
    g.close()
    # replica exchange over chains grouped by shape is refused
    g, deg, na, nb = _mixed_shapes_model()
    g.set_tempering([1.0, 1.3, 2.0, 3.5])
    g.conditionals_set(q)
    _merge_until_mixed(g)
    with pytest.raises(B.BisbmError) as e:
        g.conditionals_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "grouped by shape" in str(e.value)
    g.close()


def test_replica_exchange_counts_the_chains_on_rung_0():
    ka, kb, chains, ladder = 5, 5, 6, [1.0, 1.5, 2.2]
    rowptr, col = _graph(False)
    q = _queries(rowptr, col)
    m = _model(rowptr, col, ka, kb, chains)
    helper = _model(rowptr, col, ka, kb, 1)
    helper.shuffle_bisbm()
    helper.conditionals_set(q)
    m.shuffle_bisbm()
    m.set_tempering(ladder)
    m.tempering_run(2, 1)
    m.conditionals_set(q, keep_last=True)
    total = _zero(len(q))
    for sample in range(1, 3):
        m.tempering_run(3, 1)
        cold = [int(c) for c in np.flatnonzero(m.tempering_state()[0] == 0)]
        assert len(cold) == chains // 3
        terms = _chain_terms(helper, m, cold)
        _add_terms(total, terms, cold)
        m.conditionals_accumulate()
        assert m.conditionals_stats()["terms"] == sample * chains // 3
        _check_last_against_terms(m, q, terms, ka, kb)  # NaN rows for the chains off rung 0
    _check_stats(m.conditionals_stats(), total, 2 * chains // 3)
    m.close()
    helper.close()


def test_a_conditional_sample_touches_nothing():
    ka, kb, chains = 6, 5, 4
    rowptr, col = _graph(True)
    q = _queries(rowptr, col)
    a, b = _model(rowptr, col, ka, kb, chains), _model(rowptr, col, ka, kb, chains)
    for m in (a, b):
        m.shuffle_bisbm()
        m.run_sweeps(2)
    b.conditionals_set(q, keep_last=True)
    b.conditionals_set_reference(b.get_memberships(0))
    b.conditionals_accumulate()
    b.conditionals_accumulate()

    def state(m):
        return [(m.get_memberships(c), m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c)) for c in range(chains)], m.get_entropy()
    for step in range(2):
        sa, sb = state(a), state(b)
        for c in range(chains):
            assert all((x == y).all() for x, y in zip(sa[0][c], sb[0][c])), (step, c)
        assert _same(sa[1], sb[1])
        for m in (a, b):
            m.run_sweeps(1)
    a.close()
    b.close()


def test_marginalize_and_the_cli_reproduce_the_python_calls(tmp_path):
    rowptr, col, na, nb = O.load_graph("n_1000")
    n, chains, seed, beta = na + nb, 8, 5, 0.7
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    q = np.array([0, na + 3, 17, 0, na - 1, n - 1, 250, na + 250], dtype=np.uint32)
    qin, qout = tmp_path / "nodes.txt", tmp_path / "out.txt"
    qin.write_text("".join("%d\n" % v for v in q[:3]) + "\n" + "".join("%d\n" % v for v in q[3:]))
    labels0 = O.contiguous_labels(na, nb, 3, 3)

    def model():
        m = B.BlockModel(labels0, syn.types_vector(na, nb), 6, 3, 3, 1.0, (rowptr, col), n_chains=chains, seed=seed)
        m.shuffle_bisbm()
        return m
    # marginalize(conditionals=...) is the Python calls
    m = model()
    labels, _, st, (prob, prob_terms) = B.marginalize(m, 10, 3, 2, align=True, conditionals=(q, beta))
    assert st["terms"] == prob_terms == 3 * chains and len(labels) == n and prob.shape == (len(q), 3)
    m2 = model()
    m2.run_sweeps(10)
    m2.marginals_reset()
    m2.marginals_set_alignment(True)
    m2.conditionals_set(q, beta)
    for sample in range(3):
        m2.run_sweeps(2)
        m2.marginals_accumulate(None)
        if sample == 0:
            m2.conditionals_set_reference(m2.marginals_reference()[0])
        m2.conditionals_accumulate()
    st2 = m2.conditionals_stats()
    assert all(_same(st[k], st2[k]) for k in ("stay", "entropy", "margin")) and (st["free"] == st2["free"]).all()
    assert _same(prob, m2.conditionals_marginals()[0])
    m.close()
    m2.close()
    # without align: the stats only
    m = model()
    out = B.marginalize(m, 10, 3, 2, conditionals=(q, beta))
    assert len(out) == 3 and all(_same(out[2][k], st[k]) for k in ("stay", "entropy", "margin"))
    m.close()
    # the command line
    sizes = [str(x) for x in np.bincount(labels0)]
    base = [cli, "-e", el, "-y", str(na), str(nb), "-z", "3", "3", "-n", *sizes, "-r", "-d", str(seed), "--rng", "philox",
            "--chains", str(chains), "-b", str(10 * n), "-t", str(6 * n), "-f", str(2 * n), "--marginalize"]
    for align in (True, False):
        r = subprocess.run(base + (["--align"] if align else []) + ["--conditionals", str(qin), str(qout), "--conditionals_beta", str(beta)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert len(r.stdout.split()) == n  # (stdout: the marginal labels still)
        lines = qout.read_text().splitlines()
        assert len(lines) == len(q)
        for i, line in enumerate(lines):
            tok = line.split()
            assert int(tok[0]) == q[i] and len(tok) == 4 + (3 if align else 0)
            vals = np.array([float(t) for t in tok[1:]])
            want = [st["stay"][i] / st["terms"], st["entropy"][i] / st["terms"], st["margin"][i] / st["free"][i] if st["free"][i] else np.nan]
            if align:
                want += list(prob[i] / prob_terms)
            want = np.array(want)
            assert ((_bits(vals) == _bits(want)) | (np.isnan(vals) & np.isnan(want))).all(), (i, vals, want)


def test_example_runs():
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "uncertain_nodes.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "least settled nodes" in r.stdout, r.stdout + r.stderr
