"""GPU tests of the fold-in queries (include/bisbm.h, "Fold-in queries").  The model is distributed.numpy_foldin_tables /
numpy_foldin_rows (tests/test_foldin.py checks it against the literal double loop), fed with what the handle's own getters
return for every counted chain at every sample and added ONE CHAIN AT A TIME onto a running total -- the order of the additions
is part of the definition.  Posteriors, rows and top-k are compared on their bit patterns throughout; the ranking's model is
distributed.numpy_query_topk applied to the rows get_row returns.

The two row-sum invariants hold up to rounding: the terms are non-negative, so the bound is n_candidates 2^-52 relative for one
chain (the derivation of test_gpu_pair_scores.py's docstring)."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_gpu_pair_scores import _merge_until_mixed, _mixed_shapes_model, _planted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
NONE = 0xFFFFFFFF
REC, SIM = B.FOLDIN_RECOMMEND, B.FOLDIN_SIMILAR
NA, NB = 903, 701  # neither count is a multiple of 4, and type b does not start on a label word
ALPHA = 0.25


def _graph(isolated=2, seed=5):
    """about 9000 edges on 903 + 701 nodes; the last `isolated` nodes of each type have no edge"""
    rowptr, col = cases.random_graph(seed, NA, NB, 9000, 4, 4, 0, isolated)
    return rowptr, col, np.diff(rowptr.astype(np.int64))


def _model(rowptr, col, na, nb, ka, kb, chains, seed=9, **kw):
    return B.BlockModel(O.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rowptr, col),
                        n_chains=chains, seed=seed, **kw)


def _virtual_nodes(na=NA, nb=NB, isolated=True):
    """11 virtual nodes, both types mixed: lists of 1, 2, 8 and 300 entries (longer than the 256 labels the table kernel gathers
    at a time), a node listed three times, lists that name an isolated node, and two identical virtual nodes (2 and 8)"""
    rs = np.random.default_rng(2)

    def b(k):
        return (na + rs.integers(0, nb - 2, k)).tolist()

    def a(k):
        return rs.integers(0, na - 2, k).tolist()
    eight = b(8)
    last_a, last_b = (na - 1, na + nb - 1) if isolated else (na - 3, na + nb - 3)
    nodes = [("a", b(1)), ("b", a(2)), ("a", eight), ("b", a(300)), ("a", b(300)), ("a", [na + 7, na + 9, na + 7, na + 7, na + 11]),
             ("b", [last_a, 5]), ("a", [last_b]), ("a", list(eight)), ("b", a(8)), ("b", [3])]
    assert len(nodes) == 11
    return nodes


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _chain(m, deg, nodes, alpha, c):
    """the model's (P, recommend row, similar row) of every virtual node in chain c, from the handle's getters"""
    lab, mm, mr, nr = m.get_memberships(c), m.get_m(c), m.get_m_r(c), m.get_n_r(c)
    ka = m.ka_kb(c)[0]
    out = []
    for t, ids in nodes:
        qt = 1 if t == "b" else 0
        P, g = D.numpy_foldin_tables(lab, mm, mr, nr, ka, qt, ids, alpha)
        rec, sim = D.numpy_foldin_rows(lab, deg, m.na, ka, qt, len(ids), P, g)
        out.append((P, rec, sim))
    return out


def _add_chains(total, m, deg, nodes, alpha, chains):
    """the given chains' terms added onto total[i] = [recommend row, similar row] one chain at a time, in the given order;
    returns the posteriors of the chains, [chain][node]"""
    post = {}
    for c in chains:
        terms = _chain(m, deg, nodes, alpha, c)
        for i, (P, rec, sim) in enumerate(terms):
            if total[i] is None:
                total[i] = [np.zeros(len(rec)), np.zeros(len(sim))]
            total[i][0] += rec
            total[i][1] += sim
        post[c] = [P for P, _, _ in terms]
    return post


def _rows(m, n_nodes, kinds=(REC, SIM)):
    got = [[m.foldin_scores(i, what) for what in kinds] for i in range(n_nodes)]
    assert len({t for row in got for _, t in row}) == 1
    return [[r for r, _ in row] for row in got], got[0][0][1]


def _check_rows(rows, total):
    for i in range(len(total)):
        for kind in range(2):
            assert _same(rows[i][kind], total[i][kind]), (i, kind, np.abs(rows[i][kind] - total[i][kind]).max())


def _check_posteriors(m, nodes, post):
    """foldin_posteriors against the model's: the rows of the chains in `post`, NaN rows for all others"""
    for i, (t, _) in enumerate(nodes):
        got = m.foldin_posteriors(i)
        assert got.shape[0] == m.n_chains
        for c in range(m.n_chains):
            if c in post:
                P = post[c][i]
                assert _same(got[c, :len(P)], P) and (got[c, len(P):] == 0).all(), (i, c)
            else:
                assert np.isnan(got[c]).all(), (i, c)


def _check_topk(m, nodes, rows, ks=(1, 10, 64)):
    """topk == numpy_query_topk of get_row's rows, integers and bits; returns the (kind, k, node) whose k-th and (k+1)-th
    eligible sums tie at a positive value"""
    tied = []
    for k in ks:
        for what, kind, excl in ((REC, 0, False), (REC, 0, True), (SIM, 1, False)):
            got_nodes, got_sums, terms = m.foldin_topk(what, k, exclude_listed=excl)
            assert got_nodes.shape == got_sums.shape == (len(nodes), k) and terms == m.foldin_scores(0, what)[1]
            for i, (t, ids) in enumerate(nodes):
                cand_b = (t == "a") == (what == REC)
                first = m.na if cand_b else 0
                listed = np.unique(np.asarray(ids, dtype=np.int64)) - first if excl else np.zeros(0, dtype=np.int64)
                idx, val = D.numpy_query_topk(rows[i][kind], k, listed)
                want = np.where(idx == NONE, NONE, idx.astype(np.int64) + first).astype(np.uint32)
                assert (got_nodes[i] == want).all(), (what, k, excl, i, got_nodes[i], want)
                assert (_bits(got_sums[i]) == _bits(val)).all(), (what, k, excl, i)
                if excl:
                    assert not np.isin(got_nodes[i].astype(np.int64), listed + first).any()
                more, _ = D.numpy_query_topk(rows[i][kind], k + 1, listed)
                if more[k] != NONE and rows[i][kind][more[k]] == rows[i][kind][more[k - 1]] > 0:
                    tied.append((what, k, i))
    return tied


@pytest.mark.parametrize("ka,kb", [(4, 4), (6, 5), (32, 32), (64, 64), (200, 56), (1, 255)])
def test_one_chain_one_sample_is_the_model_bit_for_bit(ka, kb):
    rowptr, col, deg = _graph()
    nodes = _virtual_nodes()
    m = _model(rowptr, col, NA, NB, ka, kb, 1)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    m.foldin_set(nodes, ALPHA)
    m.foldin_accumulate()
    rows, terms = _rows(m, len(nodes))
    total = [None] * len(nodes)
    post = _add_chains(total, m, deg, nodes, ALPHA, [0])
    assert terms == 1
    for i, (t, ids) in enumerate(nodes):
        assert rows[i][0].shape == ((NB,) if t == "a" else (NA,)) and rows[i][1].shape == ((NA,) if t == "a" else (NB,))
    _check_rows(rows, total)
    _check_posteriors(m, nodes, post)
    assert _same(rows[2][0], rows[8][0]) and _same(rows[2][1], rows[8][1]) and rows[2][0].max() > 0   # the identical virtual nodes
    assert (rows[0][0][NB - 2:] == 0).all() and (rows[1][0][NA - 2:] == 0).all()                      # isolated candidates
    # the invariants, on what the device returned
    m_r, n_r = m.get_m_r(0), m.get_n_r(0)
    for i, (t, ids) in enumerate(nodes):
        own = slice(ka, ka + kb) if t == "b" else slice(0, ka)
        P = post[0][i]
        assert abs(P.sum() - 1.0) <= 4 * EPS
        want = len(ids) * float(P[m_r[own] > 0].sum())
        assert abs(rows[i][0].sum() - want) <= len(rows[i][0]) * EPS * want, (i, rows[i][0].sum(), want)
        want = float((P * n_r[own]).sum())
        assert abs(rows[i][1].sum() - want) <= len(rows[i][1]) * EPS * want, (i, rows[i][1].sum(), want)
    m.close()


def test_six_chains_three_samples_reset_and_set():
    chains = 6
    rowptr, col, deg = _graph()
    nodes = _virtual_nodes()
    m = _model(rowptr, col, NA, NB, 6, 5, chains)
    m.shuffle_bisbm()
    m.foldin_set(nodes, ALPHA)
    with pytest.raises(B.BisbmError) as e:  # before the first sample
        m.foldin_posteriors(0)
    assert e.value.code == B.BISBM_ERR_STATE and "sample" in str(e.value)
    total = [None] * len(nodes)
    for _ in range(3):
        m.run_sweeps(3)
        post = _add_chains(total, m, deg, nodes, ALPHA, range(chains))
        m.foldin_accumulate()
    rows, terms = _rows(m, len(nodes))
    assert terms == 18
    _check_rows(rows, total)
    _check_posteriors(m, nodes, post)  # the last sample's
    # the sums survive a merge; the next sample adds the merged chains' terms
    m.agg_merge(1, 1)
    assert m.ka_kb(0) == (5, 4)
    rows, terms = _rows(m, len(nodes))
    assert terms == 18
    _check_rows(rows, total)
    m.run_sweeps(1)
    post = _add_chains(total, m, deg, nodes, ALPHA, range(chains))
    m.foldin_accumulate()
    rows, terms = _rows(m, len(nodes))
    assert terms == 24
    _check_rows(rows, total)
    _check_posteriors(m, nodes, post)
    # reset zeroes and keeps the virtual nodes
    m.foldin_reset()
    rows0, t0 = _rows(m, len(nodes))
    assert t0 == 0 and all((r == 0).all() for row in rows0 for r in row)
    m.foldin_accumulate()
    one = [None] * len(nodes)
    _add_chains(one, m, deg, nodes, ALPHA, range(chains))
    rows1, t1 = _rows(m, len(nodes))
    assert t1 == chains
    _check_rows(rows1, one)
    # set again replaces and zeroes; alpha defaults to the model's epsilon
    m.foldin_set(nodes[:3][::-1])
    rows2, t2 = _rows(m, 3)
    assert t2 == 0 and [len(r[0]) for r in rows2] == [NB, NA, NB] and all((r == 0).all() for row in rows2 for r in row)
    with pytest.raises(IndexError):
        m.foldin_scores(3, REC)
    m.foldin_accumulate()
    eps_total = [None] * 3
    _add_chains(eps_total, m, deg, nodes[:3][::-1], m.epsilon, range(chains))
    _check_rows(_rows(m, 3)[0], eps_total)
    # set([]) frees everything
    m.foldin_set([])
    with pytest.raises(B.BisbmError) as e:
        m.foldin_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "virtual nodes" in str(e.value)
    m.close()


@pytest.mark.parametrize("what,other", [(REC, SIM), (SIM, REC)])
def test_one_row_kind_only(what, other):
    chains = 3
    rowptr, col, deg = _graph()
    nodes = _virtual_nodes()
    m = _model(rowptr, col, NA, NB, 6, 5, chains)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    m.foldin_set(nodes, ALPHA)
    m.foldin_accumulate()
    both, _ = _rows(m, len(nodes))
    want_top = m.foldin_topk(what, 10)
    m.foldin_set(nodes, ALPHA, what=what)
    m.foldin_accumulate()
    rows, terms = _rows(m, len(nodes), kinds=(what,))
    assert terms == chains
    for i in range(len(nodes)):
        assert _same(rows[i][0], both[i][0 if what == REC else 1]), i
    got_top = m.foldin_topk(what, 10)
    assert (got_top[0] == want_top[0]).all() and (_bits(got_top[1]) == _bits(want_top[1])).all()
    for call in (lambda: m.foldin_scores(0, other), lambda: m.foldin_topk(other, 5), lambda: m.foldin_scores(0, REC | SIM),
                 lambda: m.foldin_topk(REC | SIM, 5), lambda: m.foldin_topk(0, 5)):
        with pytest.raises(B.BisbmError) as e:
            call()
        assert e.value.code == B.BISBM_ERR_INVALID_ARG, str(e.value)
    total = [None] * len(nodes)
    post = _add_chains(total, m, deg, nodes, ALPHA, range(chains))
    _check_posteriors(m, nodes, post)  # the posteriors do not depend on the kinds kept
    m.close()


@pytest.mark.parametrize("chains,samples", [(1, 1), (6, 2)])
def test_topk_is_the_host_ranking_of_the_rows(chains, samples):
    rowptr, col, deg = _graph()
    nodes = _virtual_nodes()
    m = _model(rowptr, col, NA, NB, 4, 4, chains)
    m.shuffle_bisbm()
    m.foldin_set(nodes, ALPHA)
    with pytest.raises(B.BisbmError) as e:  # before any sample
        m.foldin_topk(REC, 5)
    assert e.value.code == B.BISBM_ERR_STATE and "sample" in str(e.value)
    for _ in range(samples):
        m.run_sweeps(3)
        m.foldin_accumulate()
    rows, terms = _rows(m, len(nodes))
    assert terms == chains * samples
    tied = _check_topk(m, nodes, rows)
    # the tie rule is exercised: with one chain a similar row holds at most four different values
    if chains == 1:
        assert any(what == SIM for what, _, _ in tied), "no similar row has a tie at the k-th place: the tie rule goes untested"
    with pytest.raises(B.BisbmError) as e:
        m.foldin_topk(SIM, 5, exclude_listed=True)
    assert e.value.code == B.BISBM_ERR_INVALID_ARG and "exclude_listed" in str(e.value)
    with pytest.raises(B.BisbmError) as e:
        m.foldin_topk(REC, 0)
    assert e.value.code == B.BISBM_ERR_INVALID_ARG
    with pytest.raises(B.BisbmError) as e:
        m.foldin_topk(REC, B.QUERY_MAX_K + 1)
    assert e.value.code == B.BISBM_ERR_UNSUPPORTED and str(B.QUERY_MAX_K) in str(e.value)
    # the largest k: more than the 701 / 903 candidates, so every row is ranked in full and padded
    _check_topk(m, nodes, rows, ks=(B.QUERY_MAX_K,))
    m.close()


def test_topk_with_fewer_eligible_candidates_than_k():
    rowptr, col, na, nb = O.load_graph("southernWomen")
    nodes = [("a", [na + 1, na + 2, na + 2, na + 5]), ("b", list(range(na))), ("b", [0]), ("a", [na + j for j in range(nb - 1)])]
    m = B.BlockModel(O.contiguous_labels(na, nb, 3, 3), syn.types_vector(na, nb), 6, 3, 3, 0.001, (rowptr, col), n_chains=4, seed=5)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    m.foldin_set(nodes)
    m.foldin_accumulate()
    rows, terms = _rows(m, len(nodes))
    assert terms == 4
    _check_topk(m, nodes, rows)
    got, sums, _ = m.foldin_topk(REC, 10, exclude_listed=True)
    assert (got[1] == NONE).all() and (sums[1] == 0).all()                     # every candidate is listed
    assert got[3, 0] == na + nb - 1 and (got[3, 1:] == NONE).all()             # one candidate is left
    assert (got[0, :nb - 3] != NONE).all() and (got[0, nb - 3:] == NONE).all()  # three distinct nodes are listed
    m.close()


def test_replica_exchange_counts_the_cold_chains():
    chains, ladder = 8, [1.0, 1.6]
    rowptr, col, deg = _graph()
    nodes = _virtual_nodes()
    m = _model(rowptr, col, NA, NB, 5, 5, chains)
    m.shuffle_bisbm()
    m.set_tempering(ladder)
    m.tempering_run(2, 1)
    m.foldin_set(nodes, ALPHA)
    total = [None] * len(nodes)
    for sample in range(1, 3):
        m.tempering_run(3, 1)
        cold = np.flatnonzero(m.tempering_state()[0] == 0)
        assert len(cold) == chains // len(ladder)
        post = _add_chains(total, m, deg, nodes, ALPHA, cold)
        m.foldin_accumulate()
        assert m.foldin_scores(0, REC)[1] == 4 * sample
    rows, terms = _rows(m, len(nodes))
    assert terms == 8
    _check_rows(rows, total)
    _check_posteriors(m, nodes, post)  # NaN rows for the chains off rung 0
    m.close()


def test_chains_grouped_by_shape_are_added_group_by_group():
    g, deg, na, nb = _mixed_shapes_model()
    nodes = _virtual_nodes(na, nb, isolated=False)[:7]
    g.foldin_set(nodes, ALPHA)
    g.foldin_accumulate()  # one shape still
    total = [None] * len(nodes)
    _add_chains(total, g, deg, nodes, ALPHA, range(g.n_chains))
    assert not g.mixed_shapes
    _merge_until_mixed(g)
    shapes = [g.ka_kb(c) for c in range(g.n_chains)]
    order = sorted(range(g.n_chains), key=lambda c: (shapes.index(shapes[c]), c))  # groups in order of first appearance
    assert len(set(shapes)) >= 2 and order != list(range(g.n_chains))
    rows, terms = _rows(g, len(nodes))  # the sums survive the merge
    assert terms == 32
    _check_rows(rows, total)
    g.run_sweeps(1)
    post = _add_chains(total, g, deg, nodes, ALPHA, order)
    g.foldin_accumulate()
    rows, terms = _rows(g, len(nodes))
    assert terms == 64
    _check_rows(rows, total)
    _check_posteriors(g, nodes, post)  # rows of different lengths, padded with 0.0
    _check_topk(g, nodes, rows, ks=(10,))
    g.close()
    # replica exchange over chains grouped by shape is refused
    g, deg, na, nb = _mixed_shapes_model()
    g.set_tempering([1.0, 1.3, 2.0, 3.5])
    g.foldin_set(nodes, ALPHA)
    _merge_until_mixed(g)
    with pytest.raises(B.BisbmError) as e:
        g.foldin_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "grouped by shape" in str(e.value)
    g.close()


def test_a_device_listed_twice():
    chains = 6
    rowptr, col, deg = _graph()
    nodes = _virtual_nodes()
    m = _model(rowptr, col, NA, NB, 5, 6, chains, devices=[0, 0])
    m.shuffle_bisbm()
    m.foldin_set(nodes, ALPHA)
    dev = [[None] * len(nodes), [None] * len(nodes)]
    for _ in range(2):
        m.run_sweeps(2)
        post = _add_chains(dev[0], m, deg, nodes, ALPHA, range(0, chains // 2))
        post.update(_add_chains(dev[1], m, deg, nodes, ALPHA, range(chains // 2, chains)))
        m.foldin_accumulate()
    rows, terms = _rows(m, len(nodes))
    total = [[dev[0][i][kind] + dev[1][i][kind] for kind in range(2)] for i in range(len(nodes))]
    assert terms == 2 * chains
    _check_rows(rows, total)
    _check_posteriors(m, nodes, post)
    _check_topk(m, nodes, rows, ks=(10,))
    m.foldin_reset()
    rows0, t0 = _rows(m, len(nodes))
    assert t0 == 0 and all((r == 0).all() for row in rows0 for r in row)
    m.close()


def test_refusals():
    # a wide handle (two-byte labels)
    name, na, nb, ne, ka, kb, eps, hubs, isolated = cases.CASE["wide_labels"]
    rowptr, col = cases.random_graph(5, na, nb, ne, ka, kb, hubs, isolated)
    w = _model(rowptr, col, na, nb, ka, kb, 1, seed=2)
    w.foldin_set([("a", [na]), ("b", [0])], ALPHA)
    with pytest.raises(B.BisbmError) as e:  # before init
        w.foldin_accumulate()
    assert e.value.code in (B.BISBM_ERR_STATE, B.BISBM_ERR_UNSUPPORTED)
    w.shuffle_bisbm()
    with pytest.raises(B.BisbmError) as e:
        w.foldin_accumulate()
    assert e.value.code == B.BISBM_ERR_UNSUPPORTED and "byte labels" in str(e.value)
    w.close()
    m, deg = _planted(300, 200, 3000, 4, 4, 4)
    for call in (m.foldin_accumulate, lambda: m.foldin_scores(0, REC), lambda: m.foldin_topk(REC, 3)):
        with pytest.raises((B.BisbmError, IndexError)) as e:  # no virtual nodes
            call()
        assert isinstance(e.value, IndexError) or (e.value.code == B.BISBM_ERR_STATE and "virtual nodes" in str(e.value))
    nodes = [("a", [300, 301]), ("b", [5]), ("a", [499])]
    m.foldin_set(nodes, ALPHA)
    with pytest.raises(B.BisbmError) as e:  # no block state yet
        m.foldin_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "bisbm_init" in str(e.value)
    m.init_bisbm()
    m.foldin_accumulate()
    rows, terms = _rows(m, 3)
    bad = [(dict(nodes=[("a", [300]), ("b", [])]), "query 1"),                      # an empty list
           (dict(nodes=[("a", [300, 5])]), "query 0 position 1"),                   # a type-a node in a type-a node's list
           (dict(nodes=[("b", [5]), ("b", [5, 6, 300])]), "query 1 position 2"),
           (dict(nodes=[("a", [500])]), "query 0 position 0"),                      # not a node
           (dict(nodes=[("a", [300]), (2, [5])]), "query 1"),                       # a type above 1
           (dict(nodes=nodes, alpha=0.0), "alpha"), (dict(nodes=nodes, alpha=-1.0), "alpha"),
           (dict(nodes=nodes, alpha=float("nan")), "alpha"), (dict(nodes=nodes, alpha=float("inf")), "alpha"),
           (dict(nodes=nodes, what=0), "what"), (dict(nodes=nodes, what=4), "what"), (dict(nodes=nodes, what=7), "what")]
    for kw, names in bad:
        kw.setdefault("alpha", ALPHA)
        with pytest.raises(B.BisbmError) as e:
            m.foldin_set(**kw)
        assert e.value.code == B.BISBM_ERR_INVALID_ARG and names in str(e.value), (kw, str(e.value))
        rows2, t2 = _rows(m, 3)  # the earlier virtual nodes and their sums are intact
        assert t2 == terms == 4 and all(_same(rows2[i][kind], rows[i][kind]) for i in range(3) for kind in range(2))
    with pytest.raises(B.BisbmError) as e:  # a stride below K_own
        out = np.zeros(m.n_chains * 3)
        m._check(m._L.bisbm_foldin_get_posteriors(m._h, 0, 3, B._p(out, B._f64p)))
    assert e.value.code == B.BISBM_ERR_INVALID_ARG and "stride" in str(e.value)
    with pytest.raises(ValueError):
        m.foldin_set([("c", [300])])
    m.close()


def test_mt19937_compat_mode():
    c, deg = _planted(500, 400, 5000, 6, 5, 1, rng="mt19937-compat", gen_seed=10)
    c.shuffle_bisbm()
    c.run_sweeps(2)
    nodes = [("a", [500 + 7, 500 + 7, 899]), ("b", [7]), ("b", [499, 0, 250, 3])]
    c.foldin_set(nodes, ALPHA)
    c.foldin_accumulate()
    rows, terms = _rows(c, 3)
    total = [None] * 3
    post = _add_chains(total, c, deg, nodes, ALPHA, [0])
    assert terms == 1
    _check_rows(rows, total)
    _check_posteriors(c, nodes, post)
    c.close()


def _write_foldin(path, nodes, rec, sim):
    with open(path, "w") as f:
        for i in range(len(nodes)):
            for name, (got, scores, _) in (("recommend", rec), ("similar", sim)):
                for node, s in zip(got[i], scores[i]):
                    if node != NONE:
                        f.write("%d %s %d %s\n" % (i, name, node, "%.17g" % s))


def test_marginalize_and_the_cli_reproduce_the_python_calls(tmp_path):
    rowptr, col, na, nb = O.load_graph("southernWomen")
    n, chains, seed, k, alpha = na + nb, 8, 5, 5, 0.1
    el = os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    nodes = [("a", [na + 1, na + 2, na + 2, na + 5]), ("b", [0, 3, 4]), ("b", [17]), ("a", [na + 13])]
    qin, qout, want = tmp_path / "nodes.txt", tmp_path / "out.txt", tmp_path / "want.txt"
    qin.write_text("".join("%s %s\n" % (t, " ".join(str(v) for v in ids)) for t, ids in nodes[:2]) + "\n" +
                   "".join("%s %s\n" % (t, " ".join(str(v) for v in ids)) for t, ids in nodes[2:]))
    labels0 = O.contiguous_labels(na, nb, 3, 3)
    # marginalize(foldin=...) is the Python calls
    m = B.BlockModel(labels0, syn.types_vector(na, nb), 6, 3, 3, 1.0, (rowptr, col), n_chains=chains, seed=seed)
    m.shuffle_bisbm()
    labels, _, (rec, sim) = B.marginalize(m, 10, 3, 2, foldin=(nodes, k, alpha))
    assert rec[2] == sim[2] == 3 * chains and len(labels) == n
    m2 = B.BlockModel(labels0, syn.types_vector(na, nb), 6, 3, 3, 1.0, (rowptr, col), n_chains=chains, seed=seed)
    m2.shuffle_bisbm()
    m2.run_sweeps(10)
    m2.foldin_set(nodes, alpha)
    for _ in range(3):
        m2.run_sweeps(2)
        m2.foldin_accumulate()
    for got, ref in ((rec, m2.foldin_recommend(k)), (sim, m2.foldin_similar(k))):
        assert (got[0] == ref[0]).all() and (_bits(got[1]) == _bits(ref[1])).all() and got[2] == ref[2]
    assert not np.isin(rec[0][0], [na + 1, na + 2, na + 5]).any()  # the listed nodes are left out
    m.close()
    m2.close()
    # the command line
    sizes = [str(x) for x in np.bincount(labels0)]
    r = subprocess.run([cli, "-e", el, "-y", str(na), str(nb), "-z", "3", "3", "-n", *sizes, "-r", "-d", str(seed), "--rng", "philox",
                        "--chains", str(chains), "-b", str(10 * n), "-t", str(6 * n), "-f", str(2 * n), "--marginalize",
                        "--foldin", str(qin), str(qout), str(k), "--foldin_alpha", str(alpha)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert len(r.stdout.split()) == n  # (stdout: the marginal labels still)
    _write_foldin(want, nodes, rec, sim)
    assert qout.read_text() == want.read_text() and len(qout.read_text().splitlines()) == 2 * k * len(nodes)
