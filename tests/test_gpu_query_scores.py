"""GPU tests of the query scores (include/bisbm.h, "Query scores").  The model of the sums is distributed.numpy_pair_scores over
the enumerated (query, candidate) pairs, fed with what the handle's own getters return for every counted chain at every sample
and added ONE CHAIN AT A TIME onto a running total -- the order of the additions is part of the definition, so every row is
compared with `==`.  The model of the ranking is distributed.numpy_query_topk applied to the rows get_row returns.

The one comparison that is not bit for bit is against the device's own pair scores, which add the same non-negative terms in
another order: |a - b| <= terms 2^-52 b (the bound derived in test_gpu_pair_scores.py's docstring)."""
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
NA, NB = 903, 701  # neither candidate count is a multiple of 4, and the type-b candidates do not start on a label word


def _graph(isolated=2, seed=5):
    """about 9000 edges on 903 + 701 nodes; the last `isolated` nodes of each type have no edge"""
    rowptr, col = cases.random_graph(seed, NA, NB, 9000, 4, 4, 0, isolated)
    return rowptr, col, np.diff(rowptr.astype(np.int64))


def _model(rowptr, col, na, nb, ka, kb, chains, seed=9, **kw):
    return B.BlockModel(O.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rowptr, col),
                        n_chains=chains, seed=seed, **kw)


def _query_pairs(queries, na, nb):
    """the enumerated pairs (type-a node, type-b node) of every query, candidates in id order, and each row's slice"""
    pairs, rows, at = [], [], 0
    for q in queries:
        if q < na:
            pairs.append(np.stack([np.full(nb, q), na + np.arange(nb)], axis=1))
        else:
            pairs.append(np.stack([np.arange(na), np.full(na, q)], axis=1))
        rows.append(slice(at, at + len(pairs[-1])))
        at += len(pairs[-1])
    return np.concatenate(pairs).astype(np.int64), rows


def _add_chains(total, m, deg, pairs, chains):
    """the given chains' terms added onto `total` one chain at a time, in the given order"""
    for c in chains:
        total += D.numpy_pair_scores([m.get_memberships(c)], [m.get_m(c)], [m.get_m_r(c)], deg, pairs)
    return total


def _rows(m, n_queries):
    got = [m.query_scores(i) for i in range(n_queries)]
    assert len({t for _, t in got}) == 1
    return [r for r, _ in got], got[0][1]


def _mixed_queries(deg):
    """11 queries: both types mixed, one repeated, one isolated node of each type"""
    assert deg[NA - 1] == 0 and deg[NA + NB - 1] == 0 and (deg[:NA - 2] > 0).all() and (deg[NA:NA + NB - 2] > 0).all()
    q = np.array([0, NA + 5, 17, NA - 1, NA + NB - 1, 450, NA + 300, 17, NA + 700 - 2, 902 - 2, NA])
    assert len(q) == 11 and (q < NA).any() and (q >= NA).any()
    return q


def _neighbours(rowptr, col, q):
    return np.unique(col[int(rowptr[q]):int(rowptr[q + 1])].astype(np.int64))


def _check_topk(m, rowptr, col, na, nb, queries, rows, ks=(1, 10, 64)):
    """topk == numpy_query_topk of get_row's rows, integers and bits; returns the queries whose k-th and (k+1)-th eligible
    scores tie at a positive value, per (k, exclusion)"""
    tied = {}
    for k in ks:
        for excl in (False, True):
            nodes, sums, terms = m.query_topk(k, exclude_edges=excl)
            assert nodes.shape == sums.shape == (len(queries), k) and terms == m.query_scores(0)[1]
            for i, q in enumerate(queries):
                first = na if q < na else 0
                nbrs = _neighbours(rowptr, col, q) - first if excl else np.zeros(0, dtype=np.int64)
                idx, val = D.numpy_query_topk(rows[i], k, nbrs)
                want = np.where(idx == NONE, NONE, idx.astype(np.int64) + first).astype(np.uint32)
                assert (nodes[i] == want).all(), (k, excl, i, nodes[i], want)
                assert (sums[i].view(np.uint64) == val.view(np.uint64)).all(), (k, excl, i)
                if excl:
                    assert not np.isin(nodes[i].astype(np.int64), nbrs + first).any()
                more, _ = D.numpy_query_topk(rows[i], k + 1, nbrs)
                if more[k] != NONE and rows[i][more[k]] == rows[i][more[k - 1]] > 0:
                    tied.setdefault((k, excl), []).append(i)
    return tied


@pytest.mark.parametrize("ka,kb", [(4, 4), (8, 8), (32, 32), (64, 64), (6, 5)])
def test_one_chain_one_sample_is_the_model_bit_for_bit(ka, kb):
    rowptr, col, deg = _graph()
    queries = _mixed_queries(deg)
    pairs, rs = _query_pairs(queries, NA, NB)
    m = _model(rowptr, col, NA, NB, ka, kb, 1)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    m.query_scores_set(queries)
    m.query_scores_accumulate()
    rows, terms = _rows(m, len(queries))
    ref = _add_chains(np.zeros(len(pairs)), m, deg, pairs, [0])
    assert terms == 1
    for i, q in enumerate(queries):
        assert rows[i].shape == ((NB,) if q < NA else (NA,))
        assert (rows[i] == ref[rs[i]]).all(), (i, np.abs(rows[i] - ref[rs[i]]).max())
    assert (rows[2] == rows[7]).all() and rows[2].max() > 0            # the repeated query
    assert (rows[3] == 0).all() and (rows[4] == 0).all()               # the isolated queries
    assert (rows[0][NB - 2:] == 0).all() and (rows[1][NA - 2:] == 0).all() and rows[0][:NB - 2].min() >= 0  # isolated candidates
    m.close()


@pytest.mark.parametrize("type_b", [False, True])
def test_tile_boundaries(type_b):
    """two full candidate tiles plus a remainder that is no multiple of 4, two full query tiles plus one query"""
    n_cand, n_own, Q = 2 * B.QUERY_CAND_TILE + 3, 300, 2 * B.QUERY_TILE + 1
    assert (n_cand, Q) == (2051, 17)
    na, nb = (n_cand, n_own) if type_b else (n_own, n_cand)
    a, b = syn.planted_edges(na, nb, 9000, 4, 4, seed=6)
    rowptr, col = B.edge_to_adj((a, b), na + nb)
    deg = np.diff(rowptr.astype(np.int64))
    queries = (na if type_b else 0) + np.arange(Q) * 13
    pairs, rs = _query_pairs(queries, na, nb)
    m = _model(rowptr, col, na, nb, 4, 4, 1)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    m.query_scores_set(queries)
    m.query_scores_accumulate()
    rows, terms = _rows(m, Q)
    ref = _add_chains(np.zeros(len(pairs)), m, deg, pairs, [0])
    for i in range(Q):
        assert len(rows[i]) == n_cand and (rows[i] == ref[rs[i]]).all(), i
    assert min(r.max() for r in rows) > 0 and rows[Q - 1][n_cand - 3:].max() >= 0
    m.close()


def test_largest_byte_label_shape():
    """128 + 128 blocks: the staged rows of m at their widest"""
    na = nb = 1500
    rowptr, col = cases.random_graph(17, na, nb, 20000, 128, 128)
    deg = np.diff(rowptr.astype(np.int64))
    queries = np.array([0, na, 700, na + 1499, 1499, na + 3, 64, na + 640, 64])
    pairs, rs = _query_pairs(queries, na, nb)
    m = _model(rowptr, col, na, nb, 128, 128, 1, seed=21)
    m.shuffle_bisbm()
    m.run_sweeps(1)
    m.query_scores_set(queries)
    m.query_scores_accumulate()
    rows, terms = _rows(m, len(queries))
    ref = _add_chains(np.zeros(len(pairs)), m, deg, pairs, [0])
    assert terms == 1 and all((rows[i] == ref[rs[i]]).all() for i in range(len(queries)))
    assert sum(r.max() > 0 for r in rows) >= 7
    m.close()


def test_sixteen_chains_five_samples():
    chains = 16
    rowptr, col, deg = _graph()
    queries = _mixed_queries(deg)
    pairs, rs = _query_pairs(queries, NA, NB)
    m = _model(rowptr, col, NA, NB, 8, 8, chains)
    m.shuffle_bisbm()
    m.query_scores_set(queries)
    m.pair_scores_set(pairs)
    ref = np.zeros(len(pairs))
    for _ in range(5):
        m.run_sweeps(3)
        _add_chains(ref, m, deg, pairs, range(chains))
        m.query_scores_accumulate()
        m.pair_scores_accumulate()
    rows, terms = _rows(m, len(queries))
    assert terms == 80
    for i in range(len(queries)):
        assert (rows[i] == ref[rs[i]]).all(), i
    listed, listed_terms = m.pair_scores()
    got = np.concatenate(rows)
    assert listed_terms == 80
    assert (np.abs(got - listed) <= terms * EPS * listed).all(), (np.abs(got - listed) / np.maximum(listed, 1e-300)).max() / EPS
    # reset zeroes and keeps the queries
    m.query_scores_reset()
    rows0, t0 = _rows(m, len(queries))
    assert t0 == 0 and all((r == 0).all() for r in rows0)
    m.query_scores_accumulate()
    rows1, t1 = _rows(m, len(queries))
    one = _add_chains(np.zeros(len(pairs)), m, deg, pairs, range(chains))
    assert t1 == chains and all((rows1[i] == one[rs[i]]).all() for i in range(len(queries)))
    # set again replaces and zeroes
    m.query_scores_set(queries[:3][::-1])
    rows2, t2 = _rows(m, 3)
    assert t2 == 0 and [len(r) for r in rows2] == [NB, NA, NB] and all((r == 0).all() for r in rows2)
    with pytest.raises(IndexError):
        m.query_scores(3)
    m.query_scores_accumulate()
    assert (m.query_scores(2)[0] == one[rs[0]]).all()
    # set(0) frees everything
    m.query_scores_set(np.zeros(0, dtype=np.int64))
    with pytest.raises(B.BisbmError) as e:
        m.query_scores_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "queries" in str(e.value)
    m.close()


def test_row_sum_rule():
    """Over all candidates one chain's terms add up to d(q): sum_v d_q d_v m[b_q][b_v] / (m_r[b_q] m_r[b_v]) = d_q.  Every term
    carries at most two roundings, a cell's sum over `terms` chains terms - 1 more, numpy's sum over the n_other cells
    n_other - 1 more, all non-negative: within (terms + n_other + 1) 2^-52 of d(q) terms."""
    rowptr, col, na, nb = O.load_graph("southernWomen")
    deg = np.diff(rowptr.astype(np.int64))
    chains = 8
    m = B.BlockModel(O.contiguous_labels(na, nb, 3, 3), syn.types_vector(na, nb), 6, 3, 3, 0.001, (rowptr, col), n_chains=chains, seed=5)
    m.shuffle_bisbm()
    m.query_scores_set(np.arange(na + nb))
    for sample in range(1, 4):
        m.run_sweeps(2)
        m.query_scores_accumulate()
    rows, terms = _rows(m, na + nb)
    assert terms == 3 * chains
    for q in range(na + nb):
        n_other = nb if q < na else na
        want = float(deg[q]) * terms
        assert len(rows[q]) == n_other and abs(rows[q].sum() - want) <= (terms + n_other + 1) * EPS * want, (q, rows[q].sum(), want)
    # k = 14 with the neighbours left out: a type-a query keeps 14 - (its distinct neighbours) entries
    nodes, sums, _ = m.query_topk(14, exclude_edges=True)
    for q in range(na):
        real = nb - len(_neighbours(rowptr, col, q))
        assert (nodes[q, :real] != NONE).all() and (nodes[q, real:] == NONE).all() and (sums[q, real:] == 0).all(), q
        assert 0 < real < 14
    m.close()


@pytest.mark.parametrize("chains,samples", [(1, 1), (16, 3)])
def test_topk_is_the_host_ranking_of_the_rows(chains, samples):
    rowptr, col, deg = _graph()
    queries = _mixed_queries(deg)
    m = _model(rowptr, col, NA, NB, 4, 4, chains)
    m.shuffle_bisbm()
    m.query_scores_set(queries)
    with pytest.raises(B.BisbmError) as e:  # before any sample
        m.query_topk(5)
    assert e.value.code == B.BISBM_ERR_STATE and "sample" in str(e.value)
    for _ in range(samples):
        m.run_sweeps(3)
        m.query_scores_accumulate()
    rows, terms = _rows(m, len(queries))
    assert terms == chains * samples
    tied = _check_topk(m, rowptr, col, NA, NB, queries, rows)
    # the tie rule is exercised: some query's k-th and (k + 1)-th eligible scores are equal and positive (equal-degree nodes of
    # one block tie exactly with one chain) -- and the isolated queries tie at 0.0 throughout
    if chains == 1:
        assert tied, "no query has a tie at the k-th place: the tie rule goes untested"
    nodes, sums, _ = m.query_topk(10, exclude_edges=False)
    assert (nodes[3] == NA + np.arange(10)).all() and (sums[3] == 0).all()  # isolated type-a query: all 0.0, by id
    assert (nodes[4] == np.arange(10)).all()
    with pytest.raises(B.BisbmError) as e:
        m.query_topk(0)
    assert e.value.code == B.BISBM_ERR_INVALID_ARG
    with pytest.raises(B.BisbmError) as e:
        m.query_topk(B.QUERY_MAX_K + 1)
    assert e.value.code == B.BISBM_ERR_UNSUPPORTED and str(B.QUERY_MAX_K) in str(e.value)
    # the largest k: more than the 701 / 903 candidates, so every row is ranked in full and padded
    nodes, sums, _ = m.query_topk(B.QUERY_MAX_K, exclude_edges=False)
    for i, q in enumerate(queries):
        idx, val = D.numpy_query_topk(rows[i], B.QUERY_MAX_K)
        want = np.where(idx == NONE, NONE, idx.astype(np.int64) + (NA if q < NA else 0)).astype(np.uint32)
        assert (nodes[i] == want).all() and (sums[i].view(np.uint64) == val.view(np.uint64)).all(), i
    m.close()


def test_topk_leaves_a_multi_edge_neighbour_out_once():
    rowptr, col, deg = _graph()
    q = 17
    v = int(col[int(rowptr[q])])
    a = np.repeat(np.arange(NA), np.diff(rowptr.astype(np.int64))[:NA]).astype(np.uint64)
    b = col[:int(rowptr[NA])].astype(np.uint64)
    a, b = np.concatenate([a, [q, q]]).astype(np.uint64), np.concatenate([b, [v, v]]).astype(np.uint64)  # (q, v) three times
    rp2, cl2 = B.edge_to_adj((a, b), NA + NB)
    assert (cl2[int(rp2[q]):int(rp2[q + 1])] == v).sum() == 3
    m = _model(rp2, cl2, NA, NB, 4, 4, 1)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    queries = np.array([q, v])
    m.query_scores_set(queries)
    m.query_scores_accumulate()
    rows, _ = _rows(m, 2)
    k = 10
    nodes, sums, _ = m.query_topk(k, exclude_edges=True)
    assert v not in nodes[0] and q not in nodes[1] and (nodes != NONE).all()  # still k entries each
    with_edges, _, _ = m.query_topk(NB, exclude_edges=False)
    assert v in with_edges[0]
    _check_topk(m, rp2, cl2, NA, NB, queries, rows, ks=(k,))
    m.close()


def test_replica_exchange_counts_the_cold_chains():
    chains, ladder = 16, [1.0, 1.4, 2.0, 3.0]
    rowptr, col, deg = _graph()
    queries = _mixed_queries(deg)
    pairs, rs = _query_pairs(queries, NA, NB)
    m = _model(rowptr, col, NA, NB, 5, 5, chains)
    m.shuffle_bisbm()
    m.set_tempering(ladder)
    m.tempering_run(2, 1)
    m.query_scores_set(queries)
    ref = np.zeros(len(pairs))
    for sample in range(1, 3):
        m.tempering_run(3, 1)
        cold = np.flatnonzero(m.tempering_state()[0] == 0)
        assert len(cold) == chains // len(ladder)
        _add_chains(ref, m, deg, pairs, cold)
        m.query_scores_accumulate()
        assert m.query_scores(0)[1] == 4 * sample
    rows, terms = _rows(m, len(queries))
    assert terms == 8 and all((rows[i] == ref[rs[i]]).all() for i in range(len(queries)))
    # marginalize(tempering=..., recommend=...) samples the same way
    m2 = _model(rowptr, col, NA, NB, 5, 5, chains)
    m2.shuffle_bisbm()
    labels, counts, (nodes, scores, terms2) = B.marginalize(m2, 2, 2, 3, tempering=ladder, recommend=(queries, 7))
    rows2, t2 = _rows(m2, len(queries))
    assert t2 == terms2 == 8 and all((rows2[i] == rows[i]).all() for i in range(len(queries)))
    want_nodes, want_sums, _ = m.query_topk(7, exclude_edges=True)
    assert (nodes == want_nodes).all() and (scores == want_sums / 8).all() and len(labels) == NA + NB
    m.close()
    m2.close()


def test_chains_grouped_by_shape_are_added_group_by_group():
    g, deg, na, nb = _mixed_shapes_model()
    queries = np.array([3, na + 3, 499, na + 499, 250])
    pairs, rs = _query_pairs(queries, na, nb)
    g.query_scores_set(queries)
    g.query_scores_accumulate()  # one shape still
    ref = _add_chains(np.zeros(len(pairs)), g, deg, pairs, range(g.n_chains))
    assert not g.mixed_shapes
    _merge_until_mixed(g)
    shapes = [g.ka_kb(c) for c in range(g.n_chains)]
    order = sorted(range(g.n_chains), key=lambda c: (shapes.index(shapes[c]), c))  # groups in order of first appearance
    assert len(set(shapes)) >= 2 and order != list(range(g.n_chains))
    rows, terms = _rows(g, len(queries))  # the sums survive the merge
    assert terms == 32 and all((rows[i] == ref[rs[i]]).all() for i in range(len(queries)))
    g.run_sweeps(1)
    _add_chains(ref, g, deg, pairs, order)
    g.query_scores_accumulate()
    rows, terms = _rows(g, len(queries))
    assert terms == 64 and all((rows[i] == ref[rs[i]]).all() for i in range(len(queries)))
    g.close()
    # replica exchange over chains grouped by shape is refused
    g, deg, na, nb = _mixed_shapes_model()
    g.set_tempering([1.0, 1.3, 2.0, 3.5])
    g.query_scores_set(queries)
    _merge_until_mixed(g)
    with pytest.raises(B.BisbmError) as e:
        g.query_scores_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "grouped by shape" in str(e.value)
    g.close()


def test_a_device_listed_twice():
    chains = 16
    rowptr, col, deg = _graph()
    queries = _mixed_queries(deg)
    pairs, rs = _query_pairs(queries, NA, NB)
    m = _model(rowptr, col, NA, NB, 5, 6, chains, devices=[0, 0])
    m.shuffle_bisbm()
    m.query_scores_set(queries)
    dev = [np.zeros(len(pairs)), np.zeros(len(pairs))]
    for _ in range(2):
        m.run_sweeps(2)
        _add_chains(dev[0], m, deg, pairs, range(0, chains // 2))
        _add_chains(dev[1], m, deg, pairs, range(chains // 2, chains))
        m.query_scores_accumulate()
    rows, terms = _rows(m, len(queries))
    ref = dev[0] + dev[1]
    assert terms == 2 * chains and all((rows[i] == ref[rs[i]]).all() for i in range(len(queries)))
    _check_topk(m, rowptr, col, NA, NB, queries, rows, ks=(10,))
    m.query_scores_reset()
    rows0, t0 = _rows(m, len(queries))
    assert t0 == 0 and all((r == 0).all() for r in rows0)
    m.close()


def test_refusals():
    # a wide handle (two-byte labels): the pair scores serve it
    name, na, nb, ne, ka, kb, eps, hubs, isolated = cases.CASE["wide_labels"]
    rowptr, col = cases.random_graph(5, na, nb, ne, ka, kb, hubs, isolated)
    w = _model(rowptr, col, na, nb, ka, kb, 1, seed=2)
    w.query_scores_set([0, na])
    with pytest.raises(B.BisbmError) as e:  # before init
        w.query_scores_accumulate()
    assert e.value.code in (B.BISBM_ERR_STATE, B.BISBM_ERR_UNSUPPORTED)
    w.shuffle_bisbm()
    with pytest.raises(B.BisbmError) as e:
        w.query_scores_accumulate()
    assert e.value.code == B.BISBM_ERR_UNSUPPORTED and "bisbm_pair_scores" in str(e.value)
    w.close()
    m, deg = _planted(300, 200, 3000, 4, 4, 4)
    with pytest.raises(B.BisbmError) as e:  # no queries
        m.query_scores_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "queries" in str(e.value)
    m.query_scores_set([1, 499, 300])
    with pytest.raises(B.BisbmError) as e:  # no block state yet
        m.query_scores_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "bisbm_init" in str(e.value)
    m.init_bisbm()
    m.query_scores_accumulate()
    rows, terms = _rows(m, 3)
    for bad, index in (([0, 500], 1), ([500], 0), ([3, 4, 4000000000], 2)):
        with pytest.raises(B.BisbmError) as e:
            m.query_scores_set(np.array(bad))
        assert e.value.code == B.BISBM_ERR_INVALID_ARG and ("query %d " % index) in str(e.value), str(e.value)
        rows2, t2 = _rows(m, 3)  # the earlier queries and their sums are intact
        assert t2 == terms == 4 and all((rows2[i] == rows[i]).all() for i in range(3))
    with pytest.raises(ValueError):
        m.query_scores_set(np.zeros((3, 2), dtype=np.int64))
    m.close()
    # the mt19937-compat mode is served (the calls only read state)
    c, deg = _planted(500, 400, 5000, 6, 5, 1, rng="mt19937-compat", gen_seed=10)
    c.shuffle_bisbm()
    c.run_sweeps(2)
    queries = np.array([7, 500 + 7, 499])
    pairs, rs = _query_pairs(queries, 500, 400)
    c.query_scores_set(queries)
    c.query_scores_accumulate()
    rows, terms = _rows(c, 3)
    ref = _add_chains(np.zeros(len(pairs)), c, deg, pairs, [0])
    assert terms == 1 and all((rows[i] == ref[rs[i]]).all() for i in range(3))
    c.close()


def test_same_calls_same_bits():
    rowptr, col, deg = _graph()
    queries = _mixed_queries(deg)
    out = []
    for _ in range(2):
        m = _model(rowptr, col, NA, NB, 8, 8, 16)
        m.shuffle_bisbm()
        m.query_scores_set(queries)
        for _ in range(3):
            m.run_sweeps(2)
            m.query_scores_accumulate()
        rows, terms = _rows(m, len(queries))
        out.append((np.concatenate(rows).view(np.uint64), terms, m.query_topk(20)))
        m.close()
    assert out[0][1] == out[1][1] == 48 and (out[0][0] == out[1][0]).all()
    assert (out[0][2][0] == out[1][2][0]).all() and (out[0][2][1].view(np.uint64) == out[1][2][1].view(np.uint64)).all()


def _write_recommendations(path, queries, nodes, scores):
    with open(path, "w") as f:
        for i, q in enumerate(queries):
            for node, s in zip(nodes[i], scores[i]):
                if node != NONE:
                    f.write("%d %d %s\n" % (q, node, "%.17g" % s))


def test_cli_reproduces_the_python_path(tmp_path):
    rowptr, col, na, nb = O.load_graph("n_1000")
    n, chains, seed, k = na + nb, 8, 5, 12
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    queries = np.array([0, 731, 499, 500, 17, 999, 17])
    qin, qout, want = tmp_path / "queries.txt", tmp_path / "out.txt", tmp_path / "want.txt"
    qin.write_text("".join("%d\n" % q for q in queries))
    sizes = [str(x) for x in np.bincount(O.contiguous_labels(na, nb, 4, 4))]
    common = [cli, "-e", el, "-y", str(na), str(nb), "-z", "4", "4", "-n", *sizes, "-r", "-d", str(seed), "--rng", "philox", "--chains", str(chains),
              "-b", str(10 * n), "-t", str(6 * n), "-f", str(2 * n), "--marginalize"]
    r = subprocess.run(common + ["--recommend", str(qin), str(qout), str(k)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    m = B.BlockModel(O.contiguous_labels(na, nb, 4, 4), syn.types_vector(na, nb), 8, 4, 4, 1.0, (rowptr, col), n_chains=chains, seed=seed)
    m.shuffle_bisbm()
    labels, _, (nodes, scores, terms) = B.marginalize(m, 10, 3, 2, recommend=(queries, k))
    assert terms == 3 * chains and len(r.stdout.split()) == n == len(labels)  # (stdout: the marginal labels still)
    _write_recommendations(want, queries, nodes, scores)
    assert qout.read_text() == want.read_text() and len(qout.read_text().splitlines()) == len(queries) * k
    # --include_edges
    r = subprocess.run(common + ["--recommend", str(qin), str(qout), str(k), "--include_edges"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    nodes, scores, _ = m.recommend(k, exclude_edges=False)
    _write_recommendations(want, queries, nodes, scores)
    assert qout.read_text() == want.read_text()
    m.close()
    # --reorder: queries and candidates are given and printed in the file's own ids; the engine ranks the renumbered nodes
    r = subprocess.run(common + ["--reorder", "--recommend", str(qin), str(qout), str(k)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lo = B.locality_order(rowptr, col, na, nb)
    rp2, cl2 = lo.apply(rowptr, col)
    m = B.BlockModel(lo.to_new(O.contiguous_labels(na, nb, 4, 4)), syn.types_vector(na, nb), 8, 4, 4, 1.0, (rp2, cl2), n_chains=chains, seed=seed)
    m.shuffle_bisbm()
    _, _, (nodes, scores, _) = B.marginalize(m, 10, 3, 2, recommend=(lo.new_id[queries], k))
    old = np.argsort(lo.new_id)
    _write_recommendations(want, queries, np.where(nodes == NONE, NONE, old[np.minimum(nodes, n - 1)]), scores)
    assert qout.read_text() == want.read_text()
    m.close()


def test_example_runs():
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "recommend.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "held-out edges in the top" in r.stdout, r.stdout + r.stderr
