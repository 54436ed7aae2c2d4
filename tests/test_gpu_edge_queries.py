"""GPU tests of the edge queries (include/bisbm.h, "Edge queries").  Two models of one chain's rows, both fed with what the
handle's own getters return (block state with eta), the device's log_q (debug_log_q, fast=False), the C library's lgamma (the
values the engine's table holds) and, for w, the device's exp (debug_exp): on the small graph a loop of distributed.numpy_edge_dS
over the enumerated pairs -- the model of the listed call --, on the larger shapes distributed.numpy_edge_query_rows, which
tests/test_edge_queries.py pins to that loop bit for bit.  The chains are folded onto the running sums one at a time in the
stated order, so every row is compared on its bit patterns.  The model of the ranking is distributed.numpy_query_topk applied to
the rows get_row returns."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_edge_probs import KA, KB, NA, NB
from test_gpu_edge_probs import LG, _snapshot, chain_dS, same, small_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


def query_pairs(queries, na, nb):
    """the enumerated pairs (type-a node, type-b node) of every query, candidates in id order, and each row's slice"""
    pairs, rows, at = [], [], 0
    for q in np.asarray(queries).tolist():
        if q < na:
            pairs.append(np.stack([np.full(nb, q), na + np.arange(nb)], axis=1))
        else:
            pairs.append(np.stack([np.arange(na), np.full(na, q)], axis=1))
        rows.append(slice(at, at + len(pairs[-1])))
        at += len(pairs[-1])
    return np.concatenate(pairs).astype(np.int64), rows


def chain_rows(m, c, queries, mult, deg, na):
    """numpy_edge_query_rows of chain c of the handle, from the handle's getters and probes"""
    ka, kb = m.ka_kb(c)
    lab = m.get_memberships(c)
    M, mr, nr, eta = m._block_state(c, ("m", "m_r", "n_r", "eta"))
    ks, ns = np.concatenate([mr, mr + 1]), np.tile(nr, 2)
    table = dict(zip(zip(ks.tolist(), ns.tolist()), m.debug_log_q(ks, ns, fast=False).tolist()))
    return D.numpy_edge_query_rows(M, mr, nr, eta, deg, lab, na, ka, kb, m.num_edges, queries, mult, LG, lambda k, n: table[(k, n)])


def fold(m, w_rows, dS_rows):
    """one chain onto the running sums: one f64 add per cell, w with the device's exp"""
    for w, dS in zip(w_rows, dS_rows):
        w += np.where(dS > 700.0, 0.0, m.debug_exp(-dS))


def model_sample(m, w_rows, queries, mult, deg, na, chains=None):
    for c in (range(m.n_chains) if chains is None else chains):
        fold(m, w_rows, chain_rows(m, c, queries, mult, deg, na))


def zeros_like_rows(mult):
    return [np.zeros(len(r)) for r in mult]


def got_rows(m, n_queries):
    got = [m.edge_queries(i) for i in range(n_queries)]
    assert len({g["terms"] for g in got}) == 1
    return got, got[0]["terms"]


def assert_rows(m, n_queries, want, terms, mult=None):
    got, t = got_rows(m, n_queries)
    assert t == terms
    for i in range(n_queries):
        assert got[i]["w_sum"].shape == want[i].shape and same(got[i]["w_sum"], want[i]), (i, got[i]["w_sum"], want[i])
        if mult is not None:
            assert (got[i]["mult"] == mult[i]).all(), i
    return got


def planted(na, nb, edges, ka, kb, chains, seed=9, graph_seed=6, **kw):
    a, b = syn.planted_edges(na, nb, edges, ka, kb, seed=graph_seed)
    rowptr, col = B.edge_to_adj((a, b), na + nb)
    m = B.BlockModel(O.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rowptr, col), n_chains=chains, seed=seed, **kw)
    return m, rowptr, col, np.diff(rowptr.astype(np.int64))


def test_small_graph_every_row_is_the_listed_model_and_the_listed_call_bit_for_bit():
    """5 chains, two samples with a sweep between; the first sample is taken on the planted labels, where the isolated nodes sit
    alone in their blocks (m_r = 0).  All 27 nodes are queries, node 3 twice."""
    chains, n = 5, NA + NB
    m, a, b, labels, rowptr, col = small_model(chains)
    deg = np.diff(rowptr.astype(np.int64))
    queries = np.concatenate([np.arange(n), [3]])
    pairs, rs = query_pairs(queries, NA, NB)
    kinds = np.zeros(len(pairs), dtype=np.uint8)
    mult = D.numpy_edge_multiplicity(rowptr, col, pairs)
    mult_rows = D.numpy_edge_query_mult(rowptr, col, NA, queries)
    assert all((mult_rows[i] == mult[rs[i]]).all() for i in range(len(queries)))
    # what the rows cover, from the data
    assert {0, 1, 2} <= set(mult.tolist()) and (mult >= 2).sum() >= 2 * 4  # (four doubled edges, seen from both ends)
    assert deg[14] == 0 and deg[26] == 0  # a query and a candidate of degree 0, of either type
    top = int(np.argmax(deg))
    assert deg[top] == m.max_degree  # d + 1 of this query lies beyond the eta table
    m.init_bisbm()
    m.edge_queries_set(queries)
    m.edge_probs_set(pairs, kinds)
    w_loop, w_rows = np.zeros(len(pairs)), zeros_like_rows(mult_rows)
    for sample in (1, 2):
        if sample == 1:
            assert all(m.get_m_r(c)[2] == 0 and m.get_m_r(c)[KA + KB - 1] == 0 for c in range(chains))  # blocks with m_r = 0
            assert m.get_eta_rk_(0).shape[1] == m.max_degree + 1
        for c in range(chains):
            dS = chain_dS(m, c, pairs, kinds, mult, deg)
            w_loop += np.where(dS > 700.0, 0.0, m.debug_exp(-dS))
        model_sample(m, w_rows, queries, mult_rows, deg, NA)
        m.edge_queries_accumulate()
        m.edge_probs_accumulate()
        listed = m.edge_probs()
        assert listed["terms"] == sample * chains and same(listed["w_sum"], w_loop)
        got = assert_rows(m, len(queries), [w_loop[r] for r in rs], sample * chains, mult_rows)
        for i in range(len(queries)):
            assert same(got[i]["w_sum"], listed["w_sum"][rs[i]]) and same(got[i]["w_sum"], w_rows[i]), i
            assert np.isfinite(got[i]["log_prob"]).all()
            assert same(got[i]["log_prob"], listed["log_prob"][rs[i]])
        assert same(got[3]["w_sum"], got[n]["w_sum"])  # the repeated query
        m.run_sweeps(1)
    assert len({tuple(m.get_memberships(c)) for c in range(chains)}) > 1  # (the chains differ)
    m.edge_queries_reset()
    got, t = got_rows(m, len(queries))
    assert t == 0 and all((g["w_sum"] == 0).all() and np.isnan(g["log_prob"]).all() for g in got)
    m.close()


@pytest.mark.parametrize("type_b", [False, True])
def test_tile_boundaries_and_two_ranges_of_chains(type_b, monkeypatch):
    """two full candidate tiles plus a remainder that is no multiple of 4, two full query tiles plus one query; three chains in one
    launch, then in two (BISBM_EDGE_RANGE_CHAINS=2): the same bits"""
    n_cand, n_own, Q, chains = 2 * B.EDGE_QUERY_CAND_TILE + 3, 300, 2 * B.EDGE_QUERY_TILE + 1, 3
    assert (n_cand, Q) == (2051, 17)
    na, nb = (n_cand, n_own) if type_b else (n_own, n_cand)
    assert n_cand % 4 == 3
    m, rowptr, col, deg = planted(na, nb, 9000, 4, 4, chains)
    queries = (na if type_b else 0) + np.arange(Q) * 13
    mult = D.numpy_edge_query_mult(rowptr, col, na, queries)
    assert sum(int((r > 0).sum()) for r in mult) > 100 and len(mult[0]) == n_cand
    m.shuffle_bisbm()
    m.run_sweeps(2)
    m.edge_queries_set(queries)
    want = zeros_like_rows(mult)
    model_sample(m, want, queries, mult, deg, na)
    m.edge_queries_accumulate()
    one = assert_rows(m, Q, want, chains, mult)
    monkeypatch.setenv("BISBM_EDGE_RANGE_CHAINS", "2")
    m.edge_queries_reset()
    m.edge_queries_accumulate()
    two = assert_rows(m, Q, want, chains, mult)
    assert all(same(x["w_sum"], y["w_sum"]) for x, y in zip(one, two))
    assert min(g["w_sum"].max() for g in one) > 0
    m.close()


@pytest.mark.parametrize("na,nb,ka,kb", [(400, 400, 128, 128), (500, 300, 200, 56)])
def test_the_widest_rows_of_either_type(na, nb, ka, kb):
    """256 blocks: the LDS budget at its largest, and the two query types' rows of different lengths"""
    rowptr, col = cases.random_graph(17, na, nb, 6000, ka, kb)
    deg = np.diff(rowptr.astype(np.int64))
    m = B.BlockModel(O.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rowptr, col), n_chains=1, seed=21)
    m.shuffle_bisbm()
    m.run_sweeps(1)
    queries = np.array([0, na, na - 1, na + nb - 1, 64, na + 3, 64, na + 200, 199, 5])
    mult = D.numpy_edge_query_mult(rowptr, col, na, queries)
    m.edge_queries_set(queries)
    want = zeros_like_rows(mult)
    model_sample(m, want, queries, mult, deg, na)
    m.edge_queries_accumulate()
    assert_rows(m, len(queries), want, 1, mult)
    labels = m.get_memberships(0)
    assert len(set(labels[:na].tolist())) > 64 and len(set(labels[na:].tolist())) > 40  # (many blocks of either type are in use)
    m.close()


def test_sixteen_chains_three_samples():
    chains = 16
    m, rowptr, col, deg = planted(903, 701, 9000, 8, 8, chains)
    na = 903
    queries = np.array([0, na + 5, 17, 450, na + 300, 17, na + 700, 902, na])
    mult = D.numpy_edge_query_mult(rowptr, col, na, queries)
    m.shuffle_bisbm()
    m.edge_queries_set(queries)
    want = zeros_like_rows(mult)
    for _ in range(3):
        m.run_sweeps(2)
        model_sample(m, want, queries, mult, deg, na)
        m.edge_queries_accumulate()
    assert_rows(m, len(queries), want, 48, mult)
    m.close()


def _neighbours(rowptr, col, q):
    return np.unique(col[int(rowptr[q]):int(rowptr[q + 1])].astype(np.int64))


def test_topk_is_the_host_ranking_of_the_rows_and_leaves_the_cells_alone():
    na, nb = 903, 701
    rowptr, col = cases.random_graph(5, na, nb, 9000, 4, 4, 0, 2)
    q = 17
    v = int(col[int(rowptr[q])])
    a = np.repeat(np.arange(na), np.diff(rowptr.astype(np.int64))[:na]).astype(np.uint64)
    b = col[:int(rowptr[na])].astype(np.uint64)
    a, b = np.concatenate([a, [q]]).astype(np.uint64), np.concatenate([b, [v]]).astype(np.uint64)  # (q, v) twice
    rowptr, col = B.edge_to_adj((a, b), na + nb)
    assert (col[int(rowptr[q]):int(rowptr[q + 1])] == v).sum() == 2
    queries = np.array([q, v, 0, na + 5, na - 1, na + nb - 1, 450])
    models = []
    for _ in range(2):
        m = B.BlockModel(O.contiguous_labels(na, nb, 4, 4), syn.types_vector(na, nb), 8, 4, 4, 1.0, (rowptr, col), n_chains=1, seed=9)
        m.shuffle_bisbm()
        m.run_sweeps(3)
        m.edge_queries_set(queries)
        models.append(m)
    m, plain = models
    with pytest.raises(B.BisbmError) as e:  # before any sample
        m.edge_queries_topk(5)
    assert e.value.code == B.BISBM_ERR_STATE and "sample" in str(e.value)
    m.edge_queries_accumulate()
    got, terms = got_rows(m, len(queries))
    rows = [g["w_sum"] for g in got]
    assert terms == 1 and got[0]["mult"][v - na] == 2 and got[1]["mult"][q] == 2
    tied = []
    for k in (1, 256, 257, 1024):
        for excl in (False, True):
            nodes, sums, t = m.edge_queries_topk(k, exclude_edges=excl)
            assert nodes.shape == sums.shape == (len(queries), k) and t == 1
            for i, qi in enumerate(queries.tolist()):
                first = na if qi < na else 0
                nbrs = _neighbours(rowptr, col, qi) - first if excl else np.zeros(0, dtype=np.int64)
                idx, val = D.numpy_query_topk(rows[i], k, nbrs)
                want = np.where(idx == NONE, NONE, idx.astype(np.int64) + first).astype(np.uint32)
                assert (nodes[i] == want).all(), (k, excl, i, nodes[i], want)
                assert same(sums[i], val), (k, excl, i)
                more, _ = D.numpy_query_topk(rows[i], k + 1, nbrs)
                if more[k] != NONE and rows[i][more[k]] == rows[i][more[k - 1]]:
                    tied.append((k, excl, i))
                if k == 1024:  # fewer eligible candidates than k
                    eligible = len(rows[i]) - len(nbrs)
                    assert (nodes[i, :eligible] != NONE).all() and (nodes[i, eligible:] == NONE).all() and (sums[i, eligible:] == 0).all()
            if excl:
                assert v not in nodes[0] and q not in nodes[1]  # the neighbour by two edges is left out, once
            elif k == 1024:
                assert v in nodes[0] and q in nodes[1]
    assert tied, "no query has a tie at the k-th place: the tie rule goes untested"
    nodes, sums, lp = m.recommend_edges(10)
    want_nodes, want_sums, _ = m.edge_queries_topk(10, exclude_edges=True)
    assert (nodes == want_nodes).all() and same(sums, want_sums) and same(lp, B.BlockModel._log_odds(want_sums, 1))
    for k, code in ((0, B.BISBM_ERR_INVALID_ARG), (B.QUERY_MAX_K + 1, B.BISBM_ERR_UNSUPPORTED)):
        with pytest.raises(B.BisbmError) as e:
            m.edge_queries_topk(k)
        assert e.value.code == code
    # accumulate after the selections: the cells are what a run without them holds
    plain.edge_queries_accumulate()
    for g in (m, plain):
        g.run_sweeps(1)
        g.edge_queries_accumulate()
    after, t2 = got_rows(m, len(queries))
    ref, t3 = got_rows(plain, len(queries))
    assert t2 == t3 == 2 and all(same(x["w_sum"], y["w_sum"]) for x, y in zip(after, ref))
    m.close()
    plain.close()


def test_replica_exchange_counts_rung_zero_only():
    chains, L = 6, 3
    m, a, b, labels, rowptr, col = small_model(chains)
    deg = np.diff(rowptr.astype(np.int64))
    queries = np.array([0, NA + 1, 14, 26, 7, NA + 4])
    mult = D.numpy_edge_query_mult(rowptr, col, NA, queries)
    m.shuffle_bisbm()
    m.set_tempering([1.0, 1.5, 2.5])
    m.edge_queries_set(queries)
    want = zeros_like_rows(mult)
    for sample in (1, 2):
        m.tempering_run(3, 1)
        cold = np.flatnonzero(m.tempering_state()[0] == 0)
        assert len(cold) == chains // L
        model_sample(m, want, queries, mult, deg, NA, cold.tolist())
        m.edge_queries_accumulate()
        assert_rows(m, len(queries), want, 2 * sample, mult)
    m.close()


def test_chains_grouped_by_shape_each_group_with_its_own_edge_prior():
    rowptr, col, na, nb = O.load_graph("n_1000")
    chains = 12
    deg = np.diff(rowptr.astype(np.int64))
    g = B.BlockModel(O.contiguous_labels(na, nb, 8, 9), syn.types_vector(na, nb), 17, 8, 9, 1.0, (rowptr, col), n_chains=chains, seed=123)
    g.shuffle_bisbm()
    g.run_sweeps(3)
    queries = np.array([3, na + 3, na - 1, na + nb - 1, 250])
    mult = D.numpy_edge_query_mult(rowptr, col, na, queries)
    g.edge_queries_set(queries)
    want = zeros_like_rows(mult)
    model_sample(g, want, queries, mult, deg, na)
    g.edge_queries_accumulate()  # one shape still
    g.agg_merge(5, None, 10)  # (the diverging one-argument merge of test_gpu_edge_probs.py)
    shapes = [g.ka_kb(c) for c in range(chains)]
    assert g.mixed_shapes and len(set(shapes)) > 1
    assert_rows(g, len(queries), want, chains, mult)  # sums and terms survive the merge
    g.run_sweeps(1)
    first = {s: shapes.index(s) for s in set(shapes)}
    order = sorted(range(chains), key=lambda c: (first[shapes[c]], c))  # the groups in order of first appearance, chains ascending
    model_sample(g, want, queries, mult, deg, na, order)
    g.edge_queries_accumulate()
    assert_rows(g, len(queries), want, 2 * chains, mult)
    g.close()
    # replica exchange over chains grouped by shape is refused
    g = B.BlockModel(O.contiguous_labels(na, nb, 8, 9), syn.types_vector(na, nb), 17, 8, 9, 1.0, (rowptr, col), n_chains=chains, seed=123)
    g.shuffle_bisbm()
    g.run_sweeps(3)
    g.set_tempering([1.0, 1.3, 2.0])
    g.edge_queries_set(queries)
    g.edge_queries_accumulate()
    g.agg_merge(5, None, 10)
    assert g.mixed_shapes
    with pytest.raises(B.BisbmError) as e:
        g.edge_queries_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "grouped by shape" in str(e.value)
    assert g.edge_queries(0)["terms"] == 4
    g.close()


def test_a_device_listed_twice_adds_the_entries_sums_in_entry_order():
    chains, n = 6, NA + NB
    m, a, b, labels, rowptr, col = small_model(chains, devices=[0, 0])
    deg = np.diff(rowptr.astype(np.int64))
    queries = np.arange(n)
    mult = D.numpy_edge_query_mult(rowptr, col, NA, queries)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    m.edge_queries_set(queries)
    first = m.device_layout()[1] + [chains]
    assert len(first) == 3
    parts = [zeros_like_rows(mult) for _ in range(2)]
    for sample in range(2):
        for k in range(2):
            model_sample(m, parts[k], queries, mult, deg, NA, range(first[k], first[k + 1]))
        m.edge_queries_accumulate()
        m.run_sweeps(1)
    rows = assert_rows(m, n, [(0.0 + x) + y for x, y in zip(*parts)], 2 * chains, mult)
    nodes, sums, terms = m.edge_queries_topk(5, exclude_edges=True)
    for i in range(n):
        first_cand = NA if i < NA else 0
        idx, val = D.numpy_query_topk(rows[i]["w_sum"], 5, _neighbours(rowptr, col, i) - first_cand)
        assert (nodes[i] == np.where(idx == NONE, NONE, idx.astype(np.int64) + first_cand)).all() and same(sums[i], val), i
    m.edge_queries_reset()
    got, t = got_rows(m, n)
    assert t == 0 and all((g["w_sum"] == 0).all() for g in got)
    m.close()


def test_compat_mode_and_a_clamp_change_no_bit():
    m, a, b, labels, rowptr, col = small_model(2, rng="mt19937-compat", gen_seed=9)
    deg = np.diff(rowptr.astype(np.int64))
    queries = np.arange(NA + NB)
    mult = D.numpy_edge_query_mult(rowptr, col, NA, queries)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    m.edge_queries_set(queries)
    want = zeros_like_rows(mult)
    model_sample(m, want, queries, mult, deg, NA)
    m.edge_queries_accumulate()
    assert_rows(m, len(queries), want, 2, mult)
    m.close()
    rows = []
    for clamp in (False, True):
        m = small_model(4)[0]
        m.shuffle_bisbm()
        m.run_sweeps(2)
        if clamp:
            m.clamp([0, 5, NA + 2])
        m.edge_queries_set(queries)
        m.edge_queries_accumulate()
        rows.append(got_rows(m, len(queries))[0])
        m.close()
    assert all(same(x["w_sum"], y["w_sum"]) for x, y in zip(*rows))
    assert_rows_equal_model = [r["w_sum"].max() > 0 for r in rows[0]]
    assert all(assert_rows_equal_model)


def test_state_is_only_read_and_the_same_calls_give_the_same_bits():
    queries = np.concatenate([np.arange(NA + NB), [3]])
    m, twin = small_model(4)[0], small_model(4)[0]
    for g in (m, twin):
        g.shuffle_bisbm()
        g.run_sweeps(2)
        g.edge_queries_set(queries)
    before = _snapshot(m)
    m.edge_queries_accumulate()
    m.edge_queries_topk(3)
    assert _snapshot(m) == before == _snapshot(twin)
    assert (m.run_sweeps(1) == twin.run_sweeps(1)).all() and _snapshot(m) == _snapshot(twin)  # the next sweep too
    twin.edge_queries_accumulate()  # (a sweep later than m's)
    twin.edge_queries_reset()
    m.edge_queries_reset()
    for g in (m, twin):
        g.edge_queries_accumulate()
    a, ta = got_rows(m, len(queries))
    b, tb = got_rows(twin, len(queries))
    assert ta == tb == 4 and all(same(x["w_sum"], y["w_sum"]) for x, y in zip(a, b))
    ka, kb_ = m.edge_queries_topk(4), twin.edge_queries_topk(4)
    assert (ka[0] == kb_[0]).all() and same(ka[1], kb_[1])
    m.close()
    twin.close()


def test_refusals():
    # a wide handle (two-byte labels): the listed call serves it
    name, na, nb, ne, ka, kb, eps, hubs, isolated = cases.CASE["wide_labels"]
    rowptr, col = cases.random_graph(5, na, nb, ne, ka, kb, hubs, isolated)
    w = B.BlockModel(O.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rowptr, col), n_chains=1, seed=2)
    w.edge_queries_set([0, na])
    w.shuffle_bisbm()
    with pytest.raises(B.BisbmError) as e:
        w.edge_queries_accumulate()
    assert e.value.code == B.BISBM_ERR_UNSUPPORTED and "bisbm_edge_probs" in str(e.value)
    w.close()
    m = small_model(4)[0]
    for call in (m.edge_queries_accumulate, lambda: m.edge_queries_topk(3), m.edge_queries_reset):
        if call == m.edge_queries_reset:
            call()  # (nothing to zero: fine)
            continue
        with pytest.raises(B.BisbmError) as e:  # no queries
            call()
        assert e.value.code == B.BISBM_ERR_STATE and "queries" in str(e.value)
    with pytest.raises(IndexError):
        m.edge_queries(0)
    m.edge_queries_set([1, NA + 3, 14])
    with pytest.raises(B.BisbmError) as e:  # no block state yet
        m.edge_queries_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "bisbm_init" in str(e.value)
    m.init_bisbm()
    m.edge_queries_accumulate()
    rows, terms = got_rows(m, 3)
    n = NA + NB
    for bad, index in (([0, n], 1), ([n], 0), ([3, 4, 4000000000], 2)):
        with pytest.raises(B.BisbmError) as e:
            m.edge_queries_set(np.array(bad))
        assert e.value.code == B.BISBM_ERR_INVALID_ARG and ("query %d " % index) in str(e.value), str(e.value)
        rows2, t2 = got_rows(m, 3)  # the earlier queries and their sums are intact
        assert t2 == terms == 4 and all(same(x["w_sum"], y["w_sum"]) and (x["mult"] == y["mult"]).all() for x, y in zip(rows, rows2))
    with pytest.raises(ValueError):
        m.edge_queries_set(np.zeros((3, 2), dtype=np.int64))
    # every pointer of get_row may be NULL
    assert m._L.bisbm_edge_queries_get_row(m._h, 0, None, None, None) == 0
    assert m._L.bisbm_edge_queries_get_row(m._h, 3, None, None, None) == B.BISBM_ERR_INVALID_ARG
    m.edge_queries_set(np.zeros(0, dtype=np.int64))  # frees everything
    with pytest.raises(B.BisbmError) as e:
        m.edge_queries_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE
    m.close()


def test_cli_lines_equal_the_python_driver(tmp_path):
    rowptr, col, na, nb = O.load_graph("n_1000")
    n, chains, seed, k = na + nb, 8, 5, 12
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    queries = np.array([0, 731, 499, 500, 17, 999, 17])
    qin, qout = tmp_path / "queries.txt", tmp_path / "out.txt"
    qin.write_text("".join("%d\n" % q for q in queries))
    sizes = [str(x) for x in np.bincount(O.contiguous_labels(na, nb, 4, 4))]
    common = [cli, "-e", el, "-y", str(na), str(nb), "-z", "4", "4", "-n", *sizes, "-r", "-d", str(seed), "--rng", "philox", "--chains", str(chains),
              "-b", str(10 * n), "-t", str(6 * n), "-f", str(2 * n), "--marginalize"]
    m = B.BlockModel(O.contiguous_labels(na, nb, 4, 4), syn.types_vector(na, nb), 8, 4, 4, 1.0, (rowptr, col), n_chains=chains, seed=seed)
    m.shuffle_bisbm()
    labels, _, (nodes, w_sum, log_prob) = B.marginalize(m, 10, 3, 2, recommend_edges=(queries, k))
    terms = m.edge_queries(0)["terms"]
    assert terms == 3 * chains and len(labels) == n

    def lines(nodes, w_sum, log_prob):
        return ["%d %d %.17g %.17g" % (q, node, w / terms, lp) for i, q in enumerate(queries.tolist())
                for node, w, lp in zip(nodes[i].tolist(), w_sum[i].tolist(), log_prob[i].tolist()) if node != NONE]
    r = subprocess.run(common + ["--recommend_edges", str(qin), str(qout), str(k)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert len(r.stdout.split()) == n  # (stdout: the marginal labels still)
    assert qout.read_text().splitlines() == lines(nodes, w_sum, log_prob) and len(qout.read_text().splitlines()) == len(queries) * k
    r = subprocess.run(common + ["--recommend_edges", str(qin), str(qout), str(k), "--include_edges"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert qout.read_text().splitlines() == lines(*m.recommend_edges(k, exclude_edges=False))
    m.close()


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "recommend_exact.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "held-out edges in the top" in r.stdout and "recommend_edges" in r.stdout, r.stdout + r.stderr
