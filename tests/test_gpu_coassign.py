"""GPU tests of the co-assignment calls (include/bisbm.h, "Co-assignment").  The model of the counts is
distributed.numpy_coassign fed with what get_memberships returns for every counted chain at every sample; every result is an
integer, so everything is compared with `==`.  The model of the ranking is distributed.numpy_query_topk applied to the rows
get_row returns, with the query's own node as the one excluded candidate."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_gpu_pair_scores import _merge_until_mixed, _mixed_shapes_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NA, NB = 903, 701  # neither count is a multiple of 4, and the type-b nodes do not start on a label word


def _graph(isolated=2, seed=5):
    """about 9000 edges on 903 + 701 nodes; the last `isolated` nodes of each type have no edge"""
    rowptr, col = cases.random_graph(seed, NA, NB, 9000, 4, 4, 0, isolated)
    return rowptr, col, np.diff(rowptr.astype(np.int64))


def _model(rowptr, col, na, nb, ka, kb, chains, seed=9, **kw):
    return B.BlockModel(O.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rowptr, col),
                        n_chains=chains, seed=seed, **kw)


def _mixed_queries(deg):
    """11 queries: both types mixed, one repeated, one isolated node of each type"""
    assert deg[NA - 1] == 0 and deg[NA + NB - 1] == 0 and (deg[:NA - 2] > 0).all() and (deg[NA:NA + NB - 2] > 0).all()
    q = np.array([0, NA + 5, 17, NA - 1, NA + NB - 1, 450, NA + 300, 17, NA + 700 - 2, 902 - 2, NA])
    assert len(q) == 11 and (q < NA).any() and (q >= NA).any()
    return q


def _labels(m, chains):
    return [m.get_memberships(c) for c in chains]


def _rows(m, n_queries):
    got = [m.coassignment(i) for i in range(n_queries)]
    assert len({t for _, t in got}) == 1
    return [r for r, _ in got], got[0][1]


def _same(rows, want):
    assert len(rows) == len(want)
    for i, (r, w) in enumerate(zip(rows, want)):
        assert r.dtype == np.uint32 and r.shape == w.shape and (r == w).all(), (i, np.flatnonzero(r != w)[:8])
    return True


def _check_topk(m, na, queries, rows, ks):
    """coassign_topk == numpy_query_topk of the rows without the query's own node; returns the queries that had a tie at the
    k-th place"""
    tied = set()
    for k in ks:
        nodes, counts, terms = m.coassign_topk(k)
        assert nodes.shape == counts.shape == (len(queries), k) and nodes.dtype == counts.dtype == np.uint32
        assert terms == m.coassignment(0)[1]
        for i, q in enumerate(queries):
            first = 0 if q < na else na
            idx, val = D.numpy_query_topk(rows[i].astype(np.float64), k, excluded=[q - first])
            want = np.where(idx == NONE, NONE, idx.astype(np.int64) + first).astype(np.uint32)
            assert (nodes[i] == want).all(), (k, i, nodes[i], want)
            assert (counts[i] == val.astype(np.uint32)).all(), (k, i)
            assert q not in nodes[i]
            more, _ = D.numpy_query_topk(rows[i].astype(np.float64), k + 1, excluded=[q - first])
            if more[k] != NONE and rows[i][more[k]] == rows[i][more[k - 1]]:
                tied.add(i)
    return tied


@pytest.mark.parametrize("ka,kb", [(4, 4), (32, 32), (64, 64), (6, 5), (128, 128)])
def test_one_chain_one_sample(ka, kb):
    rowptr, col, deg = _graph()
    queries = _mixed_queries(deg)
    m = _model(rowptr, col, NA, NB, ka, kb, 1)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    m.coassign_set(queries)
    m.coassign_accumulate()
    rows, terms = _rows(m, len(queries))
    lab = m.get_memberships(0)
    assert terms == 1 and _same(rows, D.numpy_coassign([lab], queries, NA))
    n_r = m.get_n_r(0)
    for i, q in enumerate(queries):
        first = 0 if q < NA else NA
        assert rows[i].shape == ((NA,) if q < NA else (NB,))
        assert rows[i][q - first] == terms                 # the self cell
        assert int(rows[i].sum()) == int(n_r[lab[q]]), i   # the row sum: the size of the query's block
    assert (rows[2] == rows[7]).all()                      # the repeated query
    # symmetry between two queries of one type: (0, 17), (17, 450), (NA + 5, NA + 300), (NA, NA + 5)
    assert rows[0][17] == rows[2][0] and rows[2][450] == rows[5][17]
    assert rows[1][300] == rows[6][5] and rows[10][5] == rows[1][0]
    m.close()


def test_tile_boundaries():
    """two full candidate tiles plus a remainder that is no multiple of 4 in each type, two full query tiles plus one query of
    each type"""
    n_type, Q = 2 * B.COASSIGN_CAND_TILE + 3, 2 * B.COASSIGN_TILE + 1
    assert (n_type, Q) == (2051, 33)
    na = nb = n_type
    a, b = syn.planted_edges(na, nb, 9000, 4, 4, seed=6)
    rowptr, col = B.edge_to_adj((a, b), na + nb)
    step = (n_type - 1) // (Q - 1)
    qa = np.arange(Q) * step
    qa[-1] = na - 1
    queries = np.stack([qa, na + qa], axis=1).reshape(-1)  # the types alternate in the caller's order
    assert len(queries) == 2 * Q and queries.max() == na + nb - 1
    m = _model(rowptr, col, na, nb, 4, 4, 2)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    m.coassign_set(queries)
    m.coassign_accumulate()
    rows, terms = _rows(m, len(queries))
    assert terms == 2 and _same(rows, D.numpy_coassign(_labels(m, range(2)), queries, na))
    assert all(r[q - (0 if q < na else na)] == 2 for q, r in zip(queries, rows))
    m.close()


def test_more_counted_chains_than_a_byte_holds():
    chains = 300
    rowptr, col, deg = _graph()
    queries = _mixed_queries(deg)
    m = _model(rowptr, col, NA, NB, 4, 4, chains)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    m.coassign_set(queries)
    seen = []
    for sample in range(2):
        if sample:
            m.run_sweeps(1)
        seen += _labels(m, range(chains))
        m.coassign_accumulate()
    rows, terms = _rows(m, len(queries))
    assert terms == 600 and _same(rows, D.numpy_coassign(seen, queries, NA))
    assert max(int(r.max()) for r in rows) == 600
    m.close()


def test_identical_chains_count_exactly():
    """300 chains with the same labels, two samples: every co-block cell is exactly 600 and every other cell 0 (a partial that
    wraps at 256 gives 88)"""
    chains = 300
    rowptr, col, deg = _graph()
    queries = _mixed_queries(deg)
    lab = O.contiguous_labels(NA, NB, 4, 4)
    m = _model(rowptr, col, NA, NB, 4, 4, chains)
    m.set_memberships(lab)
    m.init_bisbm()
    m.coassign_set(queries)
    m.coassign_accumulate()
    m.coassign_accumulate()
    rows, terms = _rows(m, len(queries))
    assert terms == 600
    for i, q in enumerate(queries):
        own = lab[:NA] if q < NA else lab[NA:]
        assert (rows[i] == np.where(own == lab[q], 600, 0)).all(), i
    m.close()


def test_sixteen_chains_five_samples_and_topk():
    chains = 16
    rowptr, col, deg = _graph()
    queries = _mixed_queries(deg)
    m = _model(rowptr, col, NA, NB, 8, 8, chains)
    m.shuffle_bisbm()
    m.coassign_set(queries)
    seen = []
    for _ in range(5):
        m.run_sweeps(3)
        seen += _labels(m, range(chains))
        m.coassign_accumulate()
    rows, terms = _rows(m, len(queries))
    assert terms == 80 and _same(rows, D.numpy_coassign(seen, queries, NA))
    tied = _check_topk(m, NA, queries, rows, ks=(1, 10, 64))
    assert tied, "no query has a tie at the k-th place: the tie rule goes untested"
    # the largest k: more than the 902 / 700 eligible nodes, so every row is ranked in full and padded
    nodes, counts, _ = m.coassign_topk(B.QUERY_MAX_K)
    for i, q in enumerate(queries):
        eligible = (NA if q < NA else NB) - 1
        assert (nodes[i, :eligible] != NONE).all() and (nodes[i, eligible:] == NONE).all() and (counts[i, eligible:] == 0).all()
    _check_topk(m, NA, queries, rows, ks=(B.QUERY_MAX_K,))
    nodes, prob, t = m.similar(10)
    want_nodes, want_counts, _ = m.coassign_topk(10)
    assert t == 80 and (nodes == want_nodes).all() and prob.dtype == np.float64 and (prob == want_counts / 80).all()
    m.close()


def test_fewer_eligible_than_k():
    """three type-b nodes: a type-b query has two eligible nodes"""
    na, nb = NA, 3
    a, b = syn.planted_edges(na, nb, 2000, 4, 1, seed=8)
    rowptr, col = B.edge_to_adj((a, b), na + nb)
    m = _model(rowptr, col, na, nb, 4, 2, 4)
    m.shuffle_bisbm()
    queries = np.array([na + 1, 5, na + 2, na])
    m.coassign_set(queries)
    m.coassign_accumulate()
    rows, terms = _rows(m, len(queries))
    assert terms == 4 and _same(rows, D.numpy_coassign(_labels(m, range(4)), queries, na))
    nodes, counts, _ = m.coassign_topk(10)
    for i in (0, 2, 3):
        assert (nodes[i, :2] != NONE).all() and (nodes[i, 2:] == NONE).all() and (counts[i, 2:] == 0).all()
    assert (nodes[1] != NONE).all()
    _check_topk(m, na, queries, rows, ks=(10,))
    m.close()


def test_wide_handle_and_its_merge_down_to_byte_labels():
    rowptr, col, deg = _graph()
    queries = _mixed_queries(deg)
    m = _model(rowptr, col, NA, NB, 200, 150, 2, seed=2)
    m.shuffle_bisbm()
    m.run_sweeps(1)
    m.coassign_set(queries)
    m.coassign_accumulate()
    seen = _labels(m, range(2))
    assert max(int(x.max()) for x in seen) > 255  # two-byte labels are in use
    rows, terms = _rows(m, len(queries))
    assert terms == 2 and _same(rows, D.numpy_coassign(seen, queries, NA))
    _check_topk(m, NA, queries, rows, ks=(1, 10))
    m.agg_merge(50, 50, 10)  # 150 + 100 blocks: byte labels from here
    assert (m.KA, m.KB) == (150, 100)
    m.run_sweeps(1)
    seen += _labels(m, range(2))
    m.coassign_accumulate()
    rows, terms = _rows(m, len(queries))
    assert terms == 4 and _same(rows, D.numpy_coassign(seen, queries, NA))
    _check_topk(m, NA, queries, rows, ks=(10,))
    m.close()


def test_replica_exchange_counts_the_cold_chains():
    chains, ladder = 12, [1.0, 1.5, 2.5]
    rowptr, col, deg = _graph()
    queries = _mixed_queries(deg)
    m = _model(rowptr, col, NA, NB, 5, 5, chains)
    m.shuffle_bisbm()
    m.set_tempering(ladder)
    m.tempering_run(2, 1)
    m.coassign_set(queries)
    seen = []
    for sample in range(1, 3):
        m.tempering_run(3, 1)
        cold = np.flatnonzero(m.tempering_state()[0] == 0)
        assert len(cold) == chains // len(ladder)
        seen += _labels(m, cold)
        m.coassign_accumulate()
        assert m.coassignment(0)[1] == 4 * sample
    rows, terms = _rows(m, len(queries))
    assert terms == 8 and _same(rows, D.numpy_coassign(seen, queries, NA))
    m.close()


def test_chains_grouped_by_shape_all_count():
    g, deg, na, nb = _mixed_shapes_model()
    queries = np.array([3, na + 3, 499, na + 499, 250, 3])
    g.coassign_set(queries)
    g.coassign_accumulate()  # one shape still
    seen = _labels(g, range(g.n_chains))
    assert not g.mixed_shapes
    _merge_until_mixed(g)
    assert len({g.ka_kb(c) for c in range(g.n_chains)}) >= 2
    rows, terms = _rows(g, len(queries))  # the counts survive the merge
    assert terms == 32 and _same(rows, D.numpy_coassign(seen, queries, na))
    g.run_sweeps(1)
    seen += _labels(g, range(g.n_chains))
    g.coassign_accumulate()
    rows, terms = _rows(g, len(queries))
    assert terms == 64 and _same(rows, D.numpy_coassign(seen, queries, na))
    _check_topk(g, na, queries, rows, ks=(10,))
    g.close()
    # replica exchange over chains grouped by shape is refused
    g, deg, na, nb = _mixed_shapes_model()
    g.set_tempering([1.0, 1.3, 2.0, 3.5])
    g.coassign_set(queries)
    _merge_until_mixed(g)
    with pytest.raises(B.BisbmError) as e:
        g.coassign_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "grouped by shape" in str(e.value)
    g.close()


def test_two_device_entries_give_the_bits_of_one_handle():
    """devices=[0, 0] samples; one plain handle is then given the same labels chain by chain and counts them too"""
    chains = 16
    rowptr, col, deg = _graph()
    queries = _mixed_queries(deg)
    m = _model(rowptr, col, NA, NB, 5, 6, chains, devices=[0, 0])
    m.shuffle_bisbm()
    m.coassign_set(queries)
    samples = []
    for _ in range(2):
        m.run_sweeps(2)
        samples.append(_labels(m, range(chains)))
        m.coassign_accumulate()
    rows, terms = _rows(m, len(queries))
    assert terms == 2 * chains and _same(rows, D.numpy_coassign(samples[0] + samples[1], queries, NA))
    _check_topk(m, NA, queries, rows, ks=(10,))
    top = m.coassign_topk(20)
    m.coassign_reset()
    rows0, t0 = _rows(m, len(queries))
    assert t0 == 0 and all((r == 0).all() for r in rows0)
    m.close()
    one = _model(rowptr, col, NA, NB, 5, 6, chains)
    one.coassign_set(queries)
    for labs in samples:
        for c, lab in enumerate(labs):
            one.set_memberships(lab, c)
        one.init_bisbm()
        one.coassign_accumulate()
    rows1, t1 = _rows(one, len(queries))
    top1 = one.coassign_topk(20)
    one.close()
    assert t1 == terms and _same(rows1, rows)
    assert (top[0] == top1[0]).all() and (top[1] == top1[1]).all() and top[2] == top1[2] == 32


def test_call_order_and_refusals():
    chains = 4
    rowptr, col, deg = _graph()
    queries = _mixed_queries(deg)
    other = np.array([NA + 3, 7, 7])  # the query scores set beside the co-assignment queries

    def plain_query_scores():
        p = _model(rowptr, col, NA, NB, 4, 4, chains)
        p.shuffle_bisbm()
        p.run_sweeps(2)
        p.query_scores_set(other)
        p.query_scores_accumulate()
        p.run_sweeps(1)
        p.query_scores_accumulate()
        got = [p.query_scores(i) for i in range(len(other))]
        p.close()
        return got
    m = _model(rowptr, col, NA, NB, 4, 4, chains)
    with pytest.raises(B.BisbmError) as e:  # no queries
        m.coassign_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "queries" in str(e.value)
    m.coassign_set(queries)
    with pytest.raises(B.BisbmError) as e:  # no block state yet
        m.coassign_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "bisbm_init" in str(e.value)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    with pytest.raises(B.BisbmError) as e:  # before any sample
        m.coassign_topk(5)
    assert e.value.code == B.BISBM_ERR_STATE and "sample" in str(e.value)
    m.query_scores_set(other)
    m.query_scores_accumulate()
    m.coassign_accumulate()
    first = _labels(m, range(chains))
    rows, terms = _rows(m, len(queries))
    assert terms == chains and _same(rows, D.numpy_coassign(first, queries, NA))
    with pytest.raises(B.BisbmError) as e:
        m.coassign_topk(0)
    assert e.value.code == B.BISBM_ERR_INVALID_ARG
    with pytest.raises(B.BisbmError) as e:
        m.coassign_topk(B.QUERY_MAX_K + 1)
    assert e.value.code == B.BISBM_ERR_UNSUPPORTED and str(B.QUERY_MAX_K) in str(e.value)
    # a query id >= n is refused and leaves the earlier queries and their counts in place
    for bad, index in (([0, NA + NB], 1), ([NA + NB], 0), ([3, 4, 4000000000], 2)):
        with pytest.raises(B.BisbmError) as e:
            m.coassign_set(np.array(bad))
        assert e.value.code == B.BISBM_ERR_INVALID_ARG and ("query %d " % index) in str(e.value), str(e.value)
        rows2, t2 = _rows(m, len(queries))
        assert t2 == terms and _same(rows2, rows)
    with pytest.raises(ValueError):
        m.coassign_set(np.zeros((3, 2), dtype=np.int64))
    # reset zeroes the counts and keeps the queries
    m.coassign_reset()
    rows0, t0 = _rows(m, len(queries))
    assert t0 == 0 and all((r == 0).all() for r in rows0)
    with pytest.raises(B.BisbmError) as e:
        m.coassign_topk(5)
    assert e.value.code == B.BISBM_ERR_STATE
    m.run_sweeps(1)
    m.query_scores_accumulate()
    m.coassign_accumulate()
    second = _labels(m, range(chains))
    rows1, t1 = _rows(m, len(queries))
    assert t1 == chains and _same(rows1, D.numpy_coassign(second, queries, NA))
    # set again replaces the rows and zeroes
    again = queries[:3][::-1].copy()
    m.coassign_set(again)
    rows2, t2 = _rows(m, 3)
    assert t2 == 0 and [len(r) for r in rows2] == [NA, NB, NA] and all((r == 0).all() for r in rows2)
    with pytest.raises(IndexError):
        m.coassignment(3)
    m.coassign_accumulate()
    assert _same(_rows(m, 3)[0], D.numpy_coassign(second, again, NA))
    # an empty set frees everything
    m.coassign_set(np.zeros(0, dtype=np.int64))
    with pytest.raises(B.BisbmError) as e:
        m.coassign_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "queries" in str(e.value)
    with pytest.raises(B.BisbmError) as e:
        m.coassign_topk(5)
    assert e.value.code == B.BISBM_ERR_STATE
    # the query scores of the same handle never noticed
    got = [m.query_scores(i) for i in range(len(other))]
    m.close()
    for (r, t), (r0, t0) in zip(got, plain_query_scores()):
        assert t == t0 == 2 * chains and (r.view(np.uint64) == r0.view(np.uint64)).all()


def _write_similar(path, queries, nodes, prob):
    with open(path, "w") as f:
        for i, q in enumerate(queries):
            for node, s in zip(nodes[i], prob[i]):
                if node != NONE:
                    f.write("%d %d %s\n" % (q, node, "%.17g" % s))


def test_cli_marginalize_and_the_model_agree(tmp_path):
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
    r = subprocess.run(common + ["--similar", str(qin), str(qout), str(k)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def fresh(labels, rp, cl):
        m = B.BlockModel(labels, syn.types_vector(na, nb), 8, 4, 4, 1.0, (rp, cl), n_chains=chains, seed=seed)
        m.shuffle_bisbm()
        return m
    m = fresh(O.contiguous_labels(na, nb, 4, 4), rowptr, col)
    labels, _, (nodes, prob, terms) = B.marginalize(m, 10, 3, 2, similar=(queries, k))
    assert terms == 3 * chains and len(r.stdout.split()) == n == len(labels)  # (stdout: the marginal labels still)
    _write_similar(want, queries, nodes, prob)
    assert qout.read_text() == want.read_text() and len(qout.read_text().splitlines()) == len(queries) * k
    rows, _ = _rows(m, len(queries))
    m.close()
    # the model: the same chains advanced by hand, their labels taken at every sample
    m = fresh(O.contiguous_labels(na, nb, 4, 4), rowptr, col)
    m.run_sweeps(10)
    seen = []
    for _ in range(3):
        m.run_sweeps(2)
        seen += _labels(m, range(chains))
    m.close()
    ref = D.numpy_coassign(seen, queries, na)
    assert _same(rows, ref)
    for i, q in enumerate(queries):
        first = 0 if q < na else na
        idx, val = D.numpy_query_topk(ref[i].astype(np.float64), k, excluded=[q - first])
        assert (nodes[i] == idx + first).all() and (prob[i] == val / terms).all()
    # recommend and similar together: both results, in that order, at the end of the return value
    m = fresh(O.contiguous_labels(na, nb, 4, 4), rowptr, col)
    out = B.marginalize(m, 10, 3, 2, recommend=(queries, 5), similar=(queries, k))
    assert len(out) == 4 and out[2][0].shape == (len(queries), 5) and (out[3][0] == nodes).all() and (out[3][1] == prob).all()
    m.close()
    # --reorder: queries and nodes are given and printed in the file's own ids; the engine counts the renumbered nodes
    r = subprocess.run(common + ["--reorder", "--similar", str(qin), str(qout), str(k)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lo = B.locality_order(rowptr, col, na, nb)
    rp2, cl2 = lo.apply(rowptr, col)
    m = fresh(lo.to_new(O.contiguous_labels(na, nb, 4, 4)), rp2, cl2)
    _, _, (nodes, prob, _) = B.marginalize(m, 10, 3, 2, similar=(lo.new_id[queries], k))
    old = np.argsort(lo.new_id)
    _write_similar(want, queries, np.where(nodes == NONE, NONE, old[np.minimum(nodes, n - 1)]), prob)
    assert qout.read_text() == want.read_text()
    m.close()


def test_example_runs():
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "similar_nodes.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "share the block of" in r.stdout, r.stdout + r.stderr
