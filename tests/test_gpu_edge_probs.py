"""GPU tests of the edge probabilities (include/bisbm.h, "Edge probabilities").  The model is distributed.numpy_edge_dS -- the
stated host loop, pinned to the checker library's description length by tests/test_edge_probs.py -- fed with what the handle's
own getters return (block state with eta), the device's log_q (debug_log_q, fast=False), the C library's lgamma (the values
the engine's table holds; through the checker library) and, for w, the device's exp (debug_exp).  The same f64 operations in the same order: bit-equal."""
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from test_edge_probs import KA, KB, NA, NB, all_edits, edited, small_graph, tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu


def LG(i):
    """lgamma(i) of the C library, the entries of the engine's host-built table (math.lgamma is Python's own)"""
    return O.lib().orc_lgamma_fast(i) if i else math.inf


def same(a, b):
    return (np.asarray(a, dtype=np.float64).view(np.uint64) == np.asarray(b, dtype=np.float64).view(np.uint64)).all()


def small_model(chains, **kw):
    a, b, labels = small_graph()
    rowptr, col = O.edge_to_csr(a, b, NA + NB)
    m = B.BlockModel(labels, syn.types_vector(NA, NB), KA + KB, KA, KB, 1.0, (rowptr, col), n_chains=chains, seed=5, **kw)
    return m, a, b, labels, rowptr, col


def chain_dS(m, c, pairs, kinds, mult, deg):
    """the model's dS of every pair in chain c of the handle, from the handle's getters and probes"""
    ka, kb = m.ka_kb(c)
    lab = m.get_memberships(c)
    M, mr, nr, eta = m._block_state(c, ("m", "m_r", "n_r", "eta"))
    ks, ns = np.concatenate([mr - 1, mr, mr + 1]), np.tile(nr, 3)
    table = dict(zip(zip(ks.tolist(), ns.tolist()), m.debug_log_q(ks, ns, fast=False).tolist()))
    return np.array([D.numpy_edge_dS(M, mr, nr, eta, deg, lab, ka, kb, m.num_edges, u, v, kd, mu, LG, lambda k, n: table[(k, n)])
                     for (u, v), kd, mu in zip(np.asarray(pairs).tolist(), np.asarray(kinds).tolist(), np.asarray(mult).tolist())])


def fold(m, dS_sum, w_sum, dS):
    """one chain onto the running sums: one f64 add each, w with the device's exp"""
    dS_sum += dS
    w_sum += np.where(dS > 700.0, 0.0, m.debug_exp(-dS))


def model_sample(m, dS_sum, w_sum, pairs, kinds, mult, deg, chains=None):
    """every given chain (default: all), in the order given, onto the sums; returns the per-chain dS"""
    per = {}
    for c in (range(m.n_chains) if chains is None else chains):
        per[c] = chain_dS(m, c, pairs, kinds, mult, deg)
        fold(m, dS_sum, w_sum, per[c])
    return per


def test_every_chain_and_both_sums_are_the_model_bit_for_bit():
    chains = 5
    m, a, b, labels, rowptr, col = small_model(chains)
    deg = np.diff(rowptr.astype(np.int64))
    pairs, kinds = all_edits(a, b)
    mult = D.numpy_edge_multiplicity(rowptr, col, pairs)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    m.edge_probs_set(pairs, kinds, keep_last=True)
    ds, w = np.zeros(len(pairs)), np.zeros(len(pairs))
    for sample in (1, 2):
        per = model_sample(m, ds, w, pairs, kinds, mult, deg)
        m.edge_probs_accumulate()
        for i in range(len(pairs)):
            got = m.edge_probs_last(i)
            assert same(got, [per[c][i] for c in range(chains)]), (sample, i, got, [per[c][i] for c in range(chains)])
        r = m.edge_probs()
        assert r["terms"] == sample * chains and (r["mult"] == mult).all()
        assert same(r["dS_sum"], ds) and same(r["w_sum"], w)
        assert same(r["mean_dS"], ds / r["terms"])
        assert np.isfinite(r["log_prob"]).all() and same(r["log_prob"], [math.log(x / r["terms"]) for x in w])
        m.run_sweeps(1)
    assert len({tuple(m.get_memberships(c)) for c in range(chains)}) > 1  # (different shuffles: the chains differ)
    m.close()


def test_dS_is_the_change_of_the_description_length():
    """12 pairs x 2 chains: the device's dS against entropy() of a second handle built on the edited graph with the chain's
    labels.  Tolerance as in tests/test_edge_probs.py: the summand count of the description length times half an ulp, twice."""
    m, a, b, labels, rowptr, col = small_model(2)
    n = NA + NB
    deg = np.diff(rowptr.astype(np.int64))
    m.shuffle_bisbm()
    m.run_sweeps(3)
    ua, vb = int(np.argmax(deg[:NA])), NA + int(np.argmax(deg[NA:]))
    edges = np.stack([a, b], axis=1)
    uniq, cnt = np.unique(edges, axis=0, return_counts=True)
    once, twice = uniq[cnt == 1], uniq[cnt >= 2]
    present = set(map(tuple, uniq.tolist()))
    absent = next((u, v) for u in range(NA - 1) for v in range(NA, n - 1) if (u, v) not in present and u != ua and v != vb)
    of_ua = next(p for p in uniq.tolist() if p[0] == ua)
    of_vb = next(p for p in uniq.tolist() if p[1] == vb)
    pairs = np.array([(ua, vb), (14, 26), (14, vb), (ua, 26), absent, once[0], twice[0],  # ADD: mu = 0, 1 and >= 2 among them
                      once[1], twice[1], of_ua, of_vb, twice[2]])                          # REMOVE: mu = 1 and >= 2
    kinds = np.array([0] * 7 + [1] * 5, dtype=np.uint8)
    mult = D.numpy_edge_multiplicity(rowptr, col, pairs)
    assert mult[4] == 0 and mult[5] == 1 and mult[6] >= 2 and mult[7] == 1 and mult[8] >= 2 and (mult[7:] >= 1).all()
    assert deg[14] == 0 and deg[26] == 0 and deg[ua] == deg[:NA].max() and deg[vb] == deg[NA:].max()
    m.edge_probs_set(pairs, kinds, keep_last=True)
    m.edge_probs_accumulate()
    assert (m.edge_probs()["mult"] == mult).all()
    S0 = m.entropy()
    worst = 0.0
    for i, ((u, v), kd) in enumerate(zip(pairs.tolist(), kinds.tolist())):
        got = m.edge_probs_last(i)
        a1, b1 = edited(a, b, u, v, kd)
        rp1, cl1 = O.edge_to_csr(a1, b1, n)
        g = B.BlockModel(labels, syn.types_vector(NA, NB), KA + KB, KA, KB, 1.0, (rp1, cl1), n_chains=2, seed=5)
        for c in range(2):
            g.set_memberships(m.get_memberships(c), chain=c)
        g.init_bisbm()
        S1 = g.entropy()
        g.close()
        for c in range(2):
            err = abs(got[c] - (S1[c] - S0[c]))
            worst = max(worst, err)
            assert err <= tolerance(n, KA, KB, m.max_degree, S0[c], S1[c]), (i, c, got[c], S1[c] - S0[c])
    print("worst |dS - (S1 - S0)| = %.3g at S0 = %.6g" % (worst, S0[0]))
    m.close()


@pytest.mark.parametrize("range_chains", [None, 4])
def test_a_tile_and_one_pair_nine_chains_unsorted_repeating_pairs(range_chains, monkeypatch):
    """Two workgroups, the second with one pair; with BISBM_EDGE_RANGE_CHAINS=4 the nine chains also go in three launches."""
    if range_chains:
        monkeypatch.setenv("BISBM_EDGE_RANGE_CHAINS", str(range_chains))
    chains, P = 9, B.EDGE_PROBS_TILE + 1
    m, a, b, labels, rowptr, col = small_model(chains)
    deg = np.diff(rowptr.astype(np.int64))
    base, base_kinds = all_edits(a, b)
    pick = np.random.default_rng(8).integers(0, len(base), P)  # (236 edits drawn 1025 times: they repeat, in no order)
    pairs, kinds = base[pick], base_kinds[pick]
    mult = D.numpy_edge_multiplicity(rowptr, col, pairs)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    m.edge_probs_set(pairs, kinds, keep_last=bool(range_chains))
    ds, w = np.zeros(P), np.zeros(P)
    # (the model per distinct edit, spread over the repeats)
    ub, uk = all_edits(a, b)
    umult = D.numpy_edge_multiplicity(rowptr, col, ub)
    for c in range(chains):
        fold(m, ds, w, chain_dS(m, c, ub, uk, umult, deg)[pick])
    m.edge_probs_accumulate()
    r = m.edge_probs()
    assert r["terms"] == chains and (r["mult"] == mult).all()
    assert same(r["dS_sum"], ds) and same(r["w_sum"], w)
    if range_chains:
        assert same(m.edge_probs_last(P - 1), [chain_dS(m, c, pairs[-1:], kinds[-1:], mult[-1:], deg)[0] for c in range(chains)])
    else:
        with pytest.raises(B.BisbmError) as e:  # nothing kept
            m.edge_probs_last(0)
        assert e.value.code == B.BISBM_ERR_STATE
    m.close()


def test_replica_exchange_counts_rung_zero_only():
    chains, L = 6, 3
    m, a, b, labels, rowptr, col = small_model(chains)
    deg = np.diff(rowptr.astype(np.int64))
    pairs, kinds = all_edits(a, b)
    pairs, kinds = pairs[::5], kinds[::5]
    mult = D.numpy_edge_multiplicity(rowptr, col, pairs)
    m.shuffle_bisbm()
    m.set_tempering([1.0, 1.5, 2.5])
    m.edge_probs_set(pairs, kinds, keep_last=True)
    ds, w = np.zeros(len(pairs)), np.zeros(len(pairs))
    for sample in (1, 2):
        m.tempering_run(3, 1)
        cold = np.flatnonzero(m.tempering_state()[0] == 0)
        assert len(cold) == chains // L
        per = model_sample(m, ds, w, pairs, kinds, mult, deg, cold.tolist())
        m.edge_probs_accumulate()
        r = m.edge_probs()
        assert r["terms"] == 2 * sample and same(r["dS_sum"], ds) and same(r["w_sum"], w)
        last = m.edge_probs_last(3)
        assert np.isnan(last[np.setdiff1d(np.arange(chains), cold)]).all() and same(last[cold], [per[c][3] for c in cold])
    m.close()


def test_chains_grouped_by_shape_each_group_with_its_own_edge_prior():
    rowptr, col, na, nb = O.load_graph("n_1000")
    n, chains = na + nb, 12
    deg = np.diff(rowptr.astype(np.int64))
    g = B.BlockModel(O.contiguous_labels(na, nb, 8, 9), syn.types_vector(na, nb), 17, 8, 9, 1.0, (rowptr, col), n_chains=chains, seed=123)
    g.shuffle_bisbm()
    g.run_sweeps(3)
    rs = np.random.default_rng(2)
    add = np.stack([rs.integers(0, na, 40), na + rs.integers(0, nb, 40)], axis=1)
    us = rs.integers(0, na, 60)
    us = us[deg[us] > 0][:24]
    rem = np.stack([us, col[rowptr[us].astype(np.int64)]], axis=1).astype(np.int64)  # every such node's first edge
    pairs, kinds = np.concatenate([add, rem]), np.array([0] * len(add) + [1] * len(rem), dtype=np.uint8)
    mult = D.numpy_edge_multiplicity(rowptr, col, pairs)
    g.edge_probs_set(pairs, kinds, keep_last=True)
    ds, w = np.zeros(len(pairs)), np.zeros(len(pairs))
    model_sample(g, ds, w, pairs, kinds, mult, deg)
    g.edge_probs_accumulate()  # one shape still
    g.agg_merge(5, None, 10)  # (the diverging one-argument merge of test_chains_may_end_with_different_block_counts)
    shapes = [g.ka_kb(c) for c in range(chains)]
    assert g.mixed_shapes and len(set(shapes)) > 1
    g.run_sweeps(1)
    # the groups in order of first appearance of their shape, every group's chains ascending: sums and terms carried over
    first = {s: shapes.index(s) for s in set(shapes)}
    order = sorted(range(chains), key=lambda c: (first[shapes[c]], c))
    per = model_sample(g, ds, w, pairs, kinds, mult, deg, order)
    g.edge_probs_accumulate()
    r = g.edge_probs()
    assert r["terms"] == 2 * chains and same(r["dS_sum"], ds) and same(r["w_sum"], w)
    for i in (0, 45):
        assert same(g.edge_probs_last(i), [per[c][i] for c in range(chains)])
    g.close()


def test_rungs_over_groups_are_refused():
    rowptr, col, na, nb = O.load_graph("n_1000")
    g = B.BlockModel(O.contiguous_labels(na, nb, 8, 9), syn.types_vector(na, nb), 17, 8, 9, 1.0, (rowptr, col), n_chains=12, seed=123)
    g.shuffle_bisbm()
    g.run_sweeps(3)
    g.set_tempering([1.0, 1.3, 2.0])
    g.edge_probs_set(np.array([[0, na]]))
    g.edge_probs_accumulate()
    g.agg_merge(5, None, 10)
    assert g.mixed_shapes
    with pytest.raises(B.BisbmError) as e:
        g.edge_probs_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "grouped by shape" in str(e.value)
    assert g.edge_probs()["terms"] == 4
    g.close()


def test_a_device_listed_twice_adds_the_entries_sums_in_entry_order():
    chains = 6
    m, a, b, labels, rowptr, col = small_model(chains, devices=[0, 0])
    deg = np.diff(rowptr.astype(np.int64))
    pairs, kinds = all_edits(a, b)
    mult = D.numpy_edge_multiplicity(rowptr, col, pairs)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    m.edge_probs_set(pairs, kinds, keep_last=True)
    first = m.device_layout()[1] + [chains]
    assert len(first) == 3
    parts = [(np.zeros(len(pairs)), np.zeros(len(pairs))) for _ in range(2)]
    per = {}
    for sample in range(2):
        for k in range(2):
            per.update(model_sample(m, parts[k][0], parts[k][1], pairs, kinds, mult, deg, range(first[k], first[k + 1])))
        m.edge_probs_accumulate()
        m.run_sweeps(1)
    r = m.edge_probs()
    assert r["terms"] == 2 * chains and (r["mult"] == mult).all()
    assert same(r["dS_sum"], (0.0 + parts[0][0]) + parts[1][0]) and same(r["w_sum"], (0.0 + parts[0][1]) + parts[1][1])
    assert same(m.edge_probs_last(7), [per[c][7] for c in range(chains)])
    m.edge_probs_reset()
    r = m.edge_probs()
    assert r["terms"] == 0 and (r["dS_sum"] == 0).all() and (r["w_sum"] == 0).all()
    m.close()


def test_wide_labels_and_the_compat_mode():
    rowptr, col, na, nb = O.load_graph("n_1000")
    deg = np.diff(rowptr.astype(np.int64))
    g = B.BlockModel(O.contiguous_labels(na, nb, 200, 150), syn.types_vector(na, nb), 350, 200, 150, 1.0, (rowptr, col), n_chains=2, seed=2)
    g.shuffle_bisbm()
    g.run_sweeps(1)
    rs = np.random.default_rng(4)
    add = np.stack([rs.integers(0, na, 40), na + rs.integers(0, nb, 40)], axis=1)
    us = np.flatnonzero(deg[:na] > 0)[:24]
    rem = np.stack([us, col[rowptr[us].astype(np.int64)]], axis=1).astype(np.int64)
    pairs, kinds = np.concatenate([add, rem]), np.array([0] * 40 + [1] * 24, dtype=np.uint8)
    mult = D.numpy_edge_multiplicity(rowptr, col, pairs)
    g.edge_probs_set(pairs, kinds)
    ds, w = np.zeros(64), np.zeros(64)
    model_sample(g, ds, w, pairs, kinds, mult, deg)
    g.edge_probs_accumulate()
    r = g.edge_probs()
    assert r["terms"] == 2 and same(r["dS_sum"], ds) and same(r["w_sum"], w)
    g.close()
    m, a, b, labels, rowptr, col = small_model(2, rng="mt19937-compat", gen_seed=9)
    deg = np.diff(rowptr.astype(np.int64))
    pairs, kinds = all_edits(a, b)
    mult = D.numpy_edge_multiplicity(rowptr, col, pairs)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    m.edge_probs_set(pairs, kinds)
    ds, w = np.zeros(len(pairs)), np.zeros(len(pairs))
    model_sample(m, ds, w, pairs, kinds, mult, deg)
    m.edge_probs_accumulate()
    r = m.edge_probs()
    assert r["terms"] == 2 and same(r["dS_sum"], ds) and same(r["w_sum"], w)
    m.close()


def test_128_plus_128_blocks_the_largest_tables_in_lds():
    """Byte labels at their limit: two buffers of 4 x 256 block terms and a 128 x 128 quadrant, 144 KiB of LDS."""
    import cases
    rowptr, col = cases.random_graph(17, 400, 400, 6000, 128, 128)
    na = nb = 400
    deg = np.diff(rowptr.astype(np.int64))
    g = B.BlockModel(O.contiguous_labels(na, nb, 128, 128), syn.types_vector(na, nb), 256, 128, 128, 1.0, (rowptr, col), n_chains=2, seed=21)
    g.shuffle_bisbm()
    g.run_sweeps(1)
    rs = np.random.default_rng(6)
    add = np.stack([rs.integers(0, na, 40), na + rs.integers(0, nb, 40)], axis=1)
    us = np.flatnonzero(deg[:na] > 0)[:24]
    rem = np.stack([us, col[rowptr[us].astype(np.int64)]], axis=1).astype(np.int64)
    pairs, kinds = np.concatenate([add, rem]), np.array([0] * 40 + [1] * 24, dtype=np.uint8)
    mult = D.numpy_edge_multiplicity(rowptr, col, pairs)
    g.edge_probs_set(pairs, kinds)
    ds, w = np.zeros(64), np.zeros(64)
    model_sample(g, ds, w, pairs, kinds, mult, deg)
    g.edge_probs_accumulate()
    r = g.edge_probs()
    assert r["terms"] == 2 and same(r["dS_sum"], ds) and same(r["w_sum"], w)
    g.close()


def _snapshot(m):
    return [(m.get_memberships(c).tolist(), [x.tolist() for x in m._block_state(c, ("m", "m_r", "n_r", "eta"))]) for c in range(m.n_chains)] + [
        m.get_entropy().tolist()]


def test_state_is_only_read_and_refusals_keep_what_was_there():
    m, a, b, labels, rowptr, col = small_model(4)
    twin = small_model(4)[0]
    pairs, kinds = all_edits(a, b)
    m.edge_probs_set(pairs, kinds)
    with pytest.raises(B.BisbmError) as e:  # no block state yet
        m.edge_probs_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "bisbm_init" in str(e.value)
    for g in (m, twin):
        g.shuffle_bisbm()
        g.run_sweeps(2)
    before = _snapshot(m)
    m.edge_probs_accumulate()
    assert _snapshot(m) == before == _snapshot(twin)
    assert (m.run_sweeps(1) == twin.run_sweeps(1)).all() and _snapshot(m) == _snapshot(twin)  # the next sweep too
    m.edge_probs_reset()
    r = m.edge_probs()
    assert r["terms"] == 0 and (r["dS_sum"] == 0).all() and (r["w_sum"] == 0).all() and np.isnan(r["log_prob"]).all()
    m.edge_probs_accumulate()  # reset keeps the pairs
    r = m.edge_probs()
    assert r["terms"] == 4 and len(r["dS_sum"]) == len(pairs)
    present = set(map(tuple, np.stack([a, b], axis=1).tolist()))
    non = next([u, v] for u in range(NA) for v in range(NA, NA + NB) if (u, v) not in present)
    edge = [int(a[0]), int(b[0])]
    for bad, bad_kinds, index, word in (([[0, NA], [5, 5]], None, 1, "type-a"), ([[NA, NA + 1]], None, 0, "type-a"),
                                        ([[0, NA], [1, NA + 1]], [0, 2], 1, "kind"),
                                        ([edge, [0, NA], non], [1, 0, 1], 2, "REMOVE")):
        with pytest.raises(B.BisbmError) as e:
            m.edge_probs_set(np.array(bad), bad_kinds)
        assert e.value.code == B.BISBM_ERR_INVALID_ARG and ("pair %d " % index) in str(e.value) and word in str(e.value), str(e.value)
        r2 = m.edge_probs()  # the earlier pairs and their sums are intact
        assert r2["terms"] == 4 and same(r2["dS_sum"], r["dS_sum"]) and same(r2["w_sum"], r["w_sum"])
    u32 = np.zeros(1, dtype=np.uint32)
    rc = m._L.bisbm_edge_probs_set(m._h, 1, B._p(u32, B._u32p), B._p(u32 + NA, B._u32p), None, 2)  # an unknown bit of `what`
    assert rc == B.BISBM_ERR_INVALID_ARG and same(m.edge_probs()["dS_sum"], r["dS_sum"])
    with pytest.raises(ValueError):
        m.edge_probs_set(np.zeros((3, 3), dtype=np.int64))
    m.edge_probs_set(np.zeros((0, 2), dtype=np.int64))  # frees everything
    for call in (m.edge_probs_accumulate, m.edge_probs):
        with pytest.raises(B.BisbmError) as e:
            call()
        assert e.value.code == B.BISBM_ERR_STATE
    m.close()
    twin.close()


def test_cli_lines_equal_the_python_driver(tmp_path):
    rowptr, col, na, nb = O.load_graph("n_1000")
    n, chains, seed = na + nb, 8, 5
    deg = np.diff(rowptr.astype(np.int64))
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    rs = np.random.default_rng(3)
    add = np.stack([rs.integers(0, na, 200), na + rs.integers(0, nb, 200)], axis=1)
    us = np.flatnonzero(deg[:na] > 0)[:100]
    rem = np.stack([us, col[rowptr[us].astype(np.int64)]], axis=1).astype(np.int64)
    pairs, kinds = np.concatenate([add, rem]), np.array([0] * 200 + [1] * 100, dtype=np.uint8)
    marks = ["", " +"] * 100 + [" -"] * 100  # (an ADD line with and without its sign)
    pin, pout = tmp_path / "pairs.txt", tmp_path / "probs.txt"
    pin.write_text("".join("%d %d%s\n" % (u, v, s) for (u, v), s in zip(pairs.tolist(), marks)))
    sizes = [str(x) for x in np.bincount(O.contiguous_labels(na, nb, 4, 4))]
    common = [cli, "-e", el, "-y", str(na), str(nb), "-z", "4", "4", "-n", *sizes, "-r", "-d", str(seed), "--rng", "philox", "--chains", str(chains),
              "-b", str(10 * n), "-t", str(6 * n), "-f", str(2 * n), "--marginalize"]
    r = subprocess.run(common + ["--edge_probs", str(pin), str(pout)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert len(r.stdout.split()) == n
    m = B.BlockModel(O.contiguous_labels(na, nb, 4, 4), syn.types_vector(na, nb), 8, 4, 4, 1.0, (rowptr, col), n_chains=chains, seed=seed)
    m.shuffle_bisbm()
    B.marginalize(m, 10, 3, 2, edge_probs=(pairs, kinds))
    e = m.edge_probs()
    assert e["terms"] == 3 * chains
    want = ["%d %d %s %d %.17g %.17g" % (u, v, "-" if kd else "+", mu, x, y)
            for (u, v), kd, mu, x, y in zip(pairs.tolist(), kinds.tolist(), e["mult"].tolist(), e["mean_dS"].tolist(), e["log_prob"].tolist())]
    assert pout.read_text().splitlines() == want
    m.close()


def test_example_runs():
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "edge_probabilities.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "terms per pair: 320" in r.stdout, r.stdout + r.stderr
