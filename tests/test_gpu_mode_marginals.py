"""GPU tests of the mode-resolved marginals (include/bisbm.h, "Mode-resolved marginals"): two planted modes recovered each in its
own histogram, exactness of the per-mode overlap / assignment / counting / argmax kernels against the numpy model of
tests/test_mode_marginals.py (aligned_sample of tests/test_align.py applied to each mode's chains with that mode's reference;
every comparison integer-exact), chains left untouched, several device entries, the refusals and state rules, the Python
driver and the CLI."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from test_align import PLANTED, agreement, planted_graph
from test_mode_marginals import TWO_MODES, mode_sample, two_mode_pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")
NONE = B.MODE_NONE

pytestmark = pytest.mark.gpu


def _model(na, nb, ka, kb, edges, chains, rng="philox", seed=9, graph_seed=4, labels=None, **kw):
    a, b = syn.planted_edges(na, nb, edges, ka, kb, seed=graph_seed)
    rp, cl = B.edge_to_adj((a, b), na + nb)
    lab = syn.contiguous_labels(na, nb, ka, kb) if labels is None else labels
    return B.BlockModel(lab, syn.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rp, cl), n_chains=chains, rng=rng, seed=seed,
                        gen_seed=seed + 1, **kw)


def _all_labels(m):
    return np.array([m.get_memberships(c) for c in range(m.n_chains)])


def _check_samples(m, moc, samples=3, sweeps_between=1):
    """`samples` mode-resolved samples of m against the model: per-mode counts, every counted chain's permutation and overlap
    total, terms, the library's choice of every reference, MAP labels and top."""
    moc = np.asarray(moc, dtype=np.uint32)
    M = int(moc[moc != NONE].max()) + 1
    na, ka, kb = m.na, m.KA, m.KB
    base = np.where(np.arange(m.n) >= na, ka, 0)
    m.marginals_reset()
    m.marginals_set_modes(moc)
    assert m.marginals_modes()["ref_chain"].tolist() == [-2] * M
    want = np.zeros((M, m.n, max(ka, kb)), dtype=np.int64)
    refs = None
    for sample in range(samples):
        labs, S = _all_labels(m), m.entropy()
        m.marginals_accumulate()
        state = m.marginals_modes()
        if refs is None:
            refs = []
            for g in range(M):
                members = np.flatnonzero(moc == g)
                ref, chain = m.marginals_reference(mode=g)
                assert chain == state["ref_chain"][g] == members[np.argmin(S[members])] and (ref == labs[chain]).all(), g
                refs.append(ref)
        counts, perms, totals = mode_sample(labs, np.where(moc == NONE, -1, moc.astype(np.int64)), refs, na, ka, kb)
        want += counts
        for c in range(m.n_chains):
            if moc[c] == NONE:
                with pytest.raises(B.BisbmError) as e:
                    m.marginals_alignment(c)
                assert e.value.code == B.BISBM_ERR_STATE
                continue
            perm, tot = m.marginals_alignment(c)
            assert (perm == perms[c]).all() and tot == totals[c], (sample, c)
        assert state["n_modes"] == M and (state["mode_of_chain"] == moc).all()
        assert state["terms"].tolist() == [(sample + 1) * int((moc == g).sum()) for g in range(M)]
        for g in range(M):
            assert (m.marginals_get(mode=g).astype(np.int64) == want[g]).all(), (sample, g)
            labels, top = m.marginals_map(mode=g, return_top=True)
            assert (labels == want[g].argmax(axis=1) + base).all() and (top == want[g].max(axis=1)).all(), (sample, g)
        if sample + 1 < samples:
            m.run_sweeps(sweeps_between)
    return want, refs


# ---------------------------------------------------------------------------------------------------- 1. two planted modes
def test_two_planted_modes_each_in_its_own_histogram():
    t = TWO_MODES
    na, nb, ka, kb = t["na"], t["nb"], t["ka"], t["kb"]
    P, Q, starts = two_mode_pool()
    m = _model(na, nb, ka, kb, 3000, t["chains"])
    for c, start in enumerate(starts):
        m.set_memberships(start, chain=c)
    m.init_bisbm()
    modes = m.partition_modes(1.5)
    assert modes["mode"].tolist() == [0, 1] * 8  # (numpy: the largest VI within a mode is 1.257, the smallest between 1.862)
    m.marginals_set_modes(modes)
    m.marginals_accumulate()
    state = m.marginals_modes()
    assert state["terms"].tolist() == [8, 8] and state["weights"].tolist() == [0.5, 0.5]
    refs = [m.marginals_reference(mode=g)[0] for g in range(2)]
    counts, _, _ = mode_sample(starts, np.arange(16) % 2, refs, na, ka, kb)
    for g, truth in enumerate((P, Q)):
        assert (m.marginals_get(mode=g).astype(np.int64) == counts[g]).all()
        assert agreement(m.marginals_map(mode=g), truth, na, ka, kb) == 1.0


# ---------------------------------------------------------------------------------------------------- 2. exactness over shapes
def _assignment(chains):
    if chains == 16:  # three modes of 9 / 1 / 4 chains and two uncounted ones, interleaved
        return [0, 2, 0, NONE, 0, 2, 1, 0, 0, 2, 0, NONE, 0, 2, 0, 0]
    moc = [c % 2 for c in range(chains)]
    if chains >= 5:
        moc[3] = NONE
    return moc


SHAPES = [  # na, nb, ka, kb, edges, chains, rng, empty_block
    (300, 200, 4, 4, 3000, 16, "philox", False),
    (300, 200, 7, 3, 3000, 8, "mt19937-compat", False),
    (900, 700, 60, 40, 20000, 6, "philox", False),   # one LDS table per workgroup
    (800, 800, 100, 100, 20000, 5, "philox", False),  # tables counted in HBM
    (600, 300, 200, 50, 12000, 4, "philox", False),   # counter rows in HBM
    (400, 300, 6, 5, 3000, 12, "mt19937-compat", True),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d+%d_%s%s" % (s[2], s[3], s[6], "_empty" if s[7] else ""))
def test_mode_samples_equal_the_model(shape):
    na, nb, ka, kb, edges, chains, rng, empty = shape
    lab = syn.contiguous_labels(na, nb, ka, kb)
    if empty:  # the last block of each type holds no node
        lab = np.where(lab == ka - 1, ka - 2, np.where(lab == ka + kb - 1, ka + kb - 2, lab)).astype(np.uint32)
    m = _model(na, nb, ka, kb, edges, chains, rng=rng, labels=lab)
    if empty:
        m.init_bisbm()
    else:
        m.shuffle_bisbm()
    m.run_sweeps(2)
    _check_samples(m, _assignment(chains))


# ---------------------------------------------------------------------------------------------------- 3. edges of the index arithmetic
def test_fewer_nodes_than_one_workgroup():
    rowptr, col, na, nb = O.load_graph("southernWomen")
    assert (na, nb) == (18, 14)
    m = B.BlockModel(O.contiguous_labels(na, nb, 2, 2), syn.types_vector(na, nb), 4, 2, 2, 1.0, (rowptr, col), n_chains=6, seed=3)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    _check_samples(m, [0, 1, 1, 0, 1, 0], samples=2)


def test_node_count_no_multiple_of_the_tiles():
    m = _model(1025, 260, 5, 3, 6000, 6)
    m.shuffle_bisbm()
    m.run_sweeps(1)
    _check_samples(m, [1, 0, NONE, 1, 0, 1], samples=2)


def test_modes_longer_than_a_permutation_chunk():
    m = _model(300, 200, 4, 4, 3000, 130)
    m.shuffle_bisbm()
    m.run_sweeps(1)
    moc = [0] * 130  # 70 / 59 / 1 chains, interleaved
    for c in range(1, 118, 2):
        moc[c] = 1
    moc[129] = 2
    assert [moc.count(g) for g in range(3)] == [70, 59, 1]
    _check_samples(m, moc, samples=2)


# ---------------------------------------------------------------------------------------------------- 4. chains untouched
def _state(m):
    out = [_all_labels(m), m.get_entropy()]
    for c in range(m.n_chains):
        out += [m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c)]
    return out


@pytest.mark.parametrize("rng", ["philox", "mt19937-compat"])
def test_mode_sampling_leaves_the_chains_untouched(rng):
    runs = []
    for per_mode in (False, True):
        m = _model(300, 200, 5, 4, 3000, 6, rng=rng)
        m.shuffle_bisbm()
        if per_mode:
            m.marginals_set_modes([0, 1, NONE, 1, 0, 0])
        rates = []
        for _ in range(3):
            rates.append(m.run_sweeps(1))
            m.marginals_accumulate()
        runs.append((_state(m), np.array(rates)))
    (s0, r0), (s1, r1) = runs
    assert (r0 == r1).all()
    for x, y in zip(s0, s1):
        assert (x == y).all()


# ---------------------------------------------------------------------------------------------------- 5. several device entries
def test_two_device_entries_equal_one_handle():
    moc = [0, 0, 1, 1, NONE, 0, 0, 2, 2, 2]  # entries hold chains 0-4 and 5-9: mode 0 spans both, mode 2 lives on the second

    def run(devices):
        m = _model(500, 400, 6, 5, 5000, 10, devices=devices)
        m.shuffle_bisbm()
        m.run_sweeps(2)
        m.marginals_set_modes(moc)
        for _ in range(2):
            m.marginals_accumulate()
            m.run_sweeps(1)
        state = m.marginals_modes()
        out = [state["terms"], state["ref_chain"]]
        for g in range(3):
            labels, top = m.marginals_map(mode=g, return_top=True)
            out += [m.marginals_get(mode=g), labels, top, m.marginals_reference(mode=g)[0]]
        out += [m.marginals_alignment(c)[0] for c in range(10) if moc[c] != NONE]
        out += [np.array([m.marginals_alignment(c)[1] for c in range(10) if moc[c] != NONE])]
        return out
    one, two = run(None), run([0, 0])
    assert len(one) == len(two)
    for x, y in zip(one, two):
        assert (np.asarray(x) == np.asarray(y)).all()
    assert one[1][2] >= 5 and one[0].tolist() == [8, 4, 6]


# ---------------------------------------------------------------------------------------------------- 6. refusals and state rules
def _refused(code, text, call, *args, **kw):
    with pytest.raises(B.BisbmError) as e:
        call(*args, **kw)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_refusals_and_state_rules():
    STATE, INVALID, UNSUPPORTED = B.BISBM_ERR_STATE, B.BISBM_ERR_INVALID_ARG, B.BISBM_ERR_UNSUPPORTED
    m = _model(300, 200, 4, 4, 3000, 4)
    m.shuffle_bisbm()
    assert m.marginals_modes()["n_modes"] == 0
    # the assignment itself
    _refused(INVALID, "chain 2", m.marginals_set_modes, [0, 1, 5, 1], n_modes=2)
    _refused(INVALID, "mode 1 has no chain", m.marginals_set_modes, [0, 2, 0, NONE], n_modes=3)
    _refused(STATE, "no modes are set", m.marginals_get, mode=0)
    # a change while the histogram holds samples, in both directions
    m.marginals_accumulate()
    _refused(STATE, "bisbm_marginals_reset first", m.marginals_set_modes, [0, 1, 0, 1])
    m.marginals_reset()
    m.marginals_set_modes([0, 1, 0, NONE])
    _refused(STATE, "no sample", m.marginals_map, mode=0)
    _refused(INVALID, "mode 2 out of range", m.marginals_get, mode=2)
    m.marginals_accumulate()
    _refused(STATE, "bisbm_marginals_reset first", m.marginals_set_modes, None)
    _refused(STATE, "bisbm_marginals_reset first", m.marginals_set_modes, [0, 1, 1, 0])
    # the pooled calls name the per-mode call
    _refused(STATE, "bisbm_marginals_get_mode", m.marginals_get)
    _refused(STATE, "bisbm_marginals_map_mode", m.marginals_map)
    _refused(STATE, "bisbm_marginals_set_mode_reference", m.marginals_set_reference, m.get_memberships(0))
    _refused(STATE, "bisbm_marginals_get_mode_reference", m.marginals_reference)
    _refused(STATE, "not counted", m.marginals_alignment, 3)
    # a caller's device buffer
    import torch
    dc = torch.zeros((500, 4), dtype=torch.int32, device=m.counts_device())
    torch.cuda.synchronize()
    _refused(UNSUPPORTED, "device_counts must be NULL", m.marginals_accumulate, dc.data_ptr())
    # the alignment mode is neither consulted nor changed
    assert m.alignment == B.ALIGN_NONE
    # reset: histograms and terms are zeroed, library-chosen references dropped, the assignment and a caller's reference stay
    assert m.marginals_modes()["terms"].tolist() == [2, 1] and min(m.marginals_modes()["ref_chain"]) >= 0
    m.marginals_reset()
    mine = m.get_memberships(3)
    m.marginals_set_reference(mine, mode=1)
    bad = mine.copy()
    bad[0] = 5
    _refused(INVALID, "outside its type", m.marginals_set_reference, bad, mode=0)
    state = m.marginals_modes()
    assert state["terms"].tolist() == [0, 0] and state["ref_chain"].tolist() == [-2, -1] and state["mode_of_chain"].tolist() == [0, 1, 0, NONE]
    assert not m.marginals_get(mode=0).any() and not m.marginals_get(mode=1).any()
    _refused(STATE, "no reference", m.marginals_reference, mode=0)
    m.marginals_accumulate()
    m.marginals_reset()
    state = m.marginals_modes()
    assert state["ref_chain"].tolist() == [-2, -1] and (m.marginals_reference(mode=1)[0] == mine).all()
    # a caller's reference per mode is what the mode is counted through
    labs = _all_labels(m)
    m.marginals_accumulate()
    ref0, chain0 = m.marginals_reference(mode=0)
    assert chain0 in (0, 2)
    counts, perms, totals = mode_sample(labs, [0, 1, 0, -1], [ref0, mine], 300, 4, 4)
    for g in range(2):
        assert (m.marginals_get(mode=g).astype(np.int64) == counts[g]).all()
    assert (m.marginals_alignment(1)[0] == perms[1]).all() and m.marginals_alignment(1)[1] == totals[1]
    # a merge that changes the block counts: a caller's stale reference is refused, then a fresh start
    m.agg_merge(1, 1, 5)
    _refused(STATE, "set it again", m.marginals_accumulate)
    m.marginals_set_reference(None, mode=1)
    labs, S = _all_labels(m), m.entropy()
    m.marginals_accumulate()
    state = m.marginals_modes()
    assert state["terms"].tolist() == [2, 1] and state["ref_chain"].tolist() == [int(np.argmin(S[[0, 2]])) * 2, 1]
    counts, _, _ = mode_sample(labs, [0, 1, 0, -1], [labs[state["ref_chain"][0]], labs[1]], 300, 3, 3)
    for g in range(2):
        assert m.marginals_get(mode=g).shape == (500, 3) and (m.marginals_get(mode=g).astype(np.int64) == counts[g]).all()
    # off again: the pooled histogram serves as before
    m.marginals_reset()
    m.marginals_set_modes(None)
    m.marginals_accumulate()
    assert m.marginals_get().sum() == 4 * 500 and m.marginals_modes()["n_modes"] == 0
    m.close()
    # replica exchange, in both orders
    t = _model(300, 200, 4, 4, 3000, 4)
    t.shuffle_bisbm()
    t.set_tempering([1.0, 2.0])
    _refused(STATE, "replica exchange is on", t.marginals_set_modes, [0, 1, 0, 1])
    t.set_tempering(None)
    t.marginals_set_modes([0, 1, 0, 1])
    _refused(STATE, "mode-resolved marginals are set", t.set_tempering, [1.0, 2.0])
    t.close()
    # a wide handle: refused at the sample
    w = _model(400, 300, 200, 100, 4000, 2)
    w.shuffle_bisbm()
    w.marginals_set_modes([0, 1])
    _refused(UNSUPPORTED, "byte labels", w.marginals_accumulate)
    w.close()
    # chains grouped by shape: at set_modes, and at the sample when the grouping came afterwards
    rowptr, col, na, nb = O.load_graph("n_1000")
    for modes_first in (False, True):
        g = B.BlockModel(O.contiguous_labels(na, nb, 6, 6), syn.types_vector(na, nb), 12, 6, 6, 1.0, (rowptr, col), n_chains=32, seed=4)
        g.shuffle_bisbm()
        g.run_sweeps(2)
        if modes_first:
            g.marginals_set_modes([c % 2 for c in range(32)])
        for _ in range(4):
            if g.mixed_shapes:
                break
            g.agg_merge(2, None, 10)
        assert g.mixed_shapes
        if modes_first:
            _refused(STATE, "block counts", g.marginals_accumulate)
        else:
            _refused(STATE, "grouped by shape", g.marginals_set_modes, [c % 2 for c in range(32)])
        g.close()


# ---------------------------------------------------------------------------------------------------- 7. the Python driver
def test_marginalize_modes_equals_the_hand_written_loop():
    moc = [0, 1, 0, 1, NONE, 1, 0, 0]

    def model():
        m = _model(300, 200, 4, 4, 3000, 8)
        m.shuffle_bisbm()
        return m
    m = model()
    out = B.marginalize_modes(m, 2, 3, 1, mode_of_chain=moc)
    h = model()
    h.run_sweeps(2)
    h.marginals_reset()
    h.marginals_set_modes(moc)
    for _ in range(3):
        h.run_sweeps(1)
        h.marginals_accumulate()
    state = h.marginals_modes()
    assert out["moved"] == 0 and (out["modes"] == np.array(moc, dtype=np.uint32)).all()
    assert out["counts"].shape == (2, 500, 4) and out["labels"].shape == out["top"].shape == (2, 500)
    assert out["terms"].tolist() == state["terms"].tolist() == [12, 9]
    assert out["weights"].tolist() == [4 / 7, 3 / 7] and out["ref_chain"].tolist() == state["ref_chain"].tolist()
    for g in range(2):
        labels, top = h.marginals_map(mode=g, return_top=True)
        assert (out["counts"][g] == h.marginals_get(mode=g)).all() and (out["labels"][g] == labels).all() and (out["top"][g] == top).all()
    # with a threshold the grouping is taken after the burn-in; the two planted modes stay apart while they are sampled
    t = TWO_MODES
    P, Q, starts = two_mode_pool()
    m = _model(t["na"], t["nb"], t["ka"], t["kb"], 3000, t["chains"])
    for c, start in enumerate(starts):
        m.set_memberships(start, chain=c)
    m.init_bisbm()
    out = B.marginalize_modes(m, 0, 1, 0, threshold=1.5)
    assert out["modes"]["mode"].tolist() == [0, 1] * 8 and out["moved"] == 0 and out["terms"].tolist() == [8, 8]
    assert agreement(out["labels"][0], P, t["na"], t["ka"], t["kb"]) == 1.0 and agreement(out["labels"][1], Q, t["na"], t["ka"], t["kb"]) == 1.0


# ---------------------------------------------------------------------------------------------------- 8. the CLI
def test_cli_mode_marginals_print_what_the_driver_computes(tmp_path):
    p = PLANTED
    a, b, truth = planted_graph()
    n = p["na"] + p["nb"]
    el = tmp_path / "planted.edgelist"
    np.savetxt(el, np.stack([a, b], axis=1), fmt="%d")
    sizes = np.bincount(truth)
    threshold = 0.5
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    r = subprocess.run([cli, "-e", str(el), "-y", str(p["na"]), str(p["nb"]), "-n", *map(str, sizes), "-z", str(p["ka"]), str(p["kb"]),
                        "-E", "1", "-d", "5", "--rng", "philox", "--chains", "16", "--randomize", "-b", str(10 * n), "-t", str(4 * n),
                        "-f", str(n), "--marginalize", "--modes", str(tmp_path / "modes.txt"), str(threshold), "--mode_marginals",
                        str(tmp_path / "mm")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    ea, eb = B.load_edge_list(str(el))
    rp, cl = B.edge_to_adj((ea, eb), n)
    m = B.BlockModel(truth, syn.types_vector(p["na"], p["nb"]), p["ka"] + p["kb"], p["ka"], p["kb"], 1.0, (rp, cl), n_chains=16, seed=5,
                     gen_seed=6)
    m.shuffle_bisbm()
    out = B.marginalize_modes(m, 10, 4, 1, threshold=threshold)
    M = len(out["terms"])
    heaviest = int(np.argmax(out["weights"]))  # (ties -> the lowest mode)
    assert r.stdout.split() == [str(x) for x in out["labels"][heaviest]]
    assert "mode_marginals: %d mode(s)" % M in r.stderr
    for g in range(M):
        got = np.loadtxt(tmp_path / ("mm.%d.txt" % g), dtype=np.int64).reshape(n, 2)
        assert (got[:, 0] == out["labels"][g]).all() and (got[:, 1] == out["top"][g]).all()
        assert "mode %d: share %g, reference chain %d, %d term(s)" % (g, out["weights"][g], out["ref_chain"][g], out["terms"][g]) in r.stderr
    assert not os.path.exists(tmp_path / ("mm.%d.txt" % M)) and "modes: " in r.stderr
