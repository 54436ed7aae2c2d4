"""GPU tests of label alignment before pooling (include/bisbm.h, "Label alignment before pooling"): recovery of a planted
partition from chains in different numberings, exactness of the overlap / assignment / aligned-histogram kernels against the
numpy model of tests/test_align.py, chains left untouched, several devices, the refusals and the CLI."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib as O
from test_align import PLANTED, agreement, aligned_sample, planted_graph, relabelled_planted_starts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu


def _model(na, nb, ka, kb, edges, chains, rng="philox", seed=9, graph_seed=4, labels=None, **kw):
    a, b = syn.planted_edges(na, nb, edges, ka, kb, seed=graph_seed)
    rp, cl = B.edge_to_adj((a, b), na + nb)
    lab = syn.contiguous_labels(na, nb, ka, kb) if labels is None else labels
    return B.BlockModel(lab, syn.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rp, cl), n_chains=chains, rng=rng, seed=seed,
                        gen_seed=seed + 1, **kw)


def _all_labels(m):
    return np.array([m.get_memberships(c) for c in range(m.n_chains)])


def test_aligned_marginals_recover_the_planted_partition():
    p = PLANTED
    a, b, truth = planted_graph()
    n, na = p["na"] + p["nb"], p["na"]
    rp, cl = B.edge_to_adj((a, b), n)
    m = B.BlockModel(truth, syn.types_vector(na, p["nb"]), p["ka"] + p["kb"], p["ka"], p["kb"], 1.0, (rp, cl), n_chains=64, seed=5)
    for c, start in enumerate(relabelled_planted_starts(truth, na, p["ka"], p["kb"], 64)):
        m.set_memberships(start, chain=c)
    m.init_bisbm()
    m.run_sweeps(5)
    S = m.entropy()
    labels, counts = B.marginalize(m, 0, 4, 1, align=True)
    ref, ref_chain = m.marginals_reference()
    assert ref_chain == int(np.argmin(S))
    assert agreement(labels, truth, na, p["ka"], p["kb"]) >= 0.95
    assert (counts.max(axis=1) / counts.sum(axis=1)).mean() >= 0.95
    # the same chains pooled without alignment: the histogram is spread over the chains' numberings
    m2 = B.BlockModel(truth, syn.types_vector(na, p["nb"]), p["ka"] + p["kb"], p["ka"], p["kb"], 1.0, (rp, cl), n_chains=64, seed=5)
    for c, start in enumerate(relabelled_planted_starts(truth, na, p["ka"], p["kb"], 64)):
        m2.set_memberships(start, chain=c)
    m2.init_bisbm()
    m2.run_sweeps(5)
    _, raw = B.marginalize(m2, 0, 4, 1)
    assert (raw.max(axis=1) / raw.sum(axis=1)).mean() <= 0.6


SHAPES = [  # na, nb, ka, kb, edges, chains, rng, empty_block
    (300, 200, 4, 4, 3000, 16, "philox", False),
    (300, 200, 7, 3, 3000, 8, "mt19937-compat", False),
    (900, 700, 60, 40, 20000, 6, "philox", False),   # one LDS table per workgroup
    (800, 800, 100, 100, 20000, 5, "philox", False),  # tables counted in HBM
    (600, 300, 200, 50, 12000, 4, "philox", False),
    (400, 300, 6, 5, 3000, 12, "mt19937-compat", True),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d+%d_%s%s" % (s[2], s[3], s[6], "_empty" if s[7] else ""))
def test_aligned_sample_equals_the_model(shape):
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
    m.marginals_reset()
    m.marginals_set_alignment(B.ALIGN_REFERENCE)
    want = np.zeros((na + nb, max(ka, kb)), dtype=np.int64)
    S0 = m.entropy()
    ref = None
    for sample in range(3):
        labs = _all_labels(m)
        m.marginals_accumulate()
        if ref is None:
            ref, chain = m.marginals_reference()
            assert chain == int(np.argmin(S0)) and (ref == labs[chain]).all()
        counts, perms, totals = aligned_sample(labs, ref, na, ka, kb)
        want += counts
        for c in range(chains):
            perm, tot = m.marginals_alignment(c)
            assert (perm == perms[c]).all() and tot == totals[c], (sample, c)
        assert (m.marginals_get().astype(np.int64) == want).all()
        m.run_sweeps(1)
    # a caller's device buffer gets the same aligned sample
    dc = torch.zeros((na + nb, max(ka, kb)), dtype=torch.int32, device=m.counts_device())
    torch.cuda.synchronize()
    labs = _all_labels(m)
    m.marginals_accumulate(dc.data_ptr())
    assert (dc.cpu().numpy().astype(np.int64) == aligned_sample(labs, ref, na, ka, kb)[0]).all()
    # a caller's reference
    m.marginals_set_reference(labs[chains - 1])
    m.marginals_accumulate(dc.data_ptr())
    assert m.marginals_reference()[1] == -1
    perm, tot = m.marginals_alignment(chains - 1)
    assert (perm == np.arange(ka + kb)).all() and tot == na + nb


def _pooled_sample_equals_the_model(m, na, ka, kb):
    m.shuffle_bisbm()
    m.run_sweeps(2)
    m.marginals_reset()
    m.marginals_set_alignment(True)
    labs = _all_labels(m)
    m.marginals_accumulate()
    ref, chain = m.marginals_reference()
    assert chain == int(np.argmin(m.entropy())) and (ref == labs[chain]).all()
    counts, perms, totals = aligned_sample(labs, ref, na, ka, kb)
    assert (m.marginals_get().astype(np.int64) == counts).all()
    for c in range(m.n_chains):
        perm, tot = m.marginals_alignment(c)
        assert (perm == perms[c]).all() and tot == totals[c], c


# The pooled sample is one mode that holds every chain: it runs the staging of a mode's permutation rows in chunks of 64 list
# positions and the grid over 256-node workgroups at these edges.
@pytest.mark.parametrize("shape", [
    (300, 200, 4, 4, 3000, 130),   # three staging chunks, the last with 2 chains
    (1025, 260, 5, 3, 6000, 6),    # the node count is no multiple of 256 or of 1024
], ids=["130_chains", "1285_nodes"])
def test_pooled_sample_at_the_chunk_and_workgroup_edges(shape):
    na, nb, ka, kb, edges, chains = shape
    m = _model(na, nb, ka, kb, edges, chains)
    _pooled_sample_equals_the_model(m, na, ka, kb)
    m.close()


def test_pooled_sample_of_fewer_nodes_than_a_workgroup():
    rowptr, col, na, nb = O.load_graph("southernWomen")
    assert (na, nb) == (18, 14)
    m = B.BlockModel(O.contiguous_labels(na, nb, 2, 2), syn.types_vector(na, nb), 4, 2, 2, 1.0, (rowptr, col), n_chains=6, seed=3)
    _pooled_sample_equals_the_model(m, na, 2, 2)
    m.close()


def test_pooled_sample_equals_one_mode_of_every_chain():
    chains = 12
    m = _model(300, 200, 6, 5, 3000, chains)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    m.marginals_reset()
    m.marginals_set_alignment(True)
    m.marginals_accumulate()
    ref, _ = m.marginals_reference()
    pooled = m.marginals_get(), [m.marginals_alignment(c) for c in range(chains)], m.marginals_map()
    assert pooled[0].sum() == chains * 500
    m.marginals_reset()
    m.marginals_set_modes(np.zeros(chains, dtype=np.uint32))
    m.marginals_set_reference(ref, mode=0)
    m.marginals_accumulate()
    assert (m.marginals_get(mode=0) == pooled[0]).all()
    for c in range(chains):
        perm, tot = m.marginals_alignment(c)
        assert (perm == pooled[1][c][0]).all() and tot == pooled[1][c][1], c
    assert (m.marginals_map(mode=0) == pooled[2]).all()
    m.close()


def _state(m):
    out = [_all_labels(m), m.get_entropy()]
    for c in range(m.n_chains):
        out += [m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c)]
    return out


@pytest.mark.parametrize("rng", ["philox", "mt19937-compat"])
def test_alignment_leaves_the_chains_untouched(rng):
    runs = []
    for align in (False, True):
        m = _model(300, 200, 5, 4, 3000, 6, rng=rng)
        m.shuffle_bisbm()
        m.marginals_set_alignment(align)
        rates = []
        for _ in range(3):
            rates.append(m.run_sweeps(1))
            m.marginals_accumulate()
        runs.append((_state(m), np.array(rates)))
    (s0, r0), (s1, r1) = runs
    assert (r0 == r1).all()
    for x, y in zip(s0, s1):
        assert (x == y).all()


def test_two_device_entries_equal_one_handle():
    def run(devices):
        m = _model(500, 400, 6, 5, 5000, 10, devices=devices)
        m.shuffle_bisbm()
        m.run_sweeps(2)
        m.marginals_set_alignment(True)
        for _ in range(2):
            m.marginals_accumulate()
            m.run_sweeps(1)
        ref, chain = m.marginals_reference()
        return m.marginals_get(), m.marginals_map(), ref, chain, [m.marginals_alignment(c)[0] for c in range(10)]
    one, two = run(None), run([0, 0])
    for x, y in zip(one[:3], two[:3]):
        assert (x == y).all()
    assert one[3] == two[3]
    assert all((x == y).all() for x, y in zip(one[4], two[4]))


def test_refusals():
    # wide mode: two-byte labels
    m = _model(400, 300, 200, 100, 4000, 2)
    m.shuffle_bisbm()
    m.marginals_set_alignment(True)
    with pytest.raises(B.BisbmError) as e:
        m.marginals_accumulate()
    assert e.value.code == B.BISBM_ERR_UNSUPPORTED and "byte labels" in str(e.value)
    # a mode change while the histogram holds samples
    m = _model(300, 200, 4, 4, 3000, 4)
    m.shuffle_bisbm()
    m.marginals_accumulate()
    with pytest.raises(B.BisbmError) as e:
        m.marginals_set_alignment(True)
    assert e.value.code == B.BISBM_ERR_STATE and "holds samples" in str(e.value)
    m.marginals_reset()
    m.marginals_set_alignment(True)
    # a reference label outside its type's blocks
    bad = syn.contiguous_labels(300, 200, 4, 4)
    bad[0] = 5
    with pytest.raises(B.BisbmError) as e:
        m.marginals_set_reference(bad)
    assert e.value.code == B.BISBM_ERR_INVALID_ARG and "outside its type" in str(e.value)
    with pytest.raises(B.BisbmError) as e:
        m.marginals_reference()
    assert e.value.code == B.BISBM_ERR_STATE
    # a caller's reference made stale by a merge
    m.marginals_set_reference(m.get_memberships(1))
    m.marginals_accumulate()
    m.agg_merge(1, 1, 5)
    with pytest.raises(B.BisbmError) as e:
        m.marginals_accumulate()
    assert e.value.code == B.BISBM_ERR_STATE and "set it again" in str(e.value)
    # ... while a library-chosen one is taken afresh
    m.marginals_set_reference(None)
    m.marginals_accumulate()
    assert m.marginals_reference()[1] >= 0


def test_cli_marginalize_align_prints_what_the_driver_computes(tmp_path):
    p = PLANTED
    a, b, truth = planted_graph()
    n = p["na"] + p["nb"]
    el = tmp_path / "planted.edgelist"
    np.savetxt(el, np.stack([a, b], axis=1), fmt="%d")
    sizes = np.bincount(truth)
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    r = subprocess.run([cli, "-e", str(el), "-y", str(p["na"]), str(p["nb"]), "-n", *map(str, sizes), "-z", str(p["ka"]), str(p["kb"]),
                        "-E", "1", "-d", "5", "--rng", "philox", "--chains", "64", "--randomize", "-b", str(10 * n), "-t", str(4 * n),
                        "-f", str(n), "--marginalize", "--align"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    ea, eb = B.load_edge_list(str(el))
    rp, cl = B.edge_to_adj((ea, eb), n)
    m = B.BlockModel(truth, syn.types_vector(p["na"], p["nb"]), p["ka"] + p["kb"], p["ka"], p["kb"], 1.0, (rp, cl), n_chains=64, seed=5,
                     gen_seed=6)
    m.shuffle_bisbm()
    labels, _ = B.marginalize(m, 10, 4, 1, align=True)
    assert r.stdout.split() == [str(x) for x in labels]
    assert "align: labels matched to chain %d" % m.marginals_reference()[1] in r.stderr
