"""CPU tests of label alignment before pooling (include/bisbm.h, "Label alignment before pooling"): the host assignment solver
against SciPy and a restatement of its tie rule, the numpy model of an aligned sample (what the GPU tests compare the device
with) on oracle chains of a planted graph, the reference choice over two gloo ranks, and the CLI's --align refusal."""
import importlib
import os
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from scipy.optimize import linear_sum_assignment

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

KS = (1, 2, 3, 7, 32, 64, 100, 255)


# ---------------------------------------------------------------------------------------------------- the model
def overlap_tables(labels, ref, na, ka, kb):
    """(C_a [ka, ka], C_b [kb, kb]) of one chain: C[r][s] = nodes of the type with the chain's label r and reference label s."""
    labels = np.asarray(labels, dtype=np.int64)
    ref = np.asarray(ref, dtype=np.int64)
    ca = np.bincount(labels[:na] * ka + ref[:na], minlength=ka * ka).reshape(ka, ka)
    cb = np.bincount((labels[na:] - ka) * kb + ref[na:] - ka, minlength=kb * kb).reshape(kb, kb)
    return ca.astype(np.uint32), cb.astype(np.uint32)


def aligned_sample(labels_by_chain, ref, na, ka, kb):
    """One aligned sample of every chain: (counts [n, max(ka, kb)], perms [chains, ka + kb] in global-label form, overlap
    totals [chains]), with the library's host solver."""
    labels_by_chain = np.asarray(labels_by_chain, dtype=np.int64)
    n = labels_by_chain.shape[1]
    base = np.where(np.arange(n) >= na, ka, 0)
    counts = np.zeros((n, max(ka, kb)), dtype=np.int64)
    perms, totals = [], []
    for lab in labels_by_chain:
        ca, cb = overlap_tables(lab, ref, na, ka, kb)
        pa, ta = B.align_assignment(ca)
        pb, tb = B.align_assignment(cb)
        perm = np.concatenate([pa, ka + pb]).astype(np.int64)
        np.add.at(counts, (np.arange(n), perm[lab] - base), 1)
        perms.append(perm)
        totals.append(ta + tb)
    return counts, np.array(perms, dtype=np.uint32), np.array(totals, dtype=np.uint64)


def agreement(labels, truth, na, ka, kb):
    """Share of nodes whose label equals the truth after the best relabelling of each type."""
    n = len(truth)
    hit = 0
    for lo, hi, base, k in ((0, na, 0, ka), (na, n, ka, kb)):
        conf = np.zeros((k, k), dtype=np.int64)
        np.add.at(conf, (np.asarray(labels[lo:hi], dtype=np.int64) - base, np.asarray(truth[lo:hi], dtype=np.int64) - base), 1)
        r, c = linear_sum_assignment(conf, maximize=True)
        hit += conf[r, c].sum()
    return hit / n


def relabelled_planted_starts(truth, na, ka, kb, chains, noise=0.2, seed=100):
    """Per chain: the planted partition in a random numbering of each type, with `noise` of the labels redrawn.  (Chains
    from shuffle_bisbm at T = 1 on this graph settle in a metastable state with one block emptied, about 5 % above the
    planted description length, in every chain tried: the recovery checks start next to the answer and let every chain pick
    its own numbering.)"""
    n = len(truth)
    node = np.arange(n)
    out = []
    for c in range(chains):
        st = np.random.default_rng(seed + c)
        perm = np.concatenate([st.permutation(ka), ka + st.permutation(kb)])
        lab = perm[truth]
        rnd = np.where(node < na, st.integers(0, ka, n), ka + st.integers(0, kb, n))
        out.append(np.where(st.random(n) < noise, rnd, lab).astype(np.uint32))
    return out


PLANTED = dict(na=2000, nb=2000, ka=4, kb=4, edges=40000, p_in=0.9, seed=3)


def planted_graph():
    p = PLANTED
    a, b = syn.planted_edges(p["na"], p["nb"], p["edges"], p["ka"], p["kb"], seed=p["seed"], p_in=p["p_in"])
    truth = syn.contiguous_labels(p["na"], p["nb"], p["ka"], p["kb"])
    return a, b, truth


# ---------------------------------------------------------------------------------------------------- the solver
def _tables(kind, k, rs):
    if kind == "random":
        return rs.integers(0, 1000, (k, k))
    if kind == "ties":
        return rs.integers(0, 3, (k, k))
    if kind == "empty":
        t = rs.integers(0, 50, (k, k))
        t[rs.random(k) < 0.3, :] = 0
        t[:, rs.random(k) < 0.3] = 0
        return t
    if kind == "permutation":
        t = np.zeros((k, k), dtype=np.int64)
        t[np.arange(k), rs.permutation(k)] = rs.integers(1, 10_000, k)
        return t
    if kind == "diagonal":
        t = rs.integers(0, 20, (k, k))
        t[np.arange(k), np.arange(k)] += rs.integers(100, 2000, k)
        return t[rs.permutation(k)]
    raise ValueError(kind)


@pytest.mark.parametrize("k", KS)
def test_assignment_is_optimal_and_a_bijection(k):
    rs = np.random.default_rng(k)
    per_kind = 12 if k >= 100 else 80
    for kind in ("random", "ties", "empty", "permutation", "diagonal"):
        for _ in range(per_kind):
            t = _tables(kind, k, rs).astype(np.uint32)
            perm, total = B.align_assignment(t)
            assert perm.dtype == np.uint32 and sorted(perm.tolist()) == list(range(k))
            r, c = linear_sum_assignment(t.astype(np.int64), maximize=True)
            assert total == int(t[r, c].astype(np.int64).sum()) == int(t[np.arange(k), perm].astype(np.int64).sum()), kind
            if kind == "permutation":
                assert (t[np.arange(k), perm] > 0).all()  # the planted permutation comes back exactly
            p2, t2 = B.align_assignment(t)
            assert (p2 == perm).all() and t2 == total


def _restated(table):
    """The definition of include/bisbm.h in plain Python: cost max(C) - C, rows inserted 0..K-1, Dijkstra steps over the
    unvisited columns taking the least reduced distance, ties to the lowest column."""
    k = len(table)
    cmax = max(max(r) for r in table)
    cost = [[cmax - int(x) for x in row] for row in table]
    inf = float("inf")
    u, v, p, way = [0] * (k + 1), [0] * (k + 1), [0] * (k + 1), [0] * (k + 1)
    for i in range(1, k + 1):
        p[0], j0 = i, 0
        minv, used = [inf] * (k + 1), [False] * (k + 1)
        while True:
            used[j0] = True
            i0, delta, j1 = p[j0], inf, None
            for j in range(1, k + 1):
                if not used[j]:
                    cur = cost[i0 - 1][j - 1] - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if minv[j] < delta:
                        delta, j1 = minv[j], j
            for j in range(k + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    perm = [0] * k
    for j in range(1, k + 1):
        perm[p[j] - 1] = j - 1
    return perm


def test_tie_rule_matches_the_restated_definition():
    rs = np.random.default_rng(7)
    cases = [np.zeros((5, 5), dtype=np.uint32), np.ones((4, 4), dtype=np.uint32), np.eye(6, dtype=np.uint32)[::-1].copy()]
    for k in (2, 3, 5, 7, 12, 20):
        for _ in range(30):
            cases.append(rs.integers(0, 2, (k, k)).astype(np.uint32))
            cases.append(_tables("empty", k, rs).clip(0, 2).astype(np.uint32))
    for t in cases:
        perm, _ = B.align_assignment(t)
        assert perm.tolist() == _restated(t.tolist()), t
    # all-equal tables: every permutation is optimal; the tie rule makes it the identity
    assert B.align_assignment(np.full((9, 9), 4, dtype=np.uint32))[0].tolist() == list(range(9))


def test_assignment_refuses_bad_arguments():
    L = B.lib()
    out = np.zeros(1, dtype=np.uint32)
    t = np.zeros(1, dtype=np.uint32)
    assert L.bisbm_align_assignment(0, B._p(t, B._u32p), B._p(out, B._u32p), None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_align_assignment(1, None, B._p(out, B._u32p), None) == B.BISBM_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        B.align_assignment(np.zeros((2, 3)))


# ---------------------------------------------------------------------------------------------------- the model on oracle chains
def test_model_of_an_aligned_sample_recovers_the_planted_partition():
    """64 oracle chains (Philox mode) of the planted 2000 + 2000 graph, each in its own numbering: the aligned MAP is the planted
    partition, the raw pooled histogram is spread over the numberings.  These are the thresholds the GPU recovery test uses."""
    p = PLANTED
    a, b, truth = planted_graph()
    n, na = p["na"] + p["nb"], p["na"]
    rowptr, col = O.edge_to_csr(a, b, n)
    labs, S = [], []
    for c, start in enumerate(relabelled_planted_starts(truth, na, p["ka"], p["kb"], 64)):
        o = O.OracleModel(rowptr, col, na, p["nb"], p["ka"], p["kb"], 1.0, start)
        o.seed_philox(5, c)
        o.init_bisbm()
        o.anneal("constant", [1.0], 5 * n, 1 << 60)
        labs.append(o.memberships())
        S.append(o.entropy())
    labs = np.array(labs)
    ref = labs[int(np.argmin(S))]
    counts, perms, totals = aligned_sample(labs, ref, na, p["ka"], p["kb"])
    base = np.where(np.arange(n) >= na, p["ka"], 0)
    assert counts.sum() == 64 * n and (counts.sum(axis=1) == 64).all()
    assert agreement(counts.argmax(axis=1) + base, truth, na, p["ka"], p["kb"]) >= 0.95
    assert (counts.max(axis=1) / 64).mean() >= 0.95
    raw = D.numpy_marginals(labs, na, p["ka"], p["kb"])
    assert (raw.max(axis=1) / 64).mean() <= 0.6
    # the reference chain aligns onto itself with the identity, overlap n
    best = int(np.argmin(S))
    assert (perms[best] == np.arange(p["ka"] + p["kb"])).all() and totals[best] == n
    # a chain's permutation maps its labels onto the reference numbering
    for c in range(0, 64, 9):
        assert agreement(perms[c][labs[c]], ref, na, p["ka"], p["kb"]) == pytest.approx((perms[c][labs[c]] == ref).mean())


# ---------------------------------------------------------------------------------------------------- two ranks
TOTAL_CHAINS = 7


class _StandIn:
    """What marginalize() needs of a BlockModel, on the host: fixed per-chain description lengths (with a tie) and labels."""

    def __init__(self, shard, n=12, na=5, ka=2, kb=3):
        self.n, self.na, self.KA, self.KB = n, na, ka, kb
        self.kmax = max(ka, kb)
        self.shard = shard
        S = np.array([5.0, 3.0, 4.0, 9.0, 3.0, 3.0, 8.0])  # global chains 1, 4, 5 tie at the lowest value
        self.S = S[shard.first_chain_id: shard.first_chain_id + shard.n_local]
        self.references, self.modes = [], []

    def labels(self, gid):
        rs = np.random.default_rng(gid)
        return np.concatenate([rs.integers(0, self.KA, self.na), self.KA + rs.integers(0, self.KB, self.n - self.na)]).astype(np.uint32)

    def entropy(self):
        return self.S.copy()

    def get_memberships(self, chain=0):
        return self.labels(self.shard.first_chain_id + chain)

    def run_sweeps(self, sweeps):
        pass

    def counts_device(self):
        return torch.device("cpu")

    def marginals_set_alignment(self, mode):
        self.modes.append(int(mode))

    def marginals_set_reference(self, labels=None):
        self.references.append(None if labels is None else np.asarray(labels).copy())

    def marginals_accumulate(self, ptr=None):
        pass


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _align_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        shard = D.ChainShard(TOTAL_CHAINS)
        model = _StandIn(shard)
        gid, lab = shard.lowest_chain_labels(model)
        B.marginalize(model, 0, 2, 1, shard=shard)  # align=False: neither the mode nor the reference is touched
        assert model.modes == [] and model.references == []
        labels, _ = B.marginalize(model, 0, 2, 1, shard=shard, align=True)
        assert model.modes == [1] and len(model.references) == 1 and labels.shape == (model.n,)
        np.save(os.path.join(out_dir, "ref%d.npy" % rank), np.concatenate([[gid], lab, model.references[0]]))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_world2_gloo_every_rank_gets_the_global_lowest_chain_as_reference(tmp_path):
    mp.spawn(_align_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "ref0.npy"), np.load(tmp_path / "ref1.npy")
    assert (r0 == r1).all()
    # chains 0..3 on rank 0, 4..6 on rank 1; the lowest description length is shared by chains 1, 4 and 5: chain 1 wins
    assert r0[0] == 1
    want = _StandIn(D.ChainShard(TOTAL_CHAINS, rank=0, world_size=1)).labels(1)
    n = len(want)
    assert (r0[1: 1 + n] == want).all() and (r0[1 + n:] == want).all()


# ---------------------------------------------------------------------------------------------------- CLI
def test_cli_align_needs_marginalize(tmp_path):
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    if not os.path.exists(cli):
        B.build(force=True)
    el = os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist")
    r = subprocess.run([cli, "-e", el, "-y", "18", "14", "-z", "2", "2", "-n", "9", "9", "7", "7", "--align"], capture_output=True, text=True)
    assert (r.returncode, r.stdout) == (1, "")
    assert r.stderr == "--align aligns the chains' block labels before pooling: it needs --marginalize.\n"
    r = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert "--align" in r.stderr
    # with --marginalize the run gets as far as the device (without one: bisbm_create's error; with one: the labels)
    r = subprocess.run([cli, "-e", el, "-y", "18", "14", "-z", "2", "2", "-n", "9", "9", "7", "7", "-d", "3", "--rng", "philox", "-b", "64",
                        "-t", "128", "-f", "32", "--chains", "4", "--marginalize", "--align"], capture_output=True, text=True)
    if r.returncode == 0:
        assert len(r.stdout.split()) == 32 and "align: labels matched to chain" in r.stderr
    else:
        assert r.returncode == 3 and "no hip device" in r.stderr.lower(), r.stderr
