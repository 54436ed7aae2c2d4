"""CPU checks of the pair scores (include/bisbm.h, "Posterior-predictive pair scores"): the numpy statement of the definition
(distributed.numpy_pair_scores, the reference of the GPU tests), the refusals of `mcmc --score_pairs` that need no device, and
the pooling over ranks at world size 2 over gloo."""
import importlib
import os
import socket
import subprocess

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")


def block_state(a, b, labels, K):
    """(m [K, K] symmetric, m_r [K], deg [n]) of a partition, as get_m / get_m_r return them."""
    a, b, labels = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    m = np.zeros((K, K), dtype=np.int32)
    np.add.at(m, (labels[a], labels[b]), 1)
    np.add.at(m, (labels[b], labels[a]), 1)
    deg = np.bincount(np.concatenate([a, b]), minlength=len(labels))
    return m, m.sum(axis=1).astype(np.int32), deg


def all_pairs(na, nb):
    u, v = np.meshgrid(np.arange(na), na + np.arange(nb), indexing="ij")
    return np.stack([u.ravel(), v.ravel()], axis=1)


def test_one_chain_scores_add_up_to_the_edge_count():
    """Over all na * nb pairs the terms of one chain add up to E: sum_uv d_u d_v m[b_u][b_v] / (m_r[b_u] m_r[b_v]) =
    sum_rs m_rs.  Every term carries at most two roundings (the product with m, the quotient; d_u d_v and m_r m_r are exact
    below 2^53) and numpy's sum over P terms at most P - 1 more, all terms non-negative: within P 2^-52 E."""
    na = nb = 600
    a, b = syn.planted_edges(na, nb, 6000, 8, 8, seed=4)
    labels = syn.contiguous_labels(na, nb, 8, 8)
    m, m_r, deg = block_state(a, b, labels, 16)
    pairs = all_pairs(na, nb)
    s = D.numpy_pair_scores([labels], [m], [m_r], deg, pairs)
    E, P = len(a), len(pairs)
    assert s.shape == (P,) and s.dtype == np.float64 and (s >= 0).all()
    assert abs(s.sum() - E) <= P * 2.0 ** -52 * E, (s.sum(), E)
    assert (s[(deg[pairs[:, 0]] == 0) | (deg[pairs[:, 1]] == 0)] == 0).all()
    # one term, spelled out
    i = int(np.argmax(s))
    u, v = pairs[i]
    assert s[i] == (float(deg[u]) * float(deg[v])) * float(m[labels[u], labels[v]]) / (float(m_r[labels[u]]) * float(m_r[labels[v]]))
    # two chains of different shapes, as a list: the sums add
    lab2 = syn.contiguous_labels(na, nb, 3, 5)
    m2, m_r2, _ = block_state(a, b, lab2, 8)
    both = D.numpy_pair_scores([labels, lab2], [m, m2], [m_r, m_r2], deg, pairs[:1000])
    assert (both == s[:1000] + D.numpy_pair_scores([lab2], [m2], [m_r2], deg, pairs[:1000])).all()


def test_zero_degree_nodes_score_zero_without_a_division():
    """Nodes 2 (type a) and 5 (type b) have no edge and sit alone in blocks of degree sum 0: their pairs score 0.0, not 0 / 0."""
    a, b = np.array([0, 0, 1]), np.array([3, 4, 4])
    labels = np.array([0, 0, 1, 2, 2, 3])
    m, m_r, deg = block_state(a, b, labels, 4)
    assert m_r[1] == 0 and m_r[3] == 0
    pairs = all_pairs(3, 3)
    with np.errstate(all="raise"):
        s = D.numpy_pair_scores([labels], [m], [m_r], deg, pairs)
    assert np.isfinite(s).all() and abs(s.sum() - 3) <= 9 * 2.0 ** -52 * 3
    for i, (u, v) in enumerate(pairs):
        assert (s[i] == 0) == (u == 2 or v == 5), (u, v, s[i])


def test_cli_refusals_need_no_device(tmp_path):
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    if not os.path.exists(cli):
        B.build(force=True)
    el = os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist")
    good, out = tmp_path / "pairs.txt", tmp_path / "scores.txt"
    good.write_text("0 18\n17 31\n")

    def run(*args):
        r = subprocess.run([cli, *args], capture_output=True, text=True)
        return r.returncode, r.stdout, r.stderr
    base = ("-e", el, "-y", "18", "14", "-n", "9", "9", "7", "7", "-z", "2", "2")
    rc, so, se = run(*base, "--score_pairs", str(good), str(out))
    assert rc == 1 and so == "" and "--marginalize" in se
    rc, so, se = run(*base, "--marginalize", "--score_pairs", str(good))
    assert rc == 1 and so == "" and "Two paths" in se
    rc, so, se = run(*base, "--marginalize", "--score_pairs", str(tmp_path / "missing"), str(out))
    assert rc == 1 and so == "" and "cannot read" in se
    for text, index in (("0 18\n3 5\n", 1), ("18 19\n", 0), ("0 32\n", 0)):
        bad = tmp_path / "bad.txt"
        bad.write_text(text)
        rc, so, se = run(*base, "--marginalize", "--score_pairs", str(bad), str(out))
        assert rc == 1 and so == "" and ("pair %d " % index) in se and "type-a" in se, (text, se)
    assert not out.exists()


TOTAL_CHAINS = 5  # odd on purpose: uneven shards
NA, NB, KA, KB = 40, 30, 3, 4


def _chain(gid):
    """The partition of global chain `gid`: the contiguous labels, rolled by gid within each type."""
    a, b = syn.planted_edges(NA, NB, 400, KA, KB, seed=2)
    lab = syn.contiguous_labels(NA, NB, KA, KB)
    lab = np.concatenate([np.roll(lab[:NA], gid), np.roll(lab[NA:], 2 * gid)])
    m, m_r, deg = block_state(a, b, lab, KA + KB)
    return lab, m, m_r, deg


class _RankModel:
    """What ChainShard.pooled_pair_scores asks of a model: pair_scores() of the chains the rank owns, `samples` samples."""

    def __init__(self, shard, pairs, samples):
        self.chains = [_chain(shard.first_chain_id + c) for c in range(shard.n_local)]
        self.pairs, self.samples = pairs, samples

    def pair_scores(self):
        labs, ms, m_rs = zip(*[c[:3] for c in self.chains])
        one = D.numpy_pair_scores(labs, ms, m_rs, self.chains[0][3], self.pairs)
        return one * self.samples, self.samples * len(self.chains)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        shard = D.ChainShard(TOTAL_CHAINS)
        model = _RankModel(shard, all_pairs(NA, NB), samples=3)
        s, terms = shard.pooled_pair_scores(model)
        np.save(os.path.join(out_dir, "sum%d.npy" % rank), s)
        np.save(os.path.join(out_dir, "terms%d.npy" % rank), np.array([terms]))
        np.save(os.path.join(out_dir, "local%d.npy" % rank), model.pair_scores()[0])
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_world2_gloo_pooled_pair_scores(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    s0, s1 = np.load(tmp_path / "sum0.npy"), np.load(tmp_path / "sum1.npy")
    assert (s0 == s1).all() and s0.dtype == np.float64
    assert int(np.load(tmp_path / "terms0.npy")[0]) == int(np.load(tmp_path / "terms1.npy")[0]) == 3 * TOTAL_CHAINS
    # two ranks: one f64 addition per pair
    assert (s0 == np.load(tmp_path / "local0.npy") + np.load(tmp_path / "local1.npy")).all()
    # ... and the single-process truth: all chains at once (another order of T = 15 non-negative terms: T 2^-52 relative)
    chains = [_chain(g) for g in range(TOTAL_CHAINS)]
    labs, ms, m_rs = zip(*[c[:3] for c in chains])
    want = 3 * D.numpy_pair_scores(labs, ms, m_rs, chains[0][3], all_pairs(NA, NB))
    assert (np.abs(s0 - want) <= 15 * 2.0 ** -52 * want).all()
    E = 400
    assert abs(s0.sum() - 15 * E) <= (len(s0) + 17) * 2.0 ** -52 * 15 * E
    # world size 1: the model's own
    one = D.ChainShard(TOTAL_CHAINS, rank=0, world_size=1)
    s, t = one.pooled_pair_scores(_RankModel(one, all_pairs(NA, NB), samples=1))
    assert t == TOTAL_CHAINS and (np.abs(3 * s - want) <= 15 * 2.0 ** -52 * want).all()
