"""GPU tests of the block summaries (include/bisbm.h, "Block summaries").  Expected words come from numpy_block_sums fed with the
per-chain block states read just before the sample and the permutations of the numpy alignment model (aligned_sample of
tests/test_align.py, mode_sample of tests/test_mode_marginals.py); every comparison is word for word."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_mode_marginals import _all_labels, _model, _refused
from test_mode_marginals import TWO_MODES, mode_sample, two_mode_pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")
NONE = B.MODE_NONE

pytestmark = pytest.mark.gpu


def _block_states(m):
    """(quads [C, ka, kb], n_rs [C, K], m_rs [C, K]) of every chain, as the getters give them."""
    ka = m.KA
    quads, n_rs, m_rs = [], [], []
    for c in range(m.n_chains):
        mm, m_r, n_r, _ = m._block_state(c, ("m", "m_r", "n_r"))
        assert (mm[:ka, ka:] == mm[ka:, :ka].T).all() and not mm[:ka, :ka].any() and not mm[ka:, ka:].any()
        quads.append(mm[:ka, ka:].copy())
        n_rs.append(n_r)
        m_rs.append(m_r)
    return np.array(quads), np.array(n_rs), np.array(m_rs)


def _aligned_tables(perm, quad, n_r, m_r, ka):
    """One chain's tables carried through its permutation."""
    perm = np.asarray(perm, dtype=np.int64)
    e = np.zeros_like(quad)
    e[np.ix_(perm[:ka], perm[ka:] - ka)] = quad
    n_al, m_al = np.zeros_like(n_r), np.zeros_like(m_r)
    n_al[perm], m_al[perm] = n_r, m_r
    return e, n_al, m_al


class _Running:
    """The running model of the sums of a handle: what block_sums must return after each sample."""

    def __init__(self, m, n_modes=1):
        self.m, self.M = m, n_modes
        K = m.KA + m.KB
        self.terms = np.zeros(n_modes, dtype=np.uint64)
        self.e = np.zeros((n_modes, 3, m.KA, m.KB), dtype=np.uint64)
        self.n = np.zeros((n_modes, 3, K), dtype=np.uint64)
        self.d = np.zeros((n_modes, 3, K), dtype=np.uint64)

    def sample(self, refs, moc, check_last=False):
        """One marginals_accumulate, checked.  refs: None (pooled: the library's reference, read after the sample) or the
        references of the modes; moc: the mode every chain must be counted into (NONE: not counted)."""
        m, ka, kb = self.m, self.m.KA, self.m.KB
        moc = np.asarray(moc, dtype=np.uint32)
        labs = _all_labels(m)
        quads, n_rs, m_rs = _block_states(m)
        m.marginals_accumulate()
        if refs is None:
            refs = [m.marginals_reference()[0]]
        _, perms, _ = mode_sample(labs, np.where(moc == NONE, -1, moc.astype(np.int64)), refs, m.na, ka, kb)
        full = np.zeros((m.n_chains, ka + kb), dtype=np.uint32)
        for c, p in perms.items():
            full[c] = p
            assert (m.marginals_alignment(c)[0] == p).all(), c  # (the device's own permutation is the model's)
        add = B.numpy_block_sums(full, quads, n_rs, m_rs, moc, self.M, ka, kb)
        self.terms += add["terms"]
        self.e += add["e"]
        self.n += add["n"]
        self.d += add["d"]
        self.check()
        if check_last:
            for c in range(m.n_chains):
                if moc[c] == NONE:
                    _refused(B.BISBM_ERR_STATE, "not counted", m.block_last, c)
                    continue
                mode, e, n_al, m_al = m.block_last(c)
                we, wn, wm = _aligned_tables(full[c], quads[c], n_rs[c], m_rs[c], ka)
                assert mode == moc[c] and (e == we).all() and (n_al == wn).all() and (m_al == wm).all(), c
        return full

    def check(self):
        for g in range(self.M):
            got = self.m.block_sums(g if self.M > 1 else None)
            assert got["terms"] == int(self.terms[g]), g
            for w in range(3):  # all nine planes
                assert (got["e"][w] == self.e[g, w]).all(), (g, w)
                assert (got["n"][w] == self.n[g, w]).all(), (g, w)
                assert (got["d"][w] == self.d[g, w]).all(), (g, w)


# ---------------------------------------------------------------------------------------------------- 1. pooled, aligned
@pytest.mark.parametrize("rng", ["philox", "mt19937-compat"])
def test_pooled_aligned_samples_equal_the_model(rng):
    m = _model(301, 203, 4, 6, 3000, 5, rng=rng)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    m.marginals_set_alignment(True)
    m.block_sums_set(True, keep_last=True)
    run = _Running(m)
    run.check()  # (all zero before the first sample)
    for sample in range(3):
        run.sample(None, [0] * 5, check_last=True)
        assert run.terms.tolist() == [5 * (sample + 1)]
        m.run_sweeps(1)
    s = m.block_summary()
    assert s["terms"] == 15 and s["e_mean"].shape == (4, 6) and abs(s["share"].sum() - 1.0) < 1e-12
    raw = m.block_sums()
    assert raw["e"][0].sum() == 15 * m.num_edges and raw["n"][0].sum() == 15 * m.n  # (every chain holds every edge and every node once)


# ---------------------------------------------------------------------------------------------------- 2. static modes, chunk edge
def test_static_modes_across_the_chunk_edge_and_both_splits(monkeypatch):
    chains = 130
    moc = np.full(chains, NONE, dtype=np.uint32)
    moc[np.arange(0, 130, 2)] = 0       # 65 chains: one more than a chunk of 64 inverse permutations
    moc[np.arange(1, 129, 2)] = 1       # 64 chains: exactly one chunk (the two modes interleave in chain order)
    moc[129] = 2                        # one chain
    sizes = [int((moc == g).sum()) for g in range(3)]
    assert sizes == [65, 64, 1]

    def run(split):
        if split is None:
            monkeypatch.delenv("BISBM_BLOCK_SPLIT", raising=False)
        else:
            monkeypatch.setenv("BISBM_BLOCK_SPLIT", split)
        m = _model(1500, 1500, 32, 32, 20000, chains)  # 1024 + 128 cells: more than one workgroup of 256 per mode
        m.shuffle_bisbm()
        m.run_sweeps(1)
        m.marginals_reset()
        m.marginals_set_modes(moc)
        m.block_sums_set(True)
        return m
    m = run(None)  # the library's own split: the chunks of a mode over several workgroups, 64-bit atomics
    r = _Running(m, 3)
    refs = None
    for sample in range(2):
        labs, S = _all_labels(m), m.entropy()
        if refs is None:
            refs = [labs[np.flatnonzero(moc == g)[np.argmin(S[moc == g])]] for g in range(3)]
        r.sample(refs, moc)
        assert r.terms.tolist() == [(sample + 1) * s for s in sizes]
        m.run_sweeps(1)
    # one owner per cell gives the same words
    one = run("1")
    for _ in range(2):
        one.marginals_accumulate()
        one.run_sweeps(1)
    for g in range(3):
        a, b = m.block_sums(g), one.block_sums(g)
        assert a["terms"] == b["terms"] and all((a[k] == b[k]).all() for k in ("e", "n", "d")), g


# ---------------------------------------------------------------------------------------------------- 3. large and lopsided
@pytest.mark.parametrize("shape", [(1000, 1000, 100, 120, 3), (601, 903, 2, 250, 2)], ids=["100+120", "2+250"])
def test_large_and_lopsided_tables(shape):
    na, nb, ka, kb, chains = shape
    m = _model(na, nb, ka, kb, 20000, chains)
    m.shuffle_bisbm()
    m.run_sweeps(1)
    m.marginals_set_alignment(True)
    m.block_sums_set(True, keep_last=True)
    r = _Running(m)
    r.sample(None, [0] * chains, check_last=True)
    m.run_sweeps(1)
    r.sample(None, [0] * chains)


# ---------------------------------------------------------------------------------------------------- 4. one block, squares past 2^32
def test_one_block_of_a_type_and_squares_past_two_to_the_32():
    m = _model(150, 150, 1, 3, 70000, 2)
    m.shuffle_bisbm()
    m.run_sweeps(1)
    assert m.get_m_r(0)[0] == 70000 == m.get_m_r(1)[0]
    m.marginals_set_alignment(True)
    m.block_sums_set(True)
    r = _Running(m)
    r.sample(None, [0, 0])
    got = m.block_sums()
    assert got["d"][2].any() and got["d"][2][0] == 2 * ((70000 * 70000) >> 32)  # the split of the square is reached
    assert got["d"][1][0] == 2 * ((70000 * 70000) & 0xFFFFFFFF)
    s = m.block_summary()
    assert s["m_r_mean"][0] == 70000.0 and s["m_r_sd"][0] == 0.0


# ---------------------------------------------------------------------------------------------------- 5. one partition, many numberings
def test_identical_partitions_under_different_numberings_have_no_spread():
    na, nb, ka, kb, chains = 300, 200, 5, 4, 8
    m = _model(na, nb, ka, kb, 3000, chains)
    truth = syn.contiguous_labels(na, nb, ka, kb).astype(np.int64)
    rs = np.random.default_rng(8)
    for c in range(chains):
        perm = np.arange(ka + kb) if c == 0 else np.concatenate([rs.permutation(ka), ka + rs.permutation(kb)])
        m.set_memberships(perm[truth].astype(np.uint32), chain=c)
    m.init_bisbm()
    m.marginals_set_alignment(True)
    m.marginals_set_reference(m.get_memberships(0))
    m.block_sums_set(True)
    m.marginals_accumulate()
    s = m.block_summary()
    assert s["terms"] == chains
    for key in ("e_sd", "n_sd", "m_r_sd"):
        assert (s[key] == 0.0).all(), key
    assert (s["e_mean"] == m.get_m(0)[:ka, ka:]).all() and (s["n_mean"] == m.get_n_r(0)).all() and (s["m_r_mean"] == m.get_m_r(0)).all()


# ---------------------------------------------------------------------------------------------------- 6. replica exchange
def test_replica_exchange_sums_the_cold_chains():
    m = _model(300, 200, 4, 4, 3000, 8)
    m.shuffle_bisbm()
    m.set_tempering([1.0, 1.6])
    m.marginals_set_alignment(True)
    m.block_sums_set(True, keep_last=True)
    r = _Running(m)
    for sample in range(3):
        m.tempering_run(2, 1)
        cold = m.tempering_state()[0] == 0
        assert cold.sum() == 4
        r.sample(None, np.where(cold, 0, NONE), check_last=True)
        assert m.block_sums()["terms"] == 4 * (sample + 1)


# ---------------------------------------------------------------------------------------------------- 7. anchored modes
def test_anchored_modes_sum_the_assigned_chains_only():
    t = TWO_MODES
    P, Q, starts = two_mode_pool()
    m = _model(t["na"], t["nb"], t["ka"], t["kb"], 3000, t["chains"])
    for c in range(m.n_chains):
        m.set_memberships(starts[c], chain=c)
    m.init_bisbm()
    vi, _ = m.partition_distances_to([P, Q])
    near = np.sort(vi.min(axis=1))
    threshold = float((near[4] + near[5]) / 2)  # the five nearest chains are within it, eleven are not
    assert near[5] - near[4] > 1e-6
    want = np.where(vi.min(axis=1) <= threshold, vi.argmin(axis=1), NONE).astype(np.uint32)
    assert (want == NONE).sum() == 11 and (want != NONE).sum() == 5
    m.marginals_set_mode_anchors([P, Q], threshold)
    m.block_sums_set(True, keep_last=True)
    r = _Running(m, 2)
    r.sample([P, Q], want, check_last=True)
    state = m.marginals_modes()
    assert (state["mode_of_chain"] == want).all() and state["unassigned"] == 11
    assert [m.block_sums(g)["terms"] for g in range(2)] == state["terms"].tolist() == [int((want == g).sum()) for g in range(2)]
    out = int(np.flatnonzero(want == NONE)[0])
    _refused(B.BISBM_ERR_STATE, "not counted", m.block_last, out)


# ---------------------------------------------------------------------------------------------------- 8. several device entries
def test_three_device_entries_equal_one_handle():
    moc = [0, 1, 0, NONE, 1, 1, 0, 0, 1, 0]

    def run(devices):
        out = []
        m = _model(500, 400, 6, 5, 5000, 10, **({} if devices is None else {"devices": devices}))
        m.shuffle_bisbm()
        m.run_sweeps(2)
        m.marginals_set_alignment(True)
        m.block_sums_set(True, keep_last=True)
        for _ in range(2):
            m.marginals_accumulate()
            m.run_sweeps(1)
        out.append(m.block_sums())
        out += [dict(zip("xenm", m.block_last(c))) for c in range(10)]
        m.marginals_reset()
        m.marginals_set_modes(moc)
        m.block_sums_set(True, keep_last=True)
        for _ in range(2):
            m.marginals_accumulate()
            m.run_sweeps(1)
        out += [m.block_sums(g) for g in range(2)]
        out += [dict(zip("xenm", m.block_last(c))) for c in range(10) if moc[c] != NONE]
        return out
    one, three = run(None), run([0, 0, 0])
    assert len(one) == len(three) and one[0]["terms"] == 20 and one[11]["terms"] == 10
    for x, y in zip(one, three):
        assert x.keys() == y.keys()
        for k in x:
            assert (np.asarray(x[k]) == np.asarray(y[k])).all(), k


# ---------------------------------------------------------------------------------------------------- 9. nothing else moves
def test_the_sums_change_nothing_else():
    runs = []
    for on in (False, True):
        m = _model(300, 200, 5, 4, 3000, 6)
        m.shuffle_bisbm()
        m.marginals_set_alignment(True)
        if on:
            m.block_sums_set(True, keep_last=True)
        for _ in range(2):
            m.run_sweeps(1)
            m.marginals_accumulate()
        out = [m.marginals_get(), m.marginals_map()]
        m.run_sweeps(1)
        out += [_all_labels(m), m.get_entropy()]
        for c in range(m.n_chains):
            out += [m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c)]
        runs.append(out)
    assert len(runs[0]) == len(runs[1])
    for x, y in zip(*runs):
        assert (x == y).all()


# ---------------------------------------------------------------------------------------------------- 10. life cycle and refusals
def test_life_cycle_and_refusals():
    STATE, INVALID, UNSUPPORTED = B.BISBM_ERR_STATE, B.BISBM_ERR_INVALID_ARG, B.BISBM_ERR_UNSUPPORTED
    m = _model(300, 200, 4, 4, 3000, 4)
    m.shuffle_bisbm()
    _refused(STATE, "bisbm_block_sums_set", m.block_sums)  # get before set
    _refused(STATE, "bisbm_block_sums_set", m.block_last, 0)
    assert m._L.bisbm_block_sums_set(m._h, 2) == INVALID and m._L.bisbm_block_sums_set(m._h, 4) == INVALID
    # an unaligned sample with the sums on is refused before anything is counted
    m.block_sums_set(True)
    _refused(STATE, "bisbm_marginals_set_alignment", m.marginals_accumulate)
    assert m.block_sums()["terms"] == 0 and not m.block_sums()["e"].any()
    _refused(STATE, "no internal marginal buffer", m.marginals_get)  # (the node histogram did not start either)
    _refused(INVALID, "out of range", m.block_sums, 1)  # a mode that does not exist
    _refused(STATE, "BISBM_BLOCK_KEEP_LAST", m.block_last, 0)  # get_last without KEEP_LAST
    m.marginals_set_alignment(True)
    m.block_sums_set(True, keep_last=True)
    _refused(STATE, "no aligned sample", m.block_last, 0)  # ... before a sample
    m.marginals_accumulate()
    m.marginals_accumulate()
    assert m.block_sums()["terms"] == 8 and m.block_last(3)[0] == 0
    # marginals_reset zeroes the sums
    m.marginals_reset()
    got = m.block_sums()
    assert got["terms"] == 0 and not (got["e"].any() or got["n"].any() or got["d"].any())
    _refused(STATE, "no aligned sample", m.block_last, 0)
    m.marginals_accumulate()
    assert m.block_sums()["terms"] == 4
    # block_sums_set zeroes them
    m.block_sums_set(True)
    assert m.block_sums()["terms"] == 0 and not m.block_sums()["n"].any()
    m.marginals_accumulate()
    # agg_merge to another shape restarts them (4 + 4 -> 4 + 3: the histogram's row length stays)
    m.agg_merge(0, 1, 5)
    assert (m.KA, m.KB) == (4, 3)
    got = m.block_sums()
    assert got["terms"] == 0 and got["e"].shape == (3, 4, 3) and not got["e"].any()
    m.marginals_accumulate()
    got = m.block_sums()
    assert got["terms"] == 4 and got["n"][0].sum() == 4 * m.n and got["e"][0].sum() == 4 * m.num_edges
    # set_modes starts them afresh
    m.marginals_reset()
    m.marginals_accumulate()
    m.marginals_reset()
    m.marginals_set_modes([0, 1, 1, NONE])
    assert [m.block_sums(g)["terms"] for g in range(2)] == [0, 0]
    _refused(INVALID, "out of range", m.block_sums, 2)
    m.marginals_accumulate()
    assert [m.block_sums(g)["terms"] for g in range(2)] == [1, 2]
    # off: the buffers are freed and get fails
    m.block_sums_set(False)
    _refused(STATE, "bisbm_block_sums_set", m.block_sums, 0)
    m.marginals_accumulate()  # (and a sample runs as before)
    # a wide handle is refused by the aligned sample
    w = _model(400, 300, 200, 100, 4000, 2)
    w.shuffle_bisbm()
    w.marginals_set_alignment(True)
    w.block_sums_set(True)
    _refused(UNSUPPORTED, "byte labels", w.marginals_accumulate)


# ---------------------------------------------------------------------------------------------------- 11. drivers
def _same_summary(x, y):
    assert x.keys() == y.keys()
    for k in x:
        assert np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=True), k


def test_marginalize_with_blocks_equals_the_hand_driven_loop():
    def model():
        m = _model(300, 200, 4, 5, 3000, 8)
        m.shuffle_bisbm()
        return m
    m = model()
    labels, counts = B.marginalize(m, 2, 3, 1, align=True, blocks=True)
    h = model()
    h.run_sweeps(2)
    h.marginals_reset()
    h.marginals_set_alignment(True)
    h.block_sums_set(True)
    for _ in range(3):
        h.run_sweeps(1)
        h.marginals_accumulate()
    assert (h.marginals_get() == counts).all() and m.block_summary()["terms"] == 24
    _same_summary(m.block_summary(), h.block_summary())
    # ... and per mode
    moc = [0, 1, 0, 1, NONE, 1, 0, 0]
    m = model()
    B.marginalize_modes(m, 2, 3, 1, mode_of_chain=moc, blocks=True)
    h = model()
    h.run_sweeps(2)
    h.marginals_reset()
    h.marginals_set_modes(moc)
    h.block_sums_set(True)
    for _ in range(3):
        h.run_sweeps(1)
        h.marginals_accumulate()
    for g in range(2):
        assert m.block_summary(g)["terms"] == 3 * moc.count(g)
        _same_summary(m.block_summary(g), h.block_summary(g))


def _parse_block_summary(path):
    """[{terms, ka, kb, n_mean, n_sd, m_r_mean, m_r_sd, e_mean, e_sd}] of the file --block_summary writes."""
    modes = []
    for line in open(path).read().splitlines():
        tok = line.split()
        if tok[0] == "mode":
            assert tok[2] == "terms" and tok[4] == "ka" and tok[6] == "kb" and int(tok[1]) == len(modes)
            modes.append({"terms": int(tok[3]), "ka": int(tok[5]), "kb": int(tok[7]), "e_mean": [], "e_sd": []})
        elif tok[0] in ("e_mean", "e_sd"):
            assert int(tok[1]) == len(modes[-1][tok[0]])
            modes[-1][tok[0]].append([float(x) for x in tok[2:]])
        else:
            modes[-1][tok[0]] = [float(x) for x in tok[1:]]
    return modes


def test_cli_block_summary_writes_the_python_numbers(tmp_path):
    na, nb, ka, kb, n = 300, 200, 4, 5, 500
    a, b = syn.planted_edges(na, nb, 3000, ka, kb, seed=4)
    el = tmp_path / "planted.edgelist"
    np.savetxt(el, np.stack([a, b], axis=1), fmt="%d")
    truth = syn.contiguous_labels(na, nb, ka, kb)
    out = tmp_path / "blocks.txt"
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    r = subprocess.run([cli, "-e", str(el), "-y", str(na), str(nb), "-n", *map(str, np.bincount(truth)), "-z", str(ka), str(kb),
                        "-E", "1", "-d", "5", "--rng", "philox", "--chains", "8", "--randomize", "-b", str(3 * n), "-t", str(4 * n),
                        "-f", str(n), "--marginalize", "--align", "--block_summary", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "block_summary: 1 mode(s)" in r.stderr
    ea, eb = B.load_edge_list(str(el))
    rp, cl = B.edge_to_adj((ea, eb), n)
    m = B.BlockModel(truth, syn.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rp, cl), n_chains=8, seed=5, gen_seed=6)
    m.shuffle_bisbm()
    labels, _ = B.marginalize(m, 3, 4, 1, align=True, blocks=True)
    assert r.stdout.split() == [str(x) for x in labels]
    s = m.block_summary()
    (got,) = _parse_block_summary(out)
    assert (got["terms"], got["ka"], got["kb"]) == (32, ka, kb) and s["terms"] == 32
    for key in ("n_mean", "n_sd", "m_r_mean", "m_r_sd", "e_mean", "e_sd"):
        assert (np.array(got[key]) == s[key]).all(), key  # %.17g round-trips: the same doubles
    assert (s["e_sd"] > 0).any()


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "block_structure.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "mean block matrix" in r.stdout and "planted" in r.stdout, r.stdout + r.stderr
