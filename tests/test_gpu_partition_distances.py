"""GPU tests of the partition distances (include/bisbm.h, "Partition distances and posterior modes").  The reference is the
numpy statement of tests/test_partition_distances.py (np.add.at tables, fsum sums) fed with get_memberships(c), which the
parity tests pin to the checker.  Integers are compared bit for bit; VI and H against the exact sums within the derived bound
vi_tolerance / h_tolerance of that file, with no other slack."""
import contextlib
import importlib
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from test_partition_distances import (h_tolerance, move_nodes, numpy_contingency, numpy_entropy, numpy_vi, random_labels, relabel,
                                      vi_tolerance)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def regime(name):
    """BISBM_PARTITION_REGIME=fused|split forces the many-pairs / few-pairs path of the counting kernel; None: the library's
    own choice."""
    old = os.environ.pop("BISBM_PARTITION_REGIME", None)
    if name:
        os.environ["BISBM_PARTITION_REGIME"] = name
    try:
        yield
    finally:
        os.environ.pop("BISBM_PARTITION_REGIME", None)
        if old is not None:
            os.environ["BISBM_PARTITION_REGIME"] = old


def _model(na, nb, ka, kb, edges, chains, rng="philox", seed=9, graph_seed=4, isolated=0, **kw):
    a, b = syn.planted_edges(na, nb, edges, ka, kb, seed=graph_seed)
    rp, cl = B.edge_to_adj((a, b), na + nb + isolated)  # `isolated` type-b nodes without an edge at the end
    lab = syn.contiguous_labels(na, nb + isolated, ka, kb)
    return B.BlockModel(lab, syn.types_vector(na, nb + isolated), ka + kb, ka, kb, 1.0, (rp, cl), n_chains=chains, rng=rng, seed=seed,
                        gen_seed=seed + 1, **kw)


def _labels(m, chains):
    return {int(c): m.get_memberships(int(c)) for c in chains}


def _check_against_numpy(m, sel, vi, H, labs=None, pairs=None):
    """vi / H of the selection `sel` against the numpy statement: every pair (or the listed positions) within the bound, the
    matrix exactly symmetric, non-negative, its diagonal exactly 0."""
    sel = [int(c) for c in sel]
    labs = labs or _labels(m, sel)
    shape = {c: m.ka_kb(c) for c in sel}
    n = m.n
    assert vi.shape == (len(sel), len(sel)) and H.shape == (len(sel),)
    assert (vi == vi.T).all() and (np.diag(vi) == 0.0).all() and (vi >= 0.0).all()
    for i, c in enumerate(sel):
        want = numpy_entropy(labs[c], sum(shape[c]))
        print("H", c, H[i], want, abs(H[i] - want), h_tolerance(n, *shape[c]))
        assert abs(H[i] - want) <= h_tolerance(n, *shape[c]), (c, H[i], want)
    todo = pairs if pairs is not None else [(i, j) for i in range(len(sel)) for j in range(i + 1, len(sel))]
    worst = 0.0
    for i, j in todo:
        c, d = sel[i], sel[j]
        want = max(numpy_vi(labs[c], labs[d], sum(shape[c]), sum(shape[d])), 0.0)
        tol = vi_tolerance(n, *shape[c], *shape[d])
        worst = max(worst, abs(vi[i, j] - want) / tol)
        assert abs(vi[i, j] - want) <= tol, (c, d, vi[i, j], want, tol)
    print("worst |VI - exact| / bound over %d pairs: %.4f" % (len(todo), worst))


# ---- 1. contingency tables: integers, bit-equal to numpy ---------------------------------------------------------------------
CONTINGENCY = [  # na, nb, ka, kb, edges (n = na + nb + 3 isolated nodes: not a multiple of 4 or 1024)
    (1201, 1103, 4, 6, 12000),
    (1201, 1103, 32, 32, 12000),
    (1201, 1103, 64, 64, 12000),
    (1201, 1103, 100, 128, 12000),
    (601, 903, 2, 250, 8000),  # a table larger than the LDS: counted straight in HBM
]


@pytest.mark.parametrize("case", CONTINGENCY, ids=lambda c: "%d+%d" % (c[2], c[3]))
def test_contingency_is_bit_equal_to_numpy(case):
    na, nb, ka, kb, edges = case
    m = _model(na, nb, ka, kb, edges, 5, isolated=3)
    assert m.n % 4 != 0
    m.shuffle_bisbm()
    for step in range(2):
        labs = _labels(m, range(5))
        for c, d in ((0, 1), (3, 2), (4, 4), (1, 4)):
            t = m.partition_contingency(c, d)
            assert t.dtype == np.uint32 and t.shape == (ka + kb, ka + kb)
            assert (t.astype(np.int64) == numpy_contingency(labs[c], labs[d], ka + kb, ka + kb)).all(), (step, c, d)
            assert t.sum() == m.n and t[:ka, ka:].sum() == 0 and t[ka:, :ka].sum() == 0
        m.run_sweeps(2)  # ... and after sweeps
    with pytest.raises(B.BisbmError) as e:
        m.partition_contingency(0, 5)
    assert e.value.code == B.BISBM_ERR_INVALID_ARG and "chain 5" in str(e.value)


# ---- 2. distances of 16 chains with labels set per chain -----------------------------------------------------------------------
def _sixteen(na=3001, nb=2502, ka=8, kb=6, **kw):
    m = _model(na, nb, ka, kb, 30000, 16, **kw)
    truth = syn.contiguous_labels(na, nb, ka, kb)
    rng = np.random.default_rng(11)
    for c in range(16):
        if c < 5:
            lab = relabel(truth, na, ka, kb, rng)
        elif c < 10:
            lab = move_nodes(relabel(truth, na, ka, kb, rng), na, ka, kb, 0.05, rng)
        else:
            lab = random_labels(na, nb, ka, kb, rng)
        m.set_memberships(lab, chain=c)
    m.init_bisbm()
    return m


def test_distances_of_sixteen_set_chains():
    m = _sixteen()
    vi, H = m.partition_distances()
    _check_against_numpy(m, range(16), vi, H)
    assert (vi[:5, :5] <= vi_tolerance(m.n, 8, 6, 8, 6)).all()  # one partition in five numberings
    assert vi[:5, 10:].min() > vi[:5, 5:10].max() > 0
    vi2, H2 = m.partition_distances()
    assert (vi2 == vi).all() and (H2 == H).all()  # the same call, the same bits
    # a subset and a permuted selection: the same distances in the right positions
    tol = vi_tolerance(m.n, 8, 6, 8, 6)
    sub = [12, 3, 7]
    vs, Hs = m.partition_distances(sub)
    _check_against_numpy(m, sub, vs, Hs)
    assert (np.abs(vs - vi[np.ix_(sub, sub)]) <= 2 * tol).all() and (np.abs(Hs - H[sub]) <= 2 * h_tolerance(m.n, 8, 6)).all()
    perm = np.random.default_rng(2).permutation(16)
    vp, Hp = m.partition_distances(perm)
    _check_against_numpy(m, perm, vp, Hp)
    assert (np.abs(vp - vi[np.ix_(perm, perm)]) <= 2 * tol).all()
    # only one output asked for
    L = B.lib()
    h_only = np.zeros(16)
    assert L.bisbm_partition_distances(m._h, 16, None, None, B._p(h_only, B._f64p)) == B.BISBM_OK and (h_only == H).all()
    one, H1 = m.partition_distances([4])
    assert one.tolist() == [[0.0]] and H1[0] == H[4]


# ---- 3. both regimes and a tile edge ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [2, 3, 33, 130])
def test_both_regimes_and_tile_edges(count):
    m = _model(300, 203, 4, 6, 3000, 130)
    m.shuffle_bisbm()
    m.run_sweeps(1)
    sel = np.random.default_rng(count).permutation(130)[:count]
    labs = _labels(m, sel)
    got = {}
    for name in ("fused", "split", None):
        with regime(name):
            got[name] = m.partition_distances(sel)
        _check_against_numpy(m, sel, *got[name], labs=labs)
    # both regimes reduce the same integer tables with the same function: the same bits
    assert (got["fused"][0] == got["split"][0]).all() and (got["fused"][1] == got["split"][1]).all()
    assert (got[None][0] == got["split"][0]).all()


def test_both_regimes_with_larger_tables():
    """32 + 32 blocks (tiles of 4 x 4 pairs fill the LDS of a workgroup) and 64 + 64 (tiles of 2 x 2)."""
    for ka, kb, chains in ((32, 32, 11), (64, 64, 7)):
        m = _model(2001, 1502, ka, kb, 30000, chains)
        m.shuffle_bisbm()
        m.run_sweeps(1)
        labs = _labels(m, range(chains))
        with regime("fused"):
            f = m.partition_distances()
        with regime("split"):
            s = m.partition_distances()
        _check_against_numpy(m, range(chains), *f, labs=labs)
        assert (f[0] == s[0]).all() and (f[1] == s[1]).all()


def test_distances_with_tables_counted_straight_in_hbm():
    """2 + 250 blocks: a pair's table (62 504 cells) is larger than the LDS, so tiles of one pair are counted straight in HBM and
    reduced by the second kernel."""
    m = _model(601, 903, 2, 250, 8000, 6)
    m.shuffle_bisbm()
    m.run_sweeps(1)
    labs = _labels(m, range(6))
    for name in ("fused", None):  # (there is no fused form of this path: the switch changes nothing)
        with regime(name):
            vi, H = m.partition_distances()
        _check_against_numpy(m, range(6), vi, H, labs=labs)
    sub = [5, 1, 2]
    _check_against_numpy(m, sub, *m.partition_distances(sub), labs=labs)


# ---- 4. chains of different shapes ---------------------------------------------------------------------------------------------------
def _mixed_shapes_model(**kw):
    rowptr, col, na, nb = O.load_graph("n_1000")
    g = B.BlockModel(O.contiguous_labels(na, nb, 6, 6), syn.types_vector(na, nb), 12, 6, 6, 1.0, (rowptr, col), n_chains=32, seed=4, **kw)
    g.shuffle_bisbm()
    g.run_sweeps(2)
    for _ in range(4):
        if g.mixed_shapes:
            break
        g.agg_merge(2, None, 10)
    assert g.mixed_shapes
    return g


def test_mixed_shapes_after_a_one_argument_merge():
    g = _mixed_shapes_model()
    shapes = {g.ka_kb(c) for c in range(32)}
    assert len(shapes) > 1
    g.run_sweeps(1)
    labs = _labels(g, range(32))
    for name in ("fused", "split"):
        with regime(name):
            vi, H = g.partition_distances()
        _check_against_numpy(g, range(32), vi, H, labs=labs)
    c = 0
    d = next(x for x in range(32) if g.ka_kb(x) != g.ka_kb(0))
    t = g.partition_contingency(c, d)
    assert t.shape == (sum(g.ka_kb(c)), sum(g.ka_kb(d)))
    assert (t.astype(np.int64) == numpy_contingency(labs[c], labs[d], *t.shape)).all()


# ---- 5. mt19937-compat ------------------------------------------------------------------------------------------------------------
def test_compat_mode():
    m = _model(400, 301, 7, 3, 3000, 6, rng="mt19937-compat")
    m.shuffle_bisbm()
    m.run_sweeps(2)
    vi, H = m.partition_distances()
    _check_against_numpy(m, range(6), vi, H)


# ---- 6. replica exchange ------------------------------------------------------------------------------------------------------------
def test_replica_exchange_compares_all_chains_and_modes_default_to_rung_zero():
    m = _model(600, 501, 5, 6, 6000, 16)
    m.shuffle_bisbm()
    m.set_tempering([1.0, 1.4, 2.0, 3.0])
    m.tempering_run(4, 1)
    vi, H = m.partition_distances()
    _check_against_numpy(m, range(16), vi, H)
    rung = m.tempering_state()[0]
    cold = np.flatnonzero(rung == 0)
    out = m.partition_modes(0.5)
    assert out["chains"].tolist() == cold.tolist() and len(cold) == 4
    assert (out["vi"] == m.partition_distances(cold)[0]).all()
    assert len(out["mode"]) == 4 and abs(out["weights"].sum() - 1.0) < 1e-12
    everything = m.partition_modes(0.5, chains=np.arange(16))
    assert len(everything["mode"]) == 16


# ---- 7. several device entries ------------------------------------------------------------------------------------------------------
def test_three_device_entries_equal_one_device_bit_for_bit():
    res = []
    for devices in (None, [0, 0, 0]):
        kw = {} if devices is None else {"devices": devices}
        m = _model(900, 701, 6, 5, 9000, 21, **kw)
        m.shuffle_bisbm()
        m.run_sweeps(2)
        sel = [20, 0, 7, 8, 13, 14, 19]
        res.append((m.partition_distances(), m.partition_distances(sel), m.partition_contingency(2, 17)))
        m.close()
    one, three = res
    assert (one[0][0] == three[0][0]).all() and (one[0][1] == three[0][1]).all()
    assert (one[1][0] == three[1][0]).all() and (one[1][1] == three[1][1]).all()
    assert (one[2] == three[2]).all()


# ---- 8. - 10. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    wide = _model(400, 300, 200, 100, 4000, 2)
    wide.shuffle_bisbm()
    with pytest.raises(B.BisbmError) as e:
        wide.partition_distances()
    assert e.value.code == B.BISBM_ERR_UNSUPPORTED and "byte labels only (at most 256 blocks; " in str(e.value)
    with pytest.raises(B.BisbmError) as e:
        wide.partition_contingency(0, 1)
    assert e.value.code == B.BISBM_ERR_UNSUPPORTED
    m = _model(300, 200, 4, 4, 3000, 4)
    with pytest.raises(B.BisbmError) as e:  # before init / shuffle
        m.partition_distances()
    assert e.value.code == B.BISBM_ERR_STATE and "bisbm_init" in str(e.value)
    m.shuffle_bisbm()
    with pytest.raises(B.BisbmError) as e:
        m.partition_distances([0, 2, 1, 2])
    assert e.value.code == B.BISBM_ERR_INVALID_ARG and "chain 2 is listed twice" in str(e.value)
    with pytest.raises(B.BisbmError) as e:
        m.partition_distances([0, 4])
    assert e.value.code == B.BISBM_ERR_INVALID_ARG and "chain 4" in str(e.value) and "out of range" in str(e.value)
    with pytest.raises(B.BisbmError) as e:
        m.partition_distances([])
    assert e.value.code == B.BISBM_ERR_INVALID_ARG
    assert B.lib().bisbm_partition_distances(m._h, 3, None, None, None) == B.BISBM_ERR_INVALID_ARG  # NULL selects all 4


# ---- 11. the chains' state is untouched --------------------------------------------------------------------------------------------------
def test_state_is_untouched():
    def run(call):
        m = _model(800, 601, 6, 6, 8000, 12)
        m.shuffle_bisbm()
        m.run_sweeps(2)
        if call:
            before = (np.array([m.get_memberships(c) for c in range(12)]), m.get_entropy().copy(), m.entropy().copy())
            m.partition_distances()
            m.partition_contingency(1, 2)
            m.partition_modes(0.3)
            after = (np.array([m.get_memberships(c) for c in range(12)]), m.get_entropy(), m.entropy())
            assert all((x == y).all() for x, y in zip(before, after))
        rates = m.run_sweeps(2)
        return np.array([m.get_memberships(c) for c in range(12)]), m.get_entropy(), rates, np.array([m.get_m(c) for c in range(12)])
    plain, called = run(False), run(True)
    assert all((x == y).all() for x, y in zip(plain, called))


# ---- 12. full size ------------------------------------------------------------------------------------------------------------------------
def test_full_size_all_pairs_of_64_chains():
    na = nb = 500_000
    m = _model(na, nb, 32, 32, 2_000_000, 64, seed=3)
    truth = syn.contiguous_labels(na, nb, 32, 32)
    rng = np.random.default_rng(5)
    for c in range(64):  # even chains: the planted partition in their own numbering with 0 - 8 % of the nodes moved; odd: random
        lab = move_nodes(relabel(truth, na, 32, 32, rng), na, 32, 32, 0.02 * (c % 5), rng) if c % 2 == 0 else random_labels(na, nb, 32, 32, rng)
        m.set_memberships(lab, chain=c)
    m.init_bisbm()
    got = {}
    for name in ("fused", "split"):
        with regime(name):
            got[name] = m.partition_distances()
    assert (got["fused"][0] == got["split"][0]).all() and (got["fused"][1] == got["split"][1]).all()
    vi, H = got["fused"]
    assert (vi == vi.T).all() and (np.diag(vi) == 0).all() and (vi >= 0).all()
    pairs = set()
    while len(pairs) < 10:
        i, j = sorted(rng.choice(64, size=2, replace=False).tolist())
        pairs.add((i, j))
    pairs = sorted(pairs)
    chains = sorted({c for p in pairs for c in p})
    labs = _labels(m, chains)
    n = m.n
    for i, j in pairs:
        want = max(numpy_vi(labs[i], labs[j], 64, 64), 0.0)
        tol = vi_tolerance(n, 32, 32, 32, 32)
        print("VI", i, j, vi[i, j], want, abs(vi[i, j] - want), tol)
        assert abs(vi[i, j] - want) <= tol, (i, j, vi[i, j], want, tol)
    for c in chains:
        want = numpy_entropy(labs[c], 64)
        assert abs(H[c] - want) <= h_tolerance(n, 32, 32), (c, H[c], want)
    i, j = pairs[0]
    assert (m.partition_contingency(i, j).astype(np.int64) == numpy_contingency(labs[i], labs[j], 64, 64)).all()


# ---- 14. end to end -----------------------------------------------------------------------------------------------------------------------
def test_two_planted_answers_give_two_modes_of_eight():
    na, nb, ka, kb = 2000, 1501, 6, 5
    m = _model(na, nb, ka, kb, 20000, 16)
    rng = np.random.default_rng(8)
    A = syn.contiguous_labels(na, nb, ka, kb)
    Bp = random_labels(na, nb, ka, kb, rng)  # a different partition
    starts = []
    for c in range(16):
        base = A if c % 2 == 0 else Bp  # interleaved: even chains near A, odd chains near B
        starts.append(move_nodes(relabel(base, na, ka, kb, rng), na, ka, kb, 0.03, rng))
        m.set_memberships(starts[-1], chain=c)
    m.init_bisbm()
    K = ka + kb
    ref = np.array([[numpy_vi(starts[c], starts[d], K, K) for d in range(16)] for c in range(16)])
    same = (np.arange(16)[:, None] % 2) == (np.arange(16)[None, :] % 2)
    within, between = ref[same].max(), ref[~same].min()
    assert within < between
    tau = 0.5 * (within + between)
    out = m.partition_modes(tau)
    assert out["chains"].tolist() == list(range(16))
    assert out["mode"].tolist() == [0, 1] * 8
    assert out["weights"].tolist() == [0.5, 0.5]
    assert out["medoids"][0] % 2 == 0 and out["medoids"][1] % 2 == 1
    S = m.entropy()
    assert out["lowest_entropy"].tolist() == [int(2 * np.argmin(S[0::2])), int(2 * np.argmin(S[1::2]) + 1)]
    mode, med = B.partition_modes(out["vi"], tau)
    assert (mode == out["mode"]).all() and (med == out["medoids"]).all()


def test_cli_modes_writes_what_the_driver_computes(tmp_path):
    na, nb, ka, kb = 600, 500, 4, 4
    n = na + nb
    a, b = syn.planted_edges(na, nb, 6000, ka, kb, seed=4)
    el = tmp_path / "planted.edgelist"
    np.savetxt(el, np.stack([a, b], axis=1), fmt="%d")
    truth = syn.contiguous_labels(na, nb, ka, kb)
    sizes = np.bincount(truth)
    ea, eb = B.load_edge_list(str(el))
    rp, cl = B.edge_to_adj((ea, eb), n)
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    for extra, kw in (([], {}), (["--tempering", "1", "1.5", "2.5", "4"], {"tempering": [1.0, 1.5, 2.5, 4.0]})):
        m = B.BlockModel(truth, syn.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rp, cl), n_chains=16, seed=5, gen_seed=6)
        m.shuffle_bisbm()
        B.marginalize(m, 3, 2, 1, align=True, **kw)
        sel = np.arange(16) if not kw else np.flatnonzero(m.tempering_state()[0] == 0)
        vi, _ = m.partition_distances(sel)
        off = vi[np.triu_indices(len(sel), 1)]
        tau = float(np.median(off))
        want = m.partition_modes(tau)
        assert want["chains"].tolist() == sel.tolist()
        out = tmp_path / "modes.txt"
        r = subprocess.run([cli, "-e", str(el), "-y", str(na), str(nb), "-n", *map(str, sizes), "-z", str(ka), str(kb), "-E", "1", "-d", "5",
                            "--rng", "philox", "--chains", "16", "--randomize", "-b", str(3 * n), "-t", str(2 * n), "-f", str(n),
                            "--marginalize", "--align", "--modes", str(out), repr(tau)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        rows = [line.split() for line in out.read_text().splitlines()]
        assert [int(x[0]) for x in rows] == sel.tolist()
        assert [int(x[1]) for x in rows] == want["mode"].tolist()
        med_pos = [sel.tolist().index(c) for c in want["medoids"]]
        assert [float(x[2]) for x in rows] == [vi[i, med_pos[want["mode"][i]]] for i in range(len(sel))]
        assert "modes: %d\n" % len(want["medoids"]) in r.stderr
        for k, c in enumerate(want["medoids"]):
            assert "mode %d: %d chain(s)" % (k, (want["mode"] == k).sum()) in r.stderr and "medoid chain %d," % c in r.stderr
        # stdout (the labels) is what the run prints without the flag
        plain = subprocess.run([a_ for a_ in r.args if a_ not in ("--modes", str(out), repr(tau))], capture_output=True, text=True, timeout=600)
        assert plain.returncode == 0 and plain.stdout == r.stdout
        m.close()


def test_example_runs():
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "posterior_modes.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "modes: " in r.stdout and "contingency table" in r.stdout
