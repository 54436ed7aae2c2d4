"""GPU tests of the chain traces (include/bisbm.h, "Chain traces").  The host keeps get_memberships of every chain at every
record; the references are bisbm_partition_distances_to with the snapshot as a reference of the chain's own shape (bit for bit:
that equality is part of the definition) and the numpy statement of tests/test_partition_distances.py within its derived bound
vi_tolerance, with no other slack.  Integers are compared exactly."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_partition_distances import _mixed_shapes_model, _model, regime
from test_partition_distances import numpy_vi, vi_tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")
mz = importlib.import_module("bipartitesbm-mcmc_amd.marginalize")

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _all_labels(m):
    return np.array([m.get_memberships(c) for c in range(m.n_chains)])


def _same_raw(x, y):
    """two results of BlockModel._trace_raw, bit for bit (NaN included)"""
    return all((_bits(a) == _bits(b)).all() if a.dtype == np.float64 else (a == b).all() for a, b in zip(x[:4], y[:4])) and x[4] == y[4]


# ---- 1. the lag sums against the definition, in every regime ---------------------------------------------------------------------
CASES = [  # na, nb, ka, kb, chains, depth, rng: the smallest shapes at which each path of the counting kernel can go wrong
    (301, 203, 4, 6, 16, 5, "philox"),          # n, na no multiples of 4: the type boundary inside a label word; a partial age tile
    (301, 203, 4, 6, 16, 5, "mt19937-compat"),
    (1500, 1500, 32, 32, 16, 4, "philox"),      # full age tiles: four 8 KB tables per workgroup
    (1000, 1000, 100, 120, 5, 3, "philox"),     # one table (24 400 cells) fills a workgroup's LDS: a tile of one age
    (601, 903, 2, 250, 5, 2, "philox"),         # a table larger than the LDS: counted straight in HBM
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d+%d-%s" % (c[2], c[3], c[6]))
def test_records_match_distances_to_and_numpy_in_every_regime(case):
    na, nb, ka, kb, chains, depth, rng = case
    n, records = na + nb, 12
    models = {name: _model(na, nb, ka, kb, 10 * n, chains, rng=rng) for name in (None, "fused", "split")}
    for m in models.values():
        m.shuffle_bisbm()
        m.trace_set(depth)
    main = models[None]
    tol = vi_tolerance(n, ka, kb, ka, kb)
    hist, S_want, H_want = [], [], []
    vi_host = np.zeros((chains, depth))
    agree_prev = np.zeros((chains, depth), dtype=np.uint64)
    worst = 0.0
    for rec in range(records):
        if rec:
            for m in models.values():
                m.run_sweeps(1)
        raw = {}
        for name, m in models.items():
            with regime(name):
                m.trace_record()
            raw[name] = m._trace_raw()
        assert _same_raw(raw[None], raw["fused"]) and _same_raw(raw[None], raw["split"]), rec  # (e)
        vi_sum, agree_sum, vi_last, pairs, got_records = raw[None]
        now = _all_labels(main)
        S_want.append(main.entropy().copy())
        H_want.append(main.partition_distances()[1])
        ages = min(depth, rec)  # a partial ring at first, then several wrap-arounds
        assert got_records == rec + 1
        assert pairs.tolist() == [max(0, rec + 1 - a) for a in range(1, depth + 1)]
        assert np.isnan(vi_last[:, ages:]).all() and not np.isnan(vi_last[:, :ages]).any()
        agree = agree_sum - agree_prev
        assert (agree[:, ages:] == 0).all()
        for a in range(1, ages + 1):
            then = hist[rec - a]
            for c in range(chains):
                ref = main.partition_distances_to(then[c], chains=[c], shapes=[(ka, kb)])[0][0, 0]
                assert _bits([vi_last[c, a - 1]])[0] == _bits([ref])[0], (rec, c, a, vi_last[c, a - 1], ref)  # (a)
                want = max(numpy_vi(now[c], then[c], ka + kb, ka + kb), 0.0)
                worst = max(worst, abs(vi_last[c, a - 1] - want) / tol)
                assert abs(vi_last[c, a - 1] - want) <= tol, (rec, c, a, vi_last[c, a - 1], want, tol)  # (b)
                assert int(agree[c, a - 1]) == int((now[c] == then[c]).sum()), (rec, c, a)  # (c)
        vi_host[:, :ages] += vi_last[:, :ages]  # (one add per record and cell, as the library's)
        assert (_bits(vi_sum) == _bits(vi_host)).all()  # (d)
        agree_prev = agree_sum.copy()
        hist.append(now)
    print("worst |VI - exact| / bound: %.4f" % worst)
    assert vi_sum[:, 0].min() > 0  # the chains did move
    for name, m in models.items():  # (f)
        assert (_bits(m.trace_series("S")) == _bits(S_want)).all(), name
        assert (_bits(m.trace_series("H")) == _bits(H_want)).all(), name
    lags = main.trace_lags()
    assert lags["records"] == records and (lags["pairs"] == pairs).all()
    assert (_bits(lags["vi_mean"]) == _bits(vi_sum / pairs.astype(np.float64))).all()
    assert (_bits(lags["changed"]) == _bits(1.0 - agree_sum.astype(np.float64) / (pairs.astype(np.float64) * float(n)))).all()
    assert ((lags["changed"] >= 0) & (lags["changed"] <= 1)).all()


# ---- 2. two records with nothing between them ------------------------------------------------------------------------------------
def test_two_records_without_a_sweep_agree_everywhere():
    m = _model(301, 203, 4, 6, 3000, 8)
    m.shuffle_bisbm()
    m.run_sweeps(1)
    m.trace_set(3)
    m.trace_record()
    m.trace_record()
    vi_sum, agree_sum, vi_last, pairs, records = m._trace_raw()
    assert records == 2 and pairs.tolist() == [1, 0, 0]
    assert (agree_sum[:, 0] == m.n).all() and (agree_sum[:, 1:] == 0).all()
    assert (vi_last[:, 0] <= vi_tolerance(m.n, 4, 6, 4, 6)).all() and (vi_last[:, 0] >= 0).all()  # rounding size, not required 0.0
    lags = m.trace_lags()
    assert (lags["changed"][:, 0] == 0.0).all() and np.isnan(lags["changed"][:, 1:]).all() and np.isnan(lags["vi_mean"][:, 1:]).all()


# ---- 3. the state is only read -------------------------------------------------------------------------------------------------------
def test_state_is_untouched():
    def run(call):
        m = _model(800, 601, 6, 6, 8000, 12)
        m.shuffle_bisbm()
        m.run_sweeps(2)
        if call:
            m.trace_set(3)
            before = (_all_labels(m), m.get_entropy().copy(), m.entropy().copy())
            for _ in range(5):
                m.trace_record()
            after = (_all_labels(m), m.get_entropy(), m.entropy())
            assert all((x == y).all() for x, y in zip(before, after))
        rates = m.run_sweeps(1)
        if call:
            m.trace_record()
        return _all_labels(m), m.get_entropy(), rates, np.array([m.get_m(c) for c in range(12)])
    plain, called = run(False), run(True)
    assert all((x == y).all() for x, y in zip(plain, called))


# ---- 4. several device entries -----------------------------------------------------------------------------------------------------
def test_two_device_entries_equal_one_handle_bit_for_bit():
    res = []
    for devices in (None, [0, 0]):
        kw = {} if devices is None else {"devices": devices}
        m = _model(900, 701, 6, 5, 9000, 10, **kw)
        m.shuffle_bisbm()
        m.trace_set(4)
        out = []
        for _ in range(6):
            m.run_sweeps(1)
            m.trace_record()
            out.append(m._trace_raw())
        res.append((out, m.trace_series("S"), m.trace_series("H")))
        m.close()
    one, two = res
    assert all(_same_raw(x, y) for x, y in zip(one[0], two[0]))
    assert (_bits(one[1]) == _bits(two[1])).all() and (_bits(one[2]) == _bits(two[2])).all()
    assert one[0][-1][4] == 6 and one[0][-1][3].tolist() == [5, 4, 3, 2]


# ---- 5. the other ways to move a chain ---------------------------------------------------------------------------------------------
def test_records_between_heatbath_sweeps_and_reshuffles():
    m = _model(301, 203, 4, 6, 3000, 8)
    m.shuffle_bisbm()
    m.trace_set(2)
    hist = []
    for step in range(4):
        if step % 2:
            m.reshuffle(4)
        else:
            m.heatbath_sweeps(1)
        m.trace_record()
        now = _all_labels(m)
        vi_last = m._trace_raw()[2]
        for a in range(1, min(2, step) + 1):
            for c in range(8):
                ref = m.partition_distances_to(hist[step - a][c], chains=[c])[0][0, 0]
                assert _bits([vi_last[c, a - 1]])[0] == _bits([ref])[0], (step, c, a)
        hist.append(now)
    assert m.trace_lags()["records"] == 4


def test_chains_grouped_by_shape_are_recorded_each_in_its_own_shape():
    g = _mixed_shapes_model()
    shapes = [tuple(g.ka_kb(c)) for c in range(32)]
    assert len(set(shapes)) > 1
    g.trace_set(2)
    res = {}
    for name in ("fused", "split"):
        g.trace_reset()
        with regime(name):
            g.trace_record()
            then = _all_labels(g)
            g.trace_record()  # (no sweep between: the regimes see the same partitions)
        res[name] = g._trace_raw()
        assert (res[name][1][:, 0] == g.n).all()
    assert _same_raw(res["fused"], res["split"])
    g.run_sweeps(1)
    g.trace_record()
    now = _all_labels(g)
    vi_sum, agree_sum, vi_last, pairs, records = g._trace_raw()
    assert records == 3 and pairs.tolist() == [2, 1]
    for c in range(32):
        for a in (1, 2):
            ref = g.partition_distances_to(then[c], chains=[c], shapes=[shapes[c]])[0][0, 0]
            assert _bits([vi_last[c, a - 1]])[0] == _bits([ref])[0], (c, a)
            want = max(numpy_vi(now[c], then[c], sum(shapes[c]), sum(shapes[c])), 0.0)
            assert abs(vi_last[c, a - 1] - want) <= vi_tolerance(g.n, *shapes[c], *shapes[c]), (c, a)
        assert int(agree_sum[c, 1]) == int((now[c] == then[c]).sum())
    assert (_bits(g.trace_series("S")[-1]) == _bits(g.entropy())).all()
    assert (_bits(g.trace_series("H")[-1]) == _bits(g.partition_distances()[1])).all()


def test_every_chain_is_recorded_under_replica_exchange():
    m = _model(301, 203, 4, 6, 3000, 8)
    m.shuffle_bisbm()
    m.set_tempering([1.0, 1.5])
    m.trace_set(2)
    m.tempering_run(1, 1)
    m.trace_record()
    then = _all_labels(m)
    m.tempering_run(2, 1)
    m.trace_record()
    now = _all_labels(m)
    vi_sum, agree_sum, vi_last, pairs, records = m._trace_raw()
    assert records == 2 and not np.isnan(vi_last[:, 0]).any()  # every chain, whatever its rung
    for c in range(8):
        assert int(agree_sum[c, 0]) == int((now[c] == then[c]).sum())
        ref = m.partition_distances_to(then[c], chains=[c])[0][0, 0]
        assert _bits([vi_last[c, 0]])[0] == _bits([ref])[0]
    assert m.trace_series("S").shape == (2, 8) and (m.trace_series("S")[1] == m.entropy()).all()


# ---- 6. refusals and lifecycle ---------------------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(B.BisbmError) as e:
        call()
    return e.value.code, str(e.value)


def test_refusals_and_lifecycle():
    m = _model(300, 200, 4, 4, 3000, 4)
    assert _code(m.trace_record)[0] == B.BISBM_ERR_STATE  # no ring
    m.trace_set(3)
    code, msg = _code(m.trace_record)  # before init / shuffle
    assert code == B.BISBM_ERR_STATE and "bisbm_init or bisbm_shuffle" in msg
    assert _code(lambda: m.trace_set(1025))[0] == B.BISBM_ERR_INVALID_ARG
    m.trace_set(1024)
    m.trace_set(3)
    m.shuffle_bisbm()
    for _ in range(4):
        m.run_sweeps(1)
        m.trace_record()
    assert m.trace_lags()["records"] == 4 and m.trace_lags()["pairs"].tolist() == [3, 2, 1]
    # a merge changes every chain's shape: the held snapshots no longer compare
    m.agg_merge(1, 1, 10)
    assert tuple(m.ka_kb(0)) == (3, 3)
    code, msg = _code(m.trace_record)
    assert code == B.BISBM_ERR_STATE and "bisbm_trace_reset first" in msg
    assert m.trace_lags()["records"] == 4  # (a refused record changes nothing)
    m.trace_reset()
    lags = m.trace_lags()
    assert lags["records"] == 0 and (lags["pairs"] == 0).all() and np.isnan(lags["vi_last"]).all() and m.trace_series("S").shape == (0, 4)
    m.trace_record()
    m.run_sweeps(1)
    then = _all_labels(m)
    m.trace_record()
    m.run_sweeps(1)
    m.trace_record()
    vi_last = m._trace_raw()[2]
    assert _bits([vi_last[2, 0]])[0] == _bits([m.partition_distances_to(then[2], chains=[2])[0][0, 0]])[0]
    # a new depth forgets everything
    m.trace_set(2)
    lags = m.trace_lags()
    assert lags["records"] == 0 and lags["vi_sum"].shape == (4, 2) and (lags["vi_sum"] == 0).all() and (lags["agree_sum"] == 0).all()
    m.trace_record()
    # depth 0 frees the ring
    m.trace_set(0)
    assert _code(m.trace_record)[0] == B.BISBM_ERR_STATE
    assert _code(m.trace_lags)[0] == B.BISBM_ERR_STATE
    with pytest.raises(ValueError):
        m.trace_series("x")
    wide = _model(400, 300, 200, 100, 4000, 2)
    wide.shuffle_bisbm()
    assert _code(lambda: wide.trace_set(2))[0] == B.BISBM_ERR_UNSUPPORTED
    code, msg = _code(wide.trace_record)
    assert code == B.BISBM_ERR_UNSUPPORTED and "byte labels only" in msg


# ---- 7. the marginal driver ------------------------------------------------------------------------------------------------------------
def test_marginalize_records_after_every_sample_and_returns_what_it_did():
    out = []
    for trace in (None, 3):
        m = _model(301, 203, 4, 6, 3000, 4)
        m.shuffle_bisbm()
        out.append(mz.marginalize(m, 2, 6, 1, trace=trace))
        if trace:
            lags = m.trace_lags()
            assert lags["records"] == 6 and lags["pairs"].tolist() == [5, 4, 3]
            assert m.trace_series("S").shape == (6, 4) and (m.trace_series("S")[-1] == m.entropy()).all()
            tau, win, rhat = B.trace_summary(m.trace_series("S"))
            assert tau.shape == (4,) and win.shape == (4,)
    assert (out[0][0] == out[1][0]).all() and (out[0][1] == out[1][1]).all()
    m = _model(301, 203, 4, 6, 3000, 4)
    m.shuffle_bisbm()
    res = mz.marginalize_modes(m, 1, 3, 1, threshold=10.0, trace=2, sampler="heatbath")
    assert m.trace_lags()["records"] == 3 and res["counts"].sum() == 3 * 4 * m.n


def test_cli_trace_writes_what_the_driver_computes(tmp_path):
    na, nb, ka, kb, depth, samples = 600, 500, 4, 4, 3, 8
    n = na + nb
    a, b = syn.planted_edges(na, nb, 6000, ka, kb, seed=4)
    el = tmp_path / "planted.edgelist"
    np.savetxt(el, np.stack([a, b], axis=1), fmt="%d")
    truth = syn.contiguous_labels(na, nb, ka, kb)
    sizes = np.bincount(truth)
    rp, cl = B.edge_to_adj(B.load_edge_list(str(el)), n)
    m = B.BlockModel(truth, syn.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rp, cl), n_chains=16, seed=5, gen_seed=6)
    m.shuffle_bisbm()
    mz.marginalize(m, 3, samples, 1, trace=depth, sampler="heatbath")
    vi_sum, agree_sum, _, pairs, records = m._trace_raw()
    tau, win, rhat = B.trace_summary(m.trace_series("S"))
    out = tmp_path / "trace.txt"
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    r = subprocess.run([cli, "-e", str(el), "-y", str(na), str(nb), "-n", *map(str, sizes), "-z", str(ka), str(kb), "-E", "1", "-d", "5",
                        "--rng", "philox", "--chains", "16", "--randomize", "-b", str(3 * n), "-t", str(samples * n), "-f", str(n),
                        "--marginalize", "--heatbath", "--trace", str(out), str(depth)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "trace: %d record(s) of 16 chain(s), %d lag(s)" % (samples, depth) in r.stderr
    rows = [line.split() for line in out.read_text().splitlines()]
    assert [len(x) for x in rows] == [4] * depth + [2] * 16 + [1]
    for i in range(depth):  # means over the chains, added in chain order
        vi = agree = 0.0
        for c in range(16):
            vi += float(vi_sum[c, i])
            agree += float(agree_sum[c, i])
        den = float(pairs[i]) * 16.0
        assert (int(rows[i][0]), int(rows[i][1])) == (i + 1, samples - 1 - i)
        assert float(rows[i][2]) == vi / den and float(rows[i][3]) == 1.0 - agree / (den * float(n))
    assert [float(x[0]) for x in rows[depth:depth + 16]] == tau.tolist() and [int(x[1]) for x in rows[depth:depth + 16]] == win.tolist()
    assert float(rows[-1][0]) == rhat
    # stdout (the labels) is what the run prints without the flag
    plain = subprocess.run([x for x in r.args if x not in ("--trace", str(out), str(depth))], capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and plain.stdout == r.stdout
    m.close()


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "mixing.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "VI heatbath" in r.stdout and "tau_S" in r.stdout and "R-hat" in r.stdout
