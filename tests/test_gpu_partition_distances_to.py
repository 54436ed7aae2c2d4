"""GPU tests of the distances to reference partitions (include/bisbm.h, "Distances to reference partitions"): chains against
partitions that are no chains.  The reference is the numpy statement of tests/test_partition_distances.py (np.add.at tables,
fsum sums) fed with get_memberships(c) and the references themselves.  Bound: each of the three sums has at most 65 536 terms,
an f64 sum of that length is off by at most terms * 2^-53 relative, divided by n that leaves at most about
4 * 7.3e-12 * ln n < 3.5e-10 for n < 1e5; the shapes here have at most 24 400 cells, a third of that, hence 1e-10."""
import importlib

import numpy as np
import pytest

from test_anchored_modes import numpy_vi_to
from test_gpu_partition_distances import _model, regime
from test_partition_distances import numpy_entropy, random_labels, relabel

B = importlib.import_module("bipartitesbm-mcmc_amd")
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")
TOL = 1e-10

pytestmark = pytest.mark.gpu


def _all_labels(m):
    return np.array([m.get_memberships(c) for c in range(m.n_chains)])


CASES = [  # na, nb, ka, kb, edges, chains, rng, shapes of the references (None: the chains')
    (301, 203, 4, 6, 3000, 16, "philox", [None, (2, 3), None, (7, 2), None]),
    (301, 203, 4, 6, 3000, 16, "mt19937-compat", [None, (2, 3), None, (7, 2), None]),
    (1500, 1500, 32, 32, 20000, 16, "philox", [None, None, (5, 40), None, None]),
    (1000, 1000, 100, 120, 12000, 5, "philox", [None, (3, 2), None, None, (100, 120)]),  # one table fills a workgroup's LDS
    (601, 903, 2, 250, 8000, 5, "philox", [None, (2, 250), (4, 4), None, None]),        # a table larger than the LDS: HBM
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d+%d_n%d_%s" % (c[2], c[3], c[0] + c[1], c[6]))
def test_distances_to_references_against_numpy(case):
    na, nb, ka, kb, edges, chains, rng_mode, shapes = case
    m = _model(na, nb, ka, kb, edges, chains, rng=rng_mode)
    m.shuffle_bisbm()
    m.run_sweeps(1)
    labs = _all_labels(m)
    rng = np.random.default_rng(3)
    shapes = [(ka, kb) if s is None else s for s in shapes]
    refs = []
    for g, (rka, rkb) in enumerate(shapes):
        if (rka, rkb) == (ka, kb) and g % 2 == 0:
            refs.append(relabel(labs[g % chains], na, ka, kb, rng))  # a chain's partition in another numbering
        else:
            refs.append(random_labels(na, nb, rka, rkb, rng))
    refs = np.array(refs)
    want = numpy_vi_to(labs, refs, ka + kb, [sum(s) for s in shapes])
    want_h = np.array([numpy_entropy(r, sum(s)) for r, s in zip(refs, shapes)])
    worst = 0.0
    for n_sel in (1, 4, 5, 16):
        if n_sel > chains:
            continue
        sel = rng.permutation(chains)[:n_sel]
        for n_refs in (1, 4, 5):
            got = {}
            for name in ("fused", "split", None):
                with regime(name):
                    got[name] = m.partition_distances_to(refs[:n_refs], chains=sel, shapes=shapes[:n_refs])
            vi, H = got[None]
            assert vi.shape == (n_sel, n_refs) and H.shape == (n_refs,) and (vi >= 0.0).all()
            err = max(np.abs(vi - want[sel][:, :n_refs]).max(), np.abs(H - want_h[:n_refs]).max())
            worst = max(worst, err)
            print("n_sel %d n_refs %d: worst |VI - numpy|, |H - numpy| = %.3e" % (n_sel, n_refs, err))
            assert err <= TOL
            # both forms of the kernel reduce the same integer tables with the same function: the same bits
            for name in ("fused", "split"):
                assert (got[name][0] == vi).all() and (got[name][1] == H).all(), name
    print("worst over the case: %.3e (bound %.1e)" % (worst, TOL))
    # chains = None is every chain; a relabelled chain is its own partition
    vi_all, _ = m.partition_distances_to(refs, shapes=shapes)
    assert vi_all.shape == (chains, len(refs)) and np.abs(vi_all - want).max() <= TOL
    assert vi_all[0, 0] <= TOL
    # the same call, the same bits
    again, _ = m.partition_distances_to(refs, shapes=shapes)
    assert (again == vi_all).all()


def test_copies_of_the_chains_agree_with_the_square_call():
    m = _model(301, 203, 4, 6, 3000, 16)
    m.shuffle_bisbm()
    m.run_sweeps(1)
    labs = _all_labels(m)
    square, H = m.partition_distances()
    vi, H_ref = m.partition_distances_to(labs)
    print("worst |to - square| = %.3e, worst diagonal %.3e" % (np.abs(vi - square).max(), np.diag(vi).max()))
    assert np.abs(vi - square).max() <= TOL and np.abs(H_ref - H).max() <= TOL
    assert np.diag(vi).max() < TOL and np.abs(vi - vi.T).max() <= TOL
    sub = [9, 2, 14]
    vs, _ = m.partition_distances_to(labs[[4, 9]], chains=sub)
    assert np.abs(vs - square[np.ix_(sub, [4, 9])]).max() <= TOL


def test_state_is_untouched():
    def run(call):
        m = _model(800, 601, 6, 6, 8000, 12)
        m.shuffle_bisbm()
        m.run_sweeps(2)
        if call:
            before = (_all_labels(m), m.get_entropy().copy())
            m.partition_distances_to(before[0][:5])
            m.partition_distances_to(before[0][:1], chains=[3, 1])
            after = (_all_labels(m), m.get_entropy())
            assert all((x == y).all() for x, y in zip(before, after))
        rates = m.run_sweeps(1)
        return _all_labels(m), m.get_entropy(), rates, np.array([m.get_m(c) for c in range(12)])
    plain, called = run(False), run(True)
    assert all((x == y).all() for x, y in zip(plain, called))


def test_two_device_entries_equal_one_handle_bit_for_bit():
    res = []
    rng = np.random.default_rng(4)
    refs = np.array([random_labels(900, 701, 6, 5, rng) for _ in range(5)])
    for devices in (None, [0, 0]):
        kw = {} if devices is None else {"devices": devices}
        m = _model(900, 701, 6, 5, 9000, 10, **kw)
        m.shuffle_bisbm()
        m.run_sweeps(2)
        res.append((m.partition_distances_to(refs), m.partition_distances_to(refs[:2], chains=[9, 0, 6, 3])))
        m.close()
    one, two = res
    for x, y in zip(one, two):
        assert (x[0] == y[0]).all() and (x[1] == y[1]).all()


def test_replica_exchange_on():
    m = _model(301, 203, 4, 6, 3000, 8)
    m.shuffle_bisbm()
    m.set_tempering([1.0, 1.5])
    m.tempering_run(2, 1)
    labs = _all_labels(m)
    refs = labs[[1, 6]]
    vi, _ = m.partition_distances_to(refs)
    assert np.abs(vi - numpy_vi_to(labs, refs, 10)).max() <= TOL  # (every selected chain, whatever its rung)


def _refused(code, text, call, *args, **kw):
    with pytest.raises(B.BisbmError) as e:
        call(*args, **kw)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_refusals():
    STATE, INVALID, UNSUPPORTED = B.BISBM_ERR_STATE, B.BISBM_ERR_INVALID_ARG, B.BISBM_ERR_UNSUPPORTED
    wide = _model(400, 300, 200, 100, 4000, 2)
    wide.shuffle_bisbm()
    _refused(UNSUPPORTED, "byte labels only", wide.partition_distances_to, syn.contiguous_labels(400, 300, 4, 4), shapes=(4, 4))
    wide.close()
    m = _model(300, 200, 4, 4, 3000, 4)
    ref = syn.contiguous_labels(300, 200, 4, 4)
    _refused(STATE, "bisbm_init", m.partition_distances_to, ref)
    m.shuffle_bisbm()
    _refused(INVALID, "chain 2 is listed twice", m.partition_distances_to, ref, chains=[0, 2, 1, 2])
    _refused(INVALID, "out of range", m.partition_distances_to, ref, chains=[0, 4])
    _refused(INVALID, "no chain selected", m.partition_distances_to, ref, chains=[])
    _refused(INVALID, "n_refs = 0", m.partition_distances_to, np.zeros((0, 500), dtype=np.uint32))
    _refused(INVALID, "reference 0 has 200 + 57 blocks", m.partition_distances_to, ref, shapes=(200, 57))
    bad = np.array([ref, ref])
    bad[1, 310] = 3  # a type-b node with a type-a label
    _refused(INVALID, "reference 1: label 3 of node 310", m.partition_distances_to, bad)
    bad[1, 310] = 8
    _refused(INVALID, "reference 1: label 8 of node 310", m.partition_distances_to, bad)
    L = B.lib()
    out = np.zeros(4)
    k = np.array([4], dtype=np.uint32)
    assert L.bisbm_partition_distances_to(m._h, 4, None, 1, None, B._p(k, B._u32p), B._p(k, B._u32p), B._p(out, B._f64p), None) == INVALID
    assert L.bisbm_partition_distances_to(m._h, 4, None, 1, B._p(ref, B._u32p), B._p(k, B._u32p), B._p(k, B._u32p), None, None) == INVALID
    assert L.bisbm_partition_distances_to(m._h, 3, None, 1, B._p(ref, B._u32p), B._p(k, B._u32p), B._p(k, B._u32p), B._p(out, B._f64p), None) == INVALID
    vi, _ = m.partition_distances_to(ref)  # ... and the handle still serves
    assert vi.shape == (4, 1)
