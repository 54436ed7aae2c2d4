"""Block fields on the device (include/bisbm.h, "Block fields"): every sampler targets exp(-beta (S + Phi)).  Heat-bath sweeps and
pair reshuffles against host replays fed the model's rows plus the field, MH sweeps against a replay built from the oracle's
proposal and transition ratio, the stationary distribution over an enumerable state space, Phi itself bit for bit, replica
exchange and resampling on E = S + Phi, and the plumbing: device entries, refusals, clearing, the command line, marginalize."""
import importlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import oracle_lib as O
import test_gpu_constraints as TC
from test_gpu_constraints import ENUM_LISTS, FIRST_ID, INF, LOW_T, SEED, _code, _enumeration, _one_start, _pair_rows, _same_state, _state
from test_gpu_heatbath import _assert_state_is_a_rebuild, _bits, _case, _model, _refused
from mh_replay import mh_replay_sweep as _mh_replay_sweep  # (the shared host replay of one held MH sweep)
from test_tempering import exchange_round, philox, u53

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _every_launch_keeps_its_own_sum(monkeypatch):
    """the unfielded MH sweeps of these tests keep the sum of their own dS values (tests/test_gpu_heatbath.py does the same)"""
    monkeypatch.setenv("BISBM_KEEP_SUM", "1")


def _visit(gid, sweep, na, nb, seed=SEED):
    L = O.lib()
    return [int(L.orc_philox_visit(seed, gid, sweep, na, nb, i)) for i in range(na + nb)]


def _table(n_classes, K, seed, scale=1.0):
    """a table of entries of about `scale` nats; row 0 is the zero row"""
    field = np.random.default_rng(seed).normal(scale=scale, size=(n_classes, K))
    field[0] = 0.0
    return field


def _phi(m, c, cls, field, na, ka):
    return B.numpy_field_energy(m.get_memberships(c), cls, field, na, ka)


# ------------------------------------------------------------------------------------------------------- 1. heat bath
def _heatbath_replay(name, sweeps, make, beta=1.0, constraints=None, clamp=None):
    """tests/test_gpu_constraints.py::_heatbath_replay under fields: chain 2 of a three-chain handle with first chain id 5, after a
    shuffle and three unfielded MH sweeps, every chain set to chain 2's labels; make(visit order of the first replayed sweep,
    labels) -> (class_of_node, field).  The model's rows come from a one-chain helper's conditionals_last, go through
    numpy_field_row, the weights are built on the host with the device's exp and the choice is numpy_heatbath_choice.
    constraints(order, labels) -> (class_of_node, allowed) and clamp(order, labels) -> mask go on top."""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, chains, greedy = na + nb, 3, beta == INF
    m = _model(name, chains, first_chain_id=FIRST_ID)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    c, gid, sweep0 = chains - 1, FIRST_ID + chains - 1, 3
    lab = _one_start(m, c)
    first_order = _visit(gid, sweep0, na, nb)
    cls, field = make(first_order, lab.copy())
    cls, field = np.asarray(cls, dtype=np.uint8), np.asarray(field, dtype=np.float64)
    mask = np.zeros(n, dtype=bool) if clamp is None else np.asarray(clamp(first_order, lab.copy()), dtype=bool)
    if constraints is None:
        cn_cls, allowed = np.zeros(n, dtype=np.uint8), np.ones((1, ka + kb), dtype=bool)
    else:
        cn_cls, allowed = constraints(first_order, lab.copy())
        cn_cls, allowed = np.asarray(cn_cls, dtype=np.uint8), np.asarray(allowed, dtype=bool)
        m.constrain(cn_cls, allowed)
    if mask.any():
        m.clamp(mask)
    m.set_fields(cls, field)
    got_cls, got_field = m.fields()
    assert (got_cls == cls).all() and got_field.tobytes() == field.tobytes()
    start = lab.copy()
    cum0, S0 = m.get_entropy()[c], m.entropy()[c]
    phi0 = m.field_energy()[c]
    assert _bits(phi0) == _bits(_phi(m, c, cls, field, na, ka))
    cum = cum0
    helper = _model(name, 1, labels=lab.astype(np.uint32))
    helper.conditionals_set(None, 1.0 if greedy else beta, keep_last=True)

    def sync():
        helper.set_memberships(lab.astype(np.uint32))
        helper.init_bisbm()
        helper.conditionals_accumulate()
    sync()
    if greedy:
        moved_gpu, sweeps_gpu = m.polish(sweeps)
    else:
        moved_gpu, sweeps_gpu = m.heatbath_sweeps(sweeps, beta), None
    seen = {"free": 0, "fielded": 0, "second_chunk": 0, "type_b_last_class": 0, "min_moved": 0, "restricted": 0}
    moved, total, ran = 0, 0.0, 0
    for sw in range(sweeps):
        order = first_order if sw == 0 else _visit(gid, sweep0 + sw, na, nb)
        moved_before = moved
        for pos, v in enumerate(order):
            k_own, lo = (ka, 0) if v < na else (kb, ka)
            r = int(lab[v]) - lo
            A = allowed[cn_cls[v], lo:lo + k_own].copy()
            free = k_own > 1 and int((lab == lab[v]).sum()) > 1 and not mask[v] and A.sum() > 1
            dS = np.asarray(helper.conditionals_last(v)[0][0][:k_own], dtype=np.float64)
            f_own = field[cls[v], lo:lo + k_own]
            dE = B.numpy_field_row(dS, r, f_own)
            P = np.zeros(k_own)
            if free and not greedy:
                x = beta * (dE - dE[A].min())
                w = np.where((x > 700.0) | ~A, 0.0, m.debug_exp(-np.minimum(x, 700.0)))
                Z = 0.0
                for y in w:
                    Z = Z + float(y)
                P = w / Z
            if free:
                seen["free"] += 1
                seen["fielded"] += bool(f_own.any())
                seen["restricted"] += not A.all()
                seen["second_chunk"] += bool(k_own > 64 and (f_own[64:] != f_own[r]).any())
                seen["type_b_last_class"] += bool(v >= na and cls[v] == len(field) - 1)
                seen["min_moved"] += bool(int(np.argmin(np.where(A, dE, INF))) != int(np.argmin(np.where(A, dS, INF))))
            o = philox(SEED, gid, B.PHILOX_PURPOSE_HEATBATH, (sweep0 + sw) * n + pos)
            s = D.numpy_heatbath_choice(dE, P, r, free, u53(o[0], o[1]), greedy, allowed=None if constraints is None else A)
            if s != r:
                lab[v] = lo + s
                cum = cum + dE[s]
                total = total + dE[s]
                moved += 1
                sync()
        ran += 1
        if greedy and moved == moved_before:
            break
    assert seen["free"] > 0 and seen["fielded"] > 0 and moved > 0, (seen, moved)
    got = m.get_memberships(c)
    assert (got[mask] == start[mask]).all()
    assert (got == lab).all(), np.flatnonzero(got != lab)
    assert int(moved_gpu[c]) == moved
    if greedy:
        assert int(sweeps_gpu[c]) == ran
    acc, sw_counts = m.last_counts()
    assert int(acc[c]) == moved and int(sw_counts[c]) == ran
    for x, y in zip(_state(m, c)[1:], _state(helper, 0)[1:]):
        assert (x == y).all()
    assert _bits(m.get_entropy()[c]) == _bits(cum)
    S1, phi1 = m.entropy()[c], m.field_energy()[c]
    assert _bits(phi1) == _bits(B.numpy_field_energy(lab, cls, field, na, ka))
    print("%s beta %g: %d moves in %d sweep(s), sum dE %.6f, dS %.6f, dPhi %.6f, %s" % (name, beta, moved, ran, total, S1 - S0, phi1 - phi0, seen))
    assert abs((m.get_entropy()[c] - cum0) - ((S1 - S0) + (phi1 - phi0))) <= 1e-9 * abs(S0)  # delta cum = delta S + delta Phi
    assert allowed[cn_cls, got].all()
    for other in range(chains - 1):
        _assert_state_is_a_rebuild(m, rowptr, col, other)
    m.close()
    helper.close()
    seen.update(order=first_order, cls=cls, field=field, mask=mask, start=start, final=lab)
    return seen


def test_heat_bath_sweeps_on_the_tiny_graph_are_the_host_replay():
    """12 + 9 nodes, 3 + 2 blocks, three classes"""
    seen = _heatbath_replay("tiny", 3, lambda order, lab: (np.arange(21) % 3, _table(3, 5, 1)))
    assert seen["min_moved"] > 0


def test_heat_bath_sweep_with_a_skipped_chunk_constraints_and_a_clamp_on_top_is_the_host_replay():
    """300 + 200 nodes: the one-block classes of tests/test_gpu_constraints.py hold the positions 64 .. 127 (a skipped chunk), every
    fifth node is clamped, and every node has one of five field classes"""
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    deg = np.diff(rowptr.astype(np.int64))
    seen = _heatbath_replay(name, 1, lambda order, lab: (np.arange(na + nb) % 5, _table(5, ka + kb, 2)),
                            constraints=lambda order, lab: TC._chunk_classes(order, lab, na, nb, ka, kb, deg),
                            clamp=lambda order, lab: np.arange(na + nb) % 5 == 0)
    assert seen["restricted"] > 0 and seen["mask"].sum() == 100


def test_heat_bath_sweep_with_a_skipped_chunk_is_the_host_replay():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    seen = _heatbath_replay(name, 1, lambda order, lab: (np.arange(na + nb) % 4, _table(4, ka + kb, 3)),
                            clamp=lambda order, lab: np.isin(np.arange(na + nb), order[64:128]))
    assert seen["mask"].sum() == 64 and seen["min_moved"] > 0


def test_heat_bath_sweep_over_70_blocks_reads_the_last_class_row_in_the_second_lane_chunk():
    """70 + 3 blocks: the type-b nodes and every second type-a node are of the last class, whose row ends the allocation"""
    name = "wideK"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)

    def make(order, lab):
        cls = np.where((np.arange(na + nb) >= na) | (np.arange(na + nb) % 2 == 0), 255, 1)
        return cls, _table(256, ka + kb, 4)
    seen = _heatbath_replay(name, 1, make)
    assert seen["second_chunk"] > 3 and seen["type_b_last_class"] > 0


def test_64_and_65_targets_under_fields_are_the_host_replay():
    name = "hb_k64_k65"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    seen = _heatbath_replay(name, 1, lambda order, lab: (1 + np.arange(na + nb) % 2, _table(3, ka + kb, 5)))
    assert seen["second_chunk"] >= 1 and seen["type_b_last_class"] > 0


def test_greedy_moves_follow_the_field_and_polish_ends_at_a_minimum_of_E():
    """40 nodes get a field that makes another block the minimum of E but not of S: they move there, and polish ends with no open
    admissible move of negative dE"""
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    m = _model(name, 2)
    m.shuffle_bisbm()
    m.run_sweeps(1)
    _one_start(m, 0)
    m.polish(100)  # (a minimum of S: no free node has a downhill move)
    lab = _one_start(m, 0)
    m.conditionals_set(None, 1.0, keep_last=True)
    m.conditionals_accumulate()
    sizes = np.bincount(lab, minlength=ka + kb)
    picked, cls, rows = [], np.zeros(n, dtype=np.uint8), [np.zeros(ka + kb)]
    for v in range(n):
        lo, k = (0, ka) if v < na else (ka, kb)
        dS = np.asarray(m.conditionals_last(v)[0][0][:k])
        r = lab[v] - lo
        if len(picked) == 40 or sizes[lab[v]] < 45 or k < 2:  # (40 nodes may leave and the block stays held)
            continue
        assert (np.delete(dS, r) >= 0).all()
        s = (r + 1) % k
        row = np.zeros(ka + kb)
        row[lo + s] = -(dS[s] + 1e6)  # dE_s = dS_s + f_s = -1e6: the minimum of E, not of S, whatever the moves before it shift
        picked.append((v, lo + s))
        cls[v] = len(rows)
        rows.append(row)
    assert len(picked) == 40
    field = np.array(rows)
    m.set_fields(cls, field)
    moved, sweeps = m.polish(100)
    assert (sweeps < 100).all() and (moved >= 1).all()
    m.conditionals_accumulate()
    for c in range(2):
        after = m.get_memberships(c).astype(np.int64)
        free = np.bincount(after, minlength=ka + kb)[after] > 1
        for v in range(n):
            lo, k = (0, ka) if v < na else (ka, kb)
            dE = B.numpy_field_row(np.asarray(m.conditionals_last(v)[0][c][:k]), after[v] - lo, field[cls[v], lo:lo + k])
            assert not (free[v] and (dE < 0).any()), (c, v)
        _assert_state_is_a_rebuild(m, rowptr, col, c)
    # the first greedy sweep alone: every picked node goes to its block
    one = _model(name, 1, labels=lab.astype(np.uint32))
    one.init_bisbm()
    one.set_fields(cls, field)
    one.polish(1)
    got = one.get_memberships(0)
    assert all(int(got[v]) == s for v, s in picked)
    one.close()
    m.close()


# ------------------------------------------------------------------------------------------------------- 2. reshuffles
class _EnergyView:
    """the model with entropy() = S + Phi: what the running sum follows under fields"""

    def __init__(self, m):
        self._m = m

    def __getattr__(self, name):
        return getattr(self._m, name)

    def entropy(self):
        return self._m.entropy() + self._m.field_energy()


@pytest.mark.parametrize("name,moves,scans", [("tiny", 4, 1), ("hubs_isolated", 2, 3)])
def test_reshuffles_are_the_host_replay_on_member_dE(name, moves, scans, monkeypatch):
    """tests/test_gpu_constraints.py::_reshuffle_replay with every member's dS_o replaced by dS_o + (f[o] - f[c]): records equal"""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    chains, c = 3, 2
    m = _model(name, chains, first_chain_id=FIRST_ID)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    _one_start(m, c)
    cls, field = np.arange(na + nb) % 4, _table(4, ka + kb, 6)
    m.set_fields(cls, field)
    differs = []

    class FieldHelper(TC._Helper):
        def dS(self, lab, v, o_loc):
            plain = super().dS(lab, v, o_loc)
            lo = 0 if v < na else ka
            f = field[cls[v]]
            differs.append(f[lo + o_loc] != f[int(lab[v])])
            return plain + (float(f[lo + o_loc]) - float(f[int(lab[v])]))
    monkeypatch.setattr(TC, "_Helper", FieldHelper)
    S0, phi0, cum0 = m.entropy()[c], m.field_energy()[c], m.get_entropy()[c]
    out = TC._reshuffle_replay(_EnergyView(m), c, FIRST_ID + c, name, moves, scans, 1.0, np.zeros(na + nb, dtype=np.int64), np.ones((1, ka + kb), dtype=bool))
    assert any(x["M"] >= 2 for x in out) and any(differs)
    S1, phi1 = m.entropy()[c], m.field_energy()[c]
    assert _bits(phi1) == _bits(_phi(m, c, cls, field, na, ka))
    assert abs((m.get_entropy()[c] - cum0) - ((S1 - S0) + (phi1 - phi0))) <= 1e-9 * abs(S0)
    for other in range(chains - 1):
        _assert_state_is_a_rebuild(m, rowptr, col, other)
    m.close()


# ------------------------------------------------------------------------------------------------------- 3. MH sweeps
MH_SEED = 21  # chosen on the host (mh_replay_margin below): no accept test of the 40 replayed sweeps is closer than 1e-9
MH_BASE = 3


def _mh_field(na, nb, ka, kb):
    return np.arange(na + nb) % 4, _table(4, ka + kb, 7, scale=1.5)


def _mh_replay(exp, device=None):
    """hubs_isolated, chain 2 of three with first id 5: 3 unfielded sweeps from the contiguous labels (the oracle's own), then 20
    sweeps at T = 1 and 20 at the low T under the field.  With `device` (the handle) every sweep is compared."""
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, c = na + nb, 2
    gid = FIRST_ID + c
    cls, field = _mh_field(na, nb, ka, kb)
    o = O.OracleModel(rowptr, col, na, nb, ka, kb, eps, O.contiguous_labels(na, nb, ka, kb))
    o.seed_philox(MH_SEED, gid)
    o.init_bisbm()
    o.anneal("constant", [1.0], MH_BASE * n, 1 << 60)
    lab = o.memberships().astype(np.int64)
    probe = O.OracleModel(rowptr, col, na, nb, ka, kb, eps, O.contiguous_labels(na, nb, ka, kb))
    margin, sweeps_that_differ = INF, 0
    for k in range(40):
        T = 1.0 if k < 20 else LOW_T
        lab, accepted, mg, differs = _mh_replay_sweep(probe, lab, cls, field, gid, MH_BASE + k, T, na, nb, ka, MH_SEED, exp)
        margin = min(margin, mg)
        sweeps_that_differ += differs
        if device is not None:
            S0, phi0, cum0 = device.entropy()[c], device.field_energy()[c], device.get_entropy()[c]
            device.run_sweeps(1, temperature=T)
            assert (device.get_memberships(c) == lab).all(), k
            assert int(device.last_counts()[0][c]) == accepted, k
            S1, phi1 = device.entropy()[c], device.field_energy()[c]
            assert abs((device.get_entropy()[c] - cum0) - ((S1 - S0) + (phi1 - phi0))) <= 1e-9 * abs(S0), k
    return margin, sweeps_that_differ


def test_mh_sweeps_under_fields_are_the_replay_built_from_the_oracle():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    # the condition on the seed, with the host's exp (it needs no device): no step's two sides lie within a relative 1e-9, so
    # neither the last bits of an exponential nor u accu0 < accu1 e against u < (accu1 / accu0) e can turn a decision
    margin, differ = _mh_replay(math.exp)
    assert margin > 1e-9, margin
    assert differ >= 5, differ
    m = _model(name, 3, seed=MH_SEED, first_chain_id=FIRST_ID)
    m.init_bisbm()
    m.run_sweeps(MH_BASE)
    cls, field = _mh_field(na, nb, ka, kb)
    m.set_fields(cls, field)
    margin_dev, differ_dev = _mh_replay(lambda x: float(m.debug_exp([float(x)])[0]), device=m)
    assert margin_dev > 1e-9 and differ_dev >= 5
    print("MH under fields: 40 sweeps equal the replay; smallest relative margin %.3g, %d sweeps decide differently from dS alone" % (margin_dev, differ_dev))
    for other in range(2):
        _assert_state_is_a_rebuild(m, rowptr, col, other)
    m.close()


def test_rows_constant_over_each_type_run_the_field_instances_and_change_nothing():
    """f[s] - f[r] = 0 exactly: the fielded handle equals the plain oracle chain label for label over 30 MH sweeps, and an unfielded
    handle through heat-bath and reshuffle calls; field_energy() is the numpy loop's bits meanwhile"""
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, chains = na + nb, 2
    field = np.zeros((3, ka + kb))
    for k, (a, b) in enumerate(((0.75, -1.25), (2.5, 0.125), (-3.0, 1e-3))):
        field[k, :ka], field[k, ka:] = a, b
    cls = np.arange(n) % 3
    m, plain = _model(name, chains, first_chain_id=FIRST_ID), _model(name, chains, first_chain_id=FIRST_ID)
    for g in (m, plain):
        g.shuffle_bisbm()
    m.set_fields(cls, field)
    assert m.fields()[1].tobytes() == field.tobytes()
    orc = []
    for c in range(chains):
        o = O.OracleModel(rowptr, col, na, nb, ka, kb, eps, O.contiguous_labels(na, nb, ka, kb))
        o.seed_philox(SEED, FIRST_ID + c)
        o.shuffle_bisbm()
        orc.append(o)
    for sweep in range(30):
        m.run_sweeps(1)
        for c, o in enumerate(orc):
            o.anneal("constant", [1.0], n, 1 << 60)
            assert (o.memberships() == m.get_memberships(c)).all(), (sweep, c)
            assert int(m.last_counts()[0][c]) == o.last_accepted
        assert m.last_pass_steps() == 1  # (the generic kernel)
    plain.run_sweeps(30)
    for call in (lambda g: g.heatbath_sweeps(2, 1.0), lambda g: g.reshuffle(3, 2, 1.0), lambda g: g.polish(3)[0]):
        a, b = call(m), call(plain)
        assert (np.asarray(a) == np.asarray(b)).all()
        for c in range(chains):
            assert _same_state(_state(m, c), _state(plain, c))
            assert _bits(m.field_energy()[c]) == _bits(_phi(m, c, cls, field, na, ka))
    assert (_bits(m.get_entropy()) == _bits(plain.get_entropy())).all()
    assert (plain.field_energy() == 0.0).all()
    m.close()
    plain.close()


# ------------------------------------------------------------------------------------------ 4. stationary distribution
def _enum_field():
    """the enumerable graph under ENUM_LISTS: the two-choice nodes 0 .. 3 and the free nodes 8 .. 11 get a class each, with entries
    of about 1 nat on the blocks they may sit in; chosen on the host so that the chi-square against exp(-beta S) has power"""
    rng = np.random.default_rng(11)
    cls = np.zeros(12, dtype=np.uint8)
    rows = [np.zeros(5)]
    for v in (0, 1, 2, 3, 8, 9, 10, 11):
        row = np.zeros(5)
        blocks = ENUM_LISTS.get(v, [3, 4])
        row[blocks] = rng.choice([-1.0, 1.0], size=len(blocks)) * rng.uniform(0.7, 1.3, size=len(blocks))
        cls[v] = len(rows)
        rows.append(row)
    return cls, np.array(rows)


def _enum_targets(beta):
    states, S = _enumeration()
    cls, field = _enum_field()
    digits = (states[:, None] // 3 ** np.arange(12)) % 3
    labels = np.concatenate([digits[:, :6], digits[:, 6:] + 3], axis=1)
    Phi = np.array([B.numpy_field_energy(lab, cls, field, cases.ENUM_NA, 3) for lab in labels])
    E = S + Phi
    p_E = np.exp(-beta * (E - E.min()))
    p_S = np.exp(-beta * (S - S.min()))
    return states, p_E / p_E.sum(), p_S / p_S.sum()


@pytest.mark.parametrize("sampler,beta", [("mh", 1.0), ("mh", 5.0 / 3.0), ("heatbath", 1.0), ("reshuffle", 1.0)])
def test_fielded_chains_sample_exp_minus_beta_E(sampler, beta):
    rowptr, col = cases.enumerable_graph()
    na, nb = cases.ENUM_NA, cases.ENUM_NB
    chains, moves = 8192, 400
    states, p_E, p_S = _enum_targets(beta)
    power = chains * float(((p_E - p_S) ** 2 / p_S).sum())
    assert power >= 10 * (len(states) - 1), power  # (so that the second assertion below can fail a sampler that ignores the field)
    cn_cls, allowed = B.constraints_from_lists(na + nb, 5, ENUM_LISTS, na=na, ka=3)
    cls, field = _enum_field()
    start = B.admissible_start(na, nb, 3, 2, cn_cls, allowed)
    g = B.BlockModel(start, syn.types_vector(na, nb), 5, 3, 2, cases.ENUM_EPS, (rowptr, col), n_chains=chains, rng="philox", seed=4242)
    g.constrain(cn_cls, allowed)
    g.set_fields(cls, field)
    g.shuffle_bisbm()
    if sampler == "mh":
        g.run_sweeps(moves, temperature=1.0 / beta)
    elif sampler == "heatbath":
        g.heatbath_sweeps(moves, beta)
    else:
        g.reshuffle(moves, 1, beta)
    codes = np.array([_code(g.get_memberships(c)) for c in range(chains)])
    g.close()
    stat, dof, p = cases.chi_square(codes, states, p_E)
    p_plain = cases.chi_square(codes, states, p_S)[2]
    print("%s under fields, beta = %g: chi2 = %.1f on %d dof, p = %.3g; against exp(-beta S) p = %.3g (power %.0f)" % (sampler, beta, stat, dof, p, p_plain, power))
    assert p > 1e-3, (stat, dof, p)
    assert p_plain < 1e-6


# ------------------------------------------------------------------------------------------------------------- 5. Phi
def test_field_energy_is_the_numpy_loop_bit_for_bit():
    """3 classes with one empty on the tiny graph; 256 classes x 73 blocks on wideK, which does not fit one LDS tile (the classes
    are walked in tiles of 112), with nodes in the first and the last class of a tile"""
    for name, n_classes, used in (("tiny", 3, [0, 2]), ("wideK", 256, [0, 1, 111, 112, 113, 223, 224, 255])):
        (rowptr, col), na, nb, ka, kb, eps = _case(name)
        n, chains = na + nb, 5
        field = _table(n_classes, ka + kb, 8, scale=1e3) + 1.0 / 3.0  # (entries whose sum rounds at every add)
        cls = np.asarray(used)[np.random.default_rng(9).integers(0, len(used), n)]
        m = _model(name, chains, first_chain_id=FIRST_ID)
        m.shuffle_bisbm()
        assert (m.field_energy() == 0.0).all()
        m.set_fields(cls, field)
        for _ in range(2):
            got = m.field_energy()
            want = [_phi(m, c, cls, field, na, ka) for c in range(chains)]
            assert (_bits(got) == _bits(want)).all(), (name, got, want)
            assert len(set(got.tolist())) > 1
            m.heatbath_sweeps(1, 1.0)
        m.close()


# ------------------------------------------------------------------------------------------------- 6. replica exchange
def _sw_model(n_chains, first_id, cls, field, seed=SEED):
    rowptr, col, na, nb = O.load_graph("southernWomen")
    lab0 = O.contiguous_labels(na, nb, 3, 3)
    m = B.BlockModel(lab0, syn.types_vector(na, nb), 6, 3, 3, 0.001, (rowptr, col), n_chains=n_chains, seed=seed, first_chain_id=first_id)
    m.init_bisbm()
    m.set_fields(cls, field)
    m.shuffle_bisbm()
    return m


def test_replica_exchange_rounds_under_fields_are_the_one_chain_handles():
    """the construction of tests/test_gpu_constraints.py: 4 chains as 2 ensembles of 2 rungs, 3 rounds of {1 MH sweep, 1 heat-bath
    sweep, 1 reshuffle}, every chain against the one-chain handle of its global id with the same fields"""
    cls, field = np.arange(32) % 3, _table(3, 6, 12)
    ladder, chains, first = [1.0, 1.5], 4, 4
    m = _sw_model(chains, first, cls, field)
    ones = [_sw_model(1, first + c, cls, field) for c in range(chains)]
    m.set_tempering(ladder)
    for r in range(3):
        T_now = m.tempering_state()[1]
        m.tempering_rounds(1, mh=1, heatbath=1, reshuffles=1, scans=1)
        for c, one in enumerate(ones):
            T = float(T_now[c])
            one.run_sweeps(1, temperature=T)
            one.heatbath_sweeps(1, 1.0 / T)
            one.reshuffle(1, 1, 1.0 / T)
            assert _same_state(_state(m, c), _state(one, 0)), (r, c)
            assert _bits(m.get_entropy())[c] == _bits(one.get_entropy())[0], (r, c)
    for x in ones + [m]:
        x.close()


def test_swaps_are_decided_on_E():
    """the host model of tests/test_tempering.py fed E = entropy() + field_energy() gives the rungs and the counters; fed S alone it
    decides at least one swap differently"""
    rowptr, col, na, nb = O.load_graph("southernWomen")
    cls = np.arange(na + nb) % 4
    field = _table(4, 6, 13, scale=3.0)
    L, chains, s = 4, 8, 1
    ladder = [1.0, 1.2, 1.6, 2.5]
    m = _sw_model(chains, 0, cls, field)
    m.set_tempering(ladder)
    rung = np.array([c % L for c in range(chains)], dtype=np.uint32)
    att, acc = np.zeros(L - 1, dtype=np.uint64), np.zeros(L - 1, dtype=np.uint64)
    differ = 0
    for r in range(12):
        m.tempering_run(s, s)
        S, Phi = m.entropy(), m.field_energy()
        for c in range(chains):
            assert _bits(Phi[c]) == _bits(_phi(m, c, cls, field, na, 3))
        on_S = rung.copy()
        exchange_round(on_S, S, ladder, SEED, 0, r, att.copy(), acc.copy())
        exchange_round(rung, S + Phi, ladder, SEED, 0, r, att, acc)
        differ += int((on_S != rung).any())
        got_rung, got_T = m.tempering_state()
        assert (got_rung == rung).all(), (r, got_rung, rung)
        a2, c2, rounds = m.tempering_stats()
        assert (a2 == att).all() and (c2 == acc).all() and rounds == r + 1
    print("exchange on E: %d of 12 rounds differ from the rounds S alone decides; accepted %s of %s" % (differ, acc, att))
    assert differ >= 1 and acc.sum() > 0
    m.close()


# ------------------------------------------------------------------------------------------------------- 7. population
def test_a_resampling_step_weighs_E_and_a_slot_carries_its_ancestors_phi():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    chains = 16
    cls, field = np.arange(na + nb) % 4, _table(4, ka + kb, 14, scale=2.0)
    m = _model(name, chains)
    m.init_bisbm()
    m.set_fields(cls, field)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    S, Phi = m.entropy(), m.field_energy()
    E = S + Phi
    delta = (1.0 + 1.0 / E.std()) - 1.0  # (what the step sees of it)
    o = philox(SEED, 0, 8, 0)  # (purpose 8: the resampling step's uniform, as tests/test_gpu_population.py draws it)
    u = u53(o[0], o[1])
    _, want, log_ratio = B.population_offspring(E, delta, u)
    _, on_S, _ = B.population_offspring(S, delta, u)
    assert (want != on_S).any()  # (the field changes who survives)
    parent, got_ratio = m.population_resample(1.0, 1.0 + delta)
    assert (parent == want).all() and _bits(got_ratio) == _bits(log_ratio)
    assert len(set(parent.tolist())) < chains
    after = m.field_energy()
    for c in range(chains):
        assert _bits(after[c]) == _bits(Phi[int(parent[c])]), c
    m.close()


# --------------------------------------------------------------------------------------------------------- 8. plumbing
def _calls(m):
    """MH, heat-bath and reshuffle calls: labels, counts and the running sums after each"""
    out = []
    m.run_sweeps(1)
    out.append(([m.get_memberships(c) for c in range(m.n_chains)], m.last_counts()[0].copy(), _bits(m.get_entropy()).copy(), _bits(m.field_energy()).copy()))
    moved = m.heatbath_sweeps(1, 1.0)
    out.append(([m.get_memberships(c) for c in range(m.n_chains)], moved, _bits(m.get_entropy()).copy(), _bits(m.field_energy()).copy()))
    acc = m.reshuffle(2, 1, 1.0)
    out.append(([m.get_memberships(c) for c in range(m.n_chains)], acc, _bits(m.get_entropy()).copy(), _bits(m.field_energy()).copy()))
    return out


def _same_calls(a, b):
    for (l1, n1, s1, p1), (l2, n2, s2, p2) in zip(a, b):
        assert all((x == y).all() for x, y in zip(l1, l2)) and (n1 == n2).all() and (s1 == s2).all() and (p1 == p2).all()


def test_device_entries_behind_one_handle_and_a_refused_set():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    cls, field = np.arange(na + nb) % 4, _table(4, ka + kb, 15)
    runs = []
    for kw in ({}, {"devices": [0, 0, 0]}):
        m = _model(name, 6, first_chain_id=3, **kw)
        m.init_bisbm()
        m.set_fields(cls, field)
        bad = field.copy()
        bad[3, ka + kb - 1] = INF
        msg = _refused(lambda: m.set_fields(cls, bad), B.BISBM_ERR_INVALID_ARG)
        assert "field[3][%d]" % (ka + kb - 1) in msg and "bisbm_constraints_set" in msg, msg
        got = m.fields()  # (the refused set left the fields in place, on every entry: the calls below agree)
        assert (got[0] == cls).all() and got[1].tobytes() == field.tobytes()
        runs.append(_calls(m))
        m.close()
    _same_calls(*runs)


@pytest.mark.parametrize("how", ["clear_fields", "zero_table"])
def test_cleared_fields_leave_the_handle_of_one_that_never_had_any(how):
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, chains = na + nb, 4
    cls, field = np.arange(n) % 4, _table(4, ka + kb, 16)
    first = 4  # (a multiple of the ladder's length below)
    a = _model(name, chains, first_chain_id=first)
    a.shuffle_bisbm()
    a.set_fields(cls, field)
    a.run_sweeps(1)
    cum = a.get_entropy().copy()
    if how == "clear_fields":
        a.clear_fields()
    else:
        zero = np.zeros((2, ka + kb))
        zero[1, 0] = -0.0
        a.set_fields(cls % 2, zero)
    assert a.fields() == (None, None) and (a.field_energy() == 0.0).all()
    assert (_bits(a.get_entropy()) == _bits(cum)).all()  # (setting or clearing does not touch the sum)
    b = _model(name, chains, first_chain_id=first)
    b.shuffle_bisbm()   # (the shuffle epoch of a)
    b.run_sweeps(1)     # (... and its sweep counter)
    for c in range(chains):
        b.set_memberships(a.get_memberships(c), chain=c)
    b.init_bisbm()
    cum_a, cum_b = a.get_entropy(), b.get_entropy()

    def step(m, base):
        out = []
        m.run_sweeps(2)
        out.append(m.last_counts()[0].copy())
        steps = m.last_pass_steps()
        out.append(m.heatbath_sweeps(1, 1.0))
        out.append(m.reshuffle(2, 1, 1.0))
        rec = [{k: (_bits(v).tolist() if isinstance(v, float) else v) for k, v in x.items()} for x in m.reshuffle_last()]
        m.set_tempering([1.0, 1.4])
        m.tempering_rounds(2, mh=1, heatbath=1, reshuffles=1, scans=1)
        out.append(m.tempering_state()[0].copy())
        m.set_tempering(None)
        sums = m.get_entropy() - base  # (before the resampling: a copied slot carries its parent's sum, and the bases differ)
        out.append(m.population_resample(1.0, 1.01)[0])
        return out, rec, [_state(m, c) for c in range(chains)], sums, steps
    ra, rb = step(a, cum_a), step(b, cum_b)
    assert ra[4] == rb[4] and ra[4] > 1  # (the production kernel runs again: more than one step per pass)
    for x, y in zip(ra[0], rb[0]):
        assert (np.asarray(x) == np.asarray(y)).all()
    assert ra[1] == rb[1]
    assert all(_same_state(x, y) for x, y in zip(ra[2], rb[2]))
    # (the sums advance by the same dS values from different bases -- a's holds the dE of its fielded sweep -- so the differences
    # agree to the rounding of the sums, not bit for bit)
    assert (np.abs(ra[3] - rb[3]) <= 1e-9 * np.abs(a.entropy())).all()
    a.close()
    b.close()


def test_refusals_and_the_round_trip():
    name = "tiny"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, K = na + nb, ka + kb
    cls, field = np.arange(n) % 3, _table(3, K, 17)
    m = _model(name, 2, first_chain_id=FIRST_ID)
    m.init_bisbm()
    k = B.C.c_uint32(99)
    assert B.lib().bisbm_fields_get(m._h, B.C.byref(k), None, None) == B.BISBM_OK and k.value == 0
    assert m.fields() == (None, None)
    m.set_fields(cls, field)
    got = m.fields()
    assert got[0].dtype == np.uint8 and (got[0] == cls).all() and got[1].dtype == np.float64 and got[1].tobytes() == field.tobytes()
    assert B.lib().bisbm_fields_get(m._h, B.C.byref(k), None, None) == B.BISBM_OK and k.value == 3
    assert B.lib().bisbm_fields_get(m._h, None, None, None) == B.BISBM_OK
    for value, word in ((float("nan"), "NaN"), (INF, "+inf"), (-INF, "-inf")):
        bad = field.copy()
        bad[2, 1] = value
        msg = _refused(lambda: m.set_fields(cls, bad), B.BISBM_ERR_INVALID_ARG)
        assert "field[2][1]" in msg and word in msg and ("bisbm_constraints_set" in msg) == (value == INF), msg
    assert "class" in _refused(lambda: B.BlockModel._check(m, B.lib().bisbm_fields_set(
        m._h, 2, B._p(np.full(n, 2, dtype=np.uint8), B._u8p), B._p(np.ones(2 * K), B._f64p))), B.BISBM_ERR_INVALID_ARG)
    assert "256" in _refused(lambda: B.BlockModel._check(m, B.lib().bisbm_fields_set(
        m._h, 257, B._p(np.zeros(n, dtype=np.uint8), B._u8p), B._p(np.ones(257 * K), B._f64p))), B.BISBM_ERR_INVALID_ARG)
    for bad_call in (lambda: m.set_fields(cls[:-1], field), lambda: m.set_fields(cls, field[:, :-1]), lambda: m.set_fields(cls + 40, field),
                     lambda: m.set_fields(cls.astype(np.float64), field)):
        with pytest.raises(ValueError):
            bad_call()
    got = m.fields()
    assert (got[0] == cls).all() and got[1].tobytes() == field.tobytes()
    # merges
    state = [_state(m, c) for c in range(2)]
    assert "bisbm_fields_set(h, 0, NULL, NULL)" in _refused(lambda: m.agg_merge(1, 0), B.BISBM_ERR_STATE)
    assert "bisbm_fields_set(h, 0, NULL, NULL)" in _refused(lambda: m.agg_merge(1), B.BISBM_ERR_STATE)
    assert all(_same_state(_state(m, c), state[c]) for c in range(2)) and m.ka_kb(0) == (ka, kb)
    # entropy() stays the description length; set_memberships stays
    plain = _model(name, 2, first_chain_id=FIRST_ID)
    plain.init_bisbm()
    assert (_bits(m.entropy()) == _bits(plain.entropy())).all()
    plain.close()
    m.set_memberships(m.get_memberships(1), chain=0)
    m.init_bisbm()
    m.clear_fields()
    m.agg_merge(1, 0)  # (allowed again)
    assert m.ka_kb(0) == (ka - 1, kb)
    m.close()
    compat = _model(name, 2, rng="mt19937-compat")
    compat.init_bisbm()
    assert "MT19937" in _refused(lambda: compat.set_fields(cls, field), B.BISBM_ERR_UNSUPPORTED)
    assert compat.fields() == (None, None)
    compat.close()
    wide = _model("wide_labels", 2)
    wide.init_bisbm()
    (_, _), wna, wnb, wka, wkb, _ = _case("wide_labels")
    assert "byte labels" in _refused(lambda: wide.set_fields(np.zeros(wna + wnb, dtype=np.uint8), np.ones((1, wka + wkb))), B.BISBM_ERR_UNSUPPORTED)
    wide.close()
    from test_gpu_pair_scores import _merge_until_mixed, _mixed_shapes_model
    g, deg, gna, gnb = _mixed_shapes_model()
    _merge_until_mixed(g)
    assert len({g.ka_kb(c) for c in range(g.n_chains)}) > 1
    assert "block counts" in _refused(lambda: g.set_fields(np.zeros(g.n, dtype=np.uint8), np.ones((1, g.K))), B.BISBM_ERR_STATE)
    g.close()


def test_the_command_line_pulls_hinted_nodes_towards_their_hints(tmp_path):
    rowptr, col, na, nb = O.load_graph("n_1000")
    n = na + nb
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    planted = O.contiguous_labels(na, nb, 4, 6).astype(np.int64)
    listed = np.arange(7, n, 20)
    nxt = lambda b: np.where(b < 4, (b + 1) % 4, 4 + (b - 4 + 1) % 6)
    # a membership file that is deliberately NOT the planted partition at the listed nodes: they sit one block further, and
    # the field gives that block a weight that no likelihood of one node outweighs
    hint = {int(v): int(nxt(planted[v])) for v in listed}
    labels = planted.copy()
    labels[listed] = nxt(planted[listed])
    mb, fl = tmp_path / "labels.txt", tmp_path / "fields.txt"
    mb.write_text("".join("%d\n" % x for x in labels))
    fl.write_text("".join("%d %d:1e300\n" % (v, hint[v]) for v in reversed(sorted(hint))))
    base = [cli, "-e", el, "-y", str(na), str(nb), "-z", "4", "6", "--membership_path", str(mb), "-d", "5", "--rng", "philox", "--chains", "4",
            "-b", str(3 * n), "-t", str(4 * n), "-f", str(2 * n), "--marginalize"]
    r = subprocess.run(base + ["--fields", str(fl)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "fields: %d of %d nodes listed, 11 class(es)" % (len(listed), n) in r.stderr, r.stderr
    out = np.array(r.stdout.split(), dtype=np.int64)
    assert len(out) == n and all(out[v] == hint[int(v)] for v in listed)
    free = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert free.returncode == 0, free.stderr
    free_out = np.array(free.stdout.split(), dtype=np.int64)
    assert any(free_out[v] != hint[int(v)] for v in listed)  # (without the field they go back to the planted block)
    fl.write_text("3 0:2\n1000 4:2\n")
    bad = subprocess.run(base + ["--fields", str(fl)], capture_output=True, text=True, timeout=600)
    assert bad.returncode == 1 and "'1000'" in bad.stderr and bad.stdout == ""
    fl.write_text("3 0:2\n")
    compat = subprocess.run(base[:base.index("--rng")] + base[base.index("--rng") + 2:] + ["--fields", str(fl)], capture_output=True, text=True, timeout=600)
    assert compat.returncode == 1 and "--rng philox" in compat.stderr


def test_marginalize_sets_the_fields_before_the_burn_in():
    rowptr, col, na, nb = O.load_graph("n_1000")
    n, chains = na + nb, 8
    planted = O.contiguous_labels(na, nb, 4, 6).astype(np.int64)
    hinted = np.arange(0, n, 20)
    nxt = lambda b: np.where(b < 4, (b + 1) % 4, 4 + (b - 4 + 1) % 6)
    cls, field = B.fields_from_weights(n, 10, {int(v): {int(nxt(planted[v])): 1e300} for v in hinted}, na=na, ka=4)
    start = planted.copy()
    start[hinted] = nxt(planted[hinted])  # (the hinted nodes start one block further, where the field holds them)
    m = B.BlockModel(start, syn.types_vector(na, nb), 10, 4, 6, 1.0, (rowptr, col), n_chains=chains, seed=5)
    m.init_bisbm()
    labels = B.marginalize(m, 3, 2, 1)[0]
    assert (labels[hinted] != start[hinted]).any()  # (without the field they go back to the planted block)
    m.close()
    for kw in ({}, {"sampler": "heatbath"}, {"reshuffles": 1}, {"tempering": [1.0, 1.3], "rung_moves": {"mh": 1, "heatbath": 1, "reshuffles": 1}}):
        m = B.BlockModel(start, syn.types_vector(na, nb), 10, 4, 6, 1.0, (rowptr, col), n_chains=chains, seed=5)
        m.init_bisbm()
        labels, counts = B.marginalize(m, 3, 2, 1, fields=(cls, field), **kw)[:2]
        assert (m.fields()[0] == cls).all(), kw
        assert (labels[hinted] == start[hinted]).all(), kw
        m.close()
    m = B.BlockModel(planted, syn.types_vector(na, nb), 10, 4, 6, 1.0, (rowptr, col), n_chains=chains, seed=5)
    m.init_bisbm()
    out = B.marginalize_modes(m, 1, 2, 1, threshold=0.5, fields=(cls, field))
    assert m.fields()[1].tobytes() == field.tobytes() and out["labels"].shape[1] == n
    m.close()


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "noisy_labels.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hints as weights" in r.stdout and "hints clamped" in r.stdout and "wrongly hinted nodes" in r.stdout, r.stdout
