"""GPU tests of fielded Metropolis-Hastings sweeps on the production kernel.

A handle with block fields runs its MH sweeps on the fielded instances of the production kernel (sweep_fast_fielded_kernel): the
feeder hands every step its node's field class, the step adds f[s] - f[r] of that class's row to its finished dS, one step per pass;
a clamp and constraints beside the field come through the allowed word.  The chain is the chain the generic kernel and the held
oracle run.  After EVERY call, per chain (three chains with first chain id 5; chain 0 of two on the row-shape graphs), against the
held oracle: labels, m, m_r, n_r, eta, both columns of last_counts() and the return value are equal, the running sum agrees as
tests/test_gpu_held_oracle.py asks (sum_dS_close) and advances by dS + dPhi to 1e-9 |S| -- that module's comparisons and tolerances
(its _assert_call), no others.  On top, last_route() names the kernel that ran and what the launch carried, last_pass_steps() is 1
and last_eta_plan() is the plan of the route's kind.

The cases, their seeds and the conditions on them (no step decided by a hair, the field turns decisions, every row moves and stays)
are tests/test_fields_fast.py's, which checks them without a GPU."""
import importlib

import numpy as np
import pytest

import test_fields_fast as F
import test_gpu_held_oracle as H
import test_row_shapes as R
from test_gpu_parity import sum_dS_close

B = importlib.import_module("bipartitesbm-mcmc_amd")
SYN = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu

ENV = tuple(H.ENV) + ("BISBM_FIELD_FAST", "BISBM_KEEP_SUM")
PROD, HELD, FIELDS = B.ROUTE_PRODUCTION, B.ROUTE_HELD, B.ROUTE_FIELDS


@pytest.fixture(autouse=True)
def _clean_environment(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BISBM_KEEP_SUM", "1")


def _assert_plan(what, m, name, production):
    """the production kernel's plan -- all of eta in LDS, or a window of it on the _eta_in_hbm graphs --, or the generic kernel's"""
    plan = m.last_eta_plan()
    if not production:
        assert plan[1:] == (0, 0, 0), (what, plan)
    elif name.endswith("_eta_in_hbm"):
        assert plan[0] == 0 and plan[1] >= 1 and plan[2] >= 1 and plan[3] >= 1, (what, plan)
    else:
        assert plan == (1, 0, 0, 0), (what, plan)


def _run(m, name, t, start, ref, calls, what, production=True):
    """every call against the held oracle (tests/test_gpu_held_oracle.py's _assert_call, one step per pass), and the route"""
    (rowptr, col), na, nb, ka, kb, eps = H._case(name)
    want = (PROD if production else 0) | (HELD if (t["mask"] is not None or t["cn"] is not None) else 0) | FIELDS
    assert m.last_route() == 0  # (no MH launch yet)
    mh = B.MetropolisHasting()
    out = []
    for i, ((sched, kw, dur, wait), r) in enumerate(zip(calls, ref)):
        before = (m.get_entropy().copy(), m.entropy().copy(), m.field_energy().copy())
        rates = np.atleast_1d(mh.anneal(m, sched, kw, dur, wait)).copy()
        H._assert_call((what, i, sched), m, t, start, r, rates, before, na, ka, 1)
        assert m.last_route() == want, (what, i, m.last_route(), want)
        _assert_plan((what, i), m, name, production)
        out.append([(m.get_memberships(c), m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c)) for c in range(m.n_chains)])
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. route
@pytest.mark.parametrize("hold", F.ROUTE_HOLDS)
@pytest.mark.parametrize("name", F.ROUTE_GRAPHS)
def test_a_fielded_launch_takes_the_production_kernel_and_is_the_oracles_chain(monkeypatch, name, hold):
    """nothing forced: the production bit, the fielded bit, the held bit exactly where a clamp or lists are set, one step per pass,
    the production kernel's eta plan; BISBM_FIELD_FAST=0 and BISBM_FORCE_GENERIC=1 each clear the production bit and leave every
    integer what it was (each route is the oracle's chain)"""
    t, calls, start, ref = F.route_reference(name, hold)
    H._assert_inputs((name, hold), t, ref)
    seed = F.seed_of("route", name, hold)
    for env in (None, ("BISBM_FIELD_FAST", "1"), ("BISBM_FIELD_FAST", "0"), ("BISBM_FORCE_GENERIC", "1")):
        for k in ENV[:-1]:
            monkeypatch.delenv(k, raising=False)
        if env:
            monkeypatch.setenv(*env)
        m = H._device(name, t, seed)
        _run(m, name, t, start, ref, calls, (name, hold, env), production=env is None or env[1] == "1" and env[0] == "BISBM_FIELD_FAST")
        m.close()


# --------------------------------------------------------------------------------- 2. the switches of the production path
SWITCHES = [{"BISBM_PREDICT_SKEW": "3"}, {"BISBM_FIXED_ROLES": "1"}, {"BISBM_FIXED_ROLES": "2"}, {"BISBM_ETA_WINDOW": "1"},
            {"BISBM_LAUNCH_STEPS": "1"}, {"BISBM_KEEP_SUM": "0"}, {"BISBM_KEEP_SUM": "1"}, {"BISBM_T_TABLE_CAP": "1"}]


@pytest.mark.parametrize("env", SWITCHES, ids=["%s=%s" % kv for e in SWITCHES for kv in e.items()])
@pytest.mark.parametrize("name", F.SWITCH_GRAPHS)
def test_every_switch_of_the_production_path_leaves_the_oracles_chain(monkeypatch, name, env):
    """all three holds; three sweeps at T = 1, one at T = 0.5 and the cooling call with the early stop armed, whose tail is T = 0
    (under BISBM_T_TABLE_CAP=1 one launch per sweep: `resume` through fielded steps).  BISBM_ETA_WINDOW=1: a window of one degree,
    nearly every row takes the general step"""
    t, calls, start, ref = F.switch_reference(name)
    H._assert_inputs((name, "switches"), t, ref)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = H._device(name, t, F.seed_of("switch", name))
    _run(m, name, t, start, ref, calls, (name, env))
    if "BISBM_ETA_WINDOW" in env:
        assert m.last_eta_plan()[:2] == (0, 1)
    m.close()


# ------------------------------------------------------------------------------------------------------------ 3. row shapes
def _row_handle(g, seed, field, planted):
    m = B.BlockModel(g["labels"], SYN.types_vector(g["na"], g["nb"]), g["ka"] + g["kb"], g["ka"], g["kb"], 1.0, (g["rowptr"], g["col"]), n_chains=2,
                     rng="philox", seed=seed)
    if planted:
        m.init_bisbm()
    else:
        m.shuffle_bisbm()
    m.set_fields(*field)
    return m


@pytest.mark.parametrize("planted", [False, True], ids=["shuffled", "planted"])
@pytest.mark.parametrize("sid,dense", F.ROW_GRAPHS, ids=F.ROW_IDS)
def test_the_fielded_step_is_the_oracles_on_every_row_shape(sid, dense, planted):
    """the hot step and the general step both meet the add: rows of 1 .. 255 entries inside the eta window (8 + 7: all of eta in
    LDS) are hot, rows of 0, 256, 257 and 300 entries and everything outside the window take the general step.  Chain 0 against
    the fielded oracle after every constant call of tests/test_row_shapes.py, from the shuffled start and from the planted labels."""
    g = R.graph(sid, dense)
    n = g["na"] + g["nb"]
    ref = F.row_reference(sid, dense, planted=planted)[0]
    assert min(r["margin"] for r in ref) > 1e-9
    m = _row_handle(g, F.seed_of("rows", sid, dense), F.row_field(sid, dense), planted)
    for j, ((sched, kw, dur, wait), want) in enumerate(zip(F.row_calls(n), ref)):
        what = (sid, dense, planted, "call", j)
        cum0, S0, phi0 = m.get_entropy().copy(), m.entropy().copy(), m.field_energy().copy()
        rates = np.atleast_1d(B.MetropolisHasting().anneal(m, sched, kw, dur, wait)).copy()
        acc, sw = m.last_counts()
        assert m.last_route() == PROD | FIELDS and m.last_pass_steps() == 1, what
        plan = m.last_eta_plan()
        assert plan == (1, 0, 0, 0) if sid == "8+7" else (plan[0] == 0 and plan[1] >= 1), what + (plan,)
        assert rates[0] == want["rate"] and int(acc[0]) == want["acc"] and int(sw[0]) == want["sweeps"], what + (int(acc[0]), want["acc"])
        got = (m.get_memberships(0), m.get_m(0), m.get_m_r(0), m.get_n_r(0), m.get_eta_rk_(0))
        for part, a, b in zip(("labels", "m", "m_r", "n_r", "eta"), got, want["state"]):
            assert (np.asarray(a) == np.asarray(b)).all(), what + (part, np.flatnonzero(np.asarray(a != b).ravel())[:8])
        cum, S, phi = m.get_entropy(), m.entropy(), m.field_energy()
        assert sum_dS_close(cum[0], H._Sum(want["cum"], want["entropy"])), what + (cum[0], want["cum"])
        assert abs((cum[0] - cum0[0]) - ((S[0] - S0[0]) + (phi[0] - phi0[0]))) <= 1e-9 * abs(S0[0]), what
    m.close()


# ------------------------------------------------------------------------------------------------------------ 4. magnitudes
def test_entries_of_every_magnitude_are_added_as_the_oracle_adds_them():
    """+-40, 1e-300, -0.0 and 1e-3 in one table, at T = 0.3, T = 30 and in a constant T = 0 call (tests/test_fields_fast.py: there the
    field turns greedy steps both ways)"""
    t, calls, start, ref = F.magnitude_reference()
    H._assert_inputs((F.MAGNITUDE_GRAPH, "magnitudes"), t, ref)
    m = H._device(F.MAGNITUDE_GRAPH, t, F.seed_of("magnitudes"))
    _run(m, F.MAGNITUDE_GRAPH, t, start, ref, calls, "magnitudes")
    m.close()


# --------------------------------------------------------------------------------------- 5. a field that changes nothing
def _snap(m):
    acc, sw = m.last_counts()
    return dict(state=[(m.get_memberships(c), m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c)) for c in range(m.n_chains)],
                acc=acc.copy(), sweeps=sw.copy(), cum=m.get_entropy().copy())


def _assert_equal_bits(a, b, what):
    for c, (x, y) in enumerate(zip(a["state"], b["state"])):
        for part, u, v in zip(("labels", "m", "m_r", "n_r", "eta"), x, y):
            assert (u == v).all(), (what, c, part)
    assert (a["acc"] == b["acc"]).all() and (a["sweeps"] == b["sweeps"]).all(), what
    assert (a["cum"].view(np.uint64) == b["cum"].view(np.uint64)).all(), (what, a["cum"], b["cum"])


def test_rows_constant_over_each_type_run_the_fielded_kernel_and_change_nothing(monkeypatch):
    """f[s] - f[r] = 0 for every move: the fielded handle (one step per pass on the fielded route) is the unfielded handle (eight
    steps per pass) on every integer and on the bits of get_entropy(); after clear_fields() it is a handle that never had a field"""
    monkeypatch.setenv("BISBM_PASS_DEPTH", "8")
    name = F.NOTHING_GRAPH
    (rowptr, col), na, nb, ka, kb, eps = H._case(name)
    n = na + nb
    none = dict(mask=None, cn=None, start=None, fl=None)
    a, b = H._device(name, dict(none, fl=F.nothing_field()), F.SEED), H._device(name, none, F.SEED)
    mh = B.MetropolisHasting()
    for i, (sched, kw, dur, wait) in enumerate(F.switch_calls(n)):
        ra, rb = np.atleast_1d(mh.anneal(a, sched, kw, dur, wait)).copy(), np.atleast_1d(mh.anneal(b, sched, kw, dur, wait)).copy()
        assert (ra == rb).all(), i
        assert a.last_route() == PROD | FIELDS and a.last_pass_steps() == 1, (i, a.last_route(), a.last_pass_steps())
        assert b.last_route() == PROD and b.last_pass_steps() == 8, (i, b.last_route(), b.last_pass_steps())
        _assert_equal_bits(_snap(a), _snap(b), ("fielded", i))
    a.clear_fields()
    for i in range(2):
        a.run_sweeps(2), b.run_sweeps(2)
        assert a.last_route() == PROD and a.last_pass_steps() > 2, (i, a.last_route(), a.last_pass_steps())
        _assert_equal_bits(_snap(a), _snap(b), ("cleared", i))
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------- 6. the share rule
@pytest.mark.parametrize("pin", [None, "1"])
def test_the_share_rule_holds_for_a_fielded_handle(monkeypatch, pin):
    """490 of 500 nodes clamped beside a field: past kHeldFastMaxClampShare, the generic route; BISBM_HELD_FAST=1 pins the production
    route: the same integers, the oracle's"""
    t, calls, start, ref = F.share_reference()
    H._assert_inputs((F.SHARE_GRAPH, "490 of 500 and a field"), t, ref)
    if pin is not None:
        monkeypatch.setenv("BISBM_HELD_FAST", pin)
    m = H._device(F.SHARE_GRAPH, t, F.seed_of("share"), warm=H.WARM)
    assert m.last_route() == PROD  # (the unheld warm-up sweeps)
    mh = B.MetropolisHasting()
    (rowptr, col), na, nb, ka, kb, eps = H._case(F.SHARE_GRAPH)
    for i, ((sched, kw, dur, wait), r) in enumerate(zip(calls, ref)):
        before = (m.get_entropy().copy(), m.entropy().copy(), m.field_energy().copy())
        rates = np.atleast_1d(mh.anneal(m, sched, kw, dur, wait)).copy()
        H._assert_call((pin, i), m, t, start, r, rates, before, na, ka, 1)
        assert m.last_route() == (PROD if pin == "1" else 0) | HELD | FIELDS, (pin, i, m.last_route())
    m.close()
