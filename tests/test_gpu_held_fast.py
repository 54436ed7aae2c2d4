"""GPU tests of held Metropolis-Hastings sweeps on the production kernel.

A handle with clamped nodes and / or block constraints runs its MH sweeps on the held instances of the production kernel: the
feeder wave hands every step an allowed word (csrc/bisbm_held_word.hpp) and the stepping wave bars the targets it does not hold,
one or two steps per pass.  The chain is the chain the generic kernel runs for the same clamp and constraints -- the tie of either
kernel to the oracle is tests/test_gpu_held_oracle.py (tests/test_gpu_clamp.py and tests/test_gpu_constraints.py, which force no
kernel, check the prefix property on the device); here the two kernels are tied to each other under every switch.  Every
comparison: handle A with nothing forced, handle B under BISBM_FORCE_GENERIC=1, three chains with first chain id 5, the same
start, hold and calls; per chain the labels, m, m_r, n_r, eta and both columns of last_counts() are equal integer for integer, the
running sum of accepted dS (BISBM_KEEP_SUM=1) agrees as tests/test_gpu_parity.py asks of the production kernel (1e-9 of the sum
plus 1e-12 of the description length), and A reports two steps per pass where B reports one."""
import importlib
import os

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_heatbath import _case, _model

B = importlib.import_module("bipartitesbm-mcmc_amd")

pytestmark = pytest.mark.gpu

SEED = 21
FIRST_ID = 5
CHAINS = 3
BIG = 1 << 60
ENV = ("BISBM_FORCE_GENERIC", "BISBM_HELD_FAST", "BISBM_SINGLE_STEPS", "BISBM_PREDICT_SKEW", "BISBM_LAUNCH_STEPS", "BISBM_ETA_WINDOW",
       "BISBM_FIXED_ROLES", "BISBM_PASS_DEPTH", "BISBM_T_TABLE_CAP", "BISBM_ONE_STAGE")


@pytest.fixture(autouse=True)
def _clean_environment(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BISBM_KEEP_SUM", "1")


def _visit(gid, sweep, na, nb):
    L = O.lib()
    return [int(L.orc_philox_visit(SEED, gid, sweep, na, nb, i)) for i in range(na + nb)]


def _snap(m, extra=None):
    acc, sw = m.last_counts()
    return dict(state=[(m.get_memberships(c), m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c)) for c in range(m.n_chains)],
                acc=acc.copy(), sweeps=sw.copy(), cum=m.get_entropy().copy(), S=m.entropy().copy(), steps=m.last_pass_steps(), extra=extra)


def _assert_same(a, b, what):
    for c, (x, y) in enumerate(zip(a["state"], b["state"])):
        for part, u, v in zip(("labels", "m", "m_r", "n_r", "eta"), x, y):
            assert (u == v).all(), (what, c, part, np.flatnonzero(np.asarray(u != v).ravel())[:8])
    assert (a["acc"] == b["acc"]).all() and (a["sweeps"] == b["sweeps"]).all(), (what, a["acc"], b["acc"], a["sweeps"], b["sweeps"])
    for c in range(len(a["cum"])):  # (sum_dS_close of tests/test_gpu_parity.py, with B in the place of the oracle)
        assert abs(a["cum"][c] - b["cum"][c]) <= 1e-9 * abs(b["cum"][c]) + 1e-12 * abs(b["S"][c]), (what, c, a["cum"][c], b["cum"][c])
    if a["extra"] is not None:
        assert (np.asarray(a["extra"]) == np.asarray(b["extra"])).all(), (what, a["extra"], b["extra"])


def _half_lists(name, seed):
    """Every node but a tenth of each type (unlisted: class 0, which allows all) gets one of up to 40 random halves of its type's
    blocks; three more nodes of each type get a single block.  On k64_eta_in_hbm (50 + 64 blocks) ten type-b nodes get the class
    that allows exactly block 63 of type b beside one other block -- bit 63 of the allowed word.  Tried over seeds until the
    round-robin start leaves no block empty.  Returns (class_of_node, allowed, start labels)."""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    for attempt in range(50):
        rng = np.random.default_rng(1000 * seed + attempt)
        lists = {}
        for lo, cnt, b0, k in ((0, na, 0, ka), (na, nb, ka, kb)):
            pool = [sorted(b0 + rng.choice(k, size=max(1, k // 2), replace=False)) for _ in range(40)]
            listed = rng.random(cnt) >= 0.1
            for v in np.flatnonzero(listed):
                lists[lo + int(v)] = pool[int(rng.integers(len(pool)))]
            for v in rng.choice(cnt, size=min(3, cnt), replace=False):
                lists[lo + int(v)] = [b0 + int(rng.integers(k))]
        if name == "k64_eta_in_hbm":
            for v in rng.choice(nb, size=10, replace=False):
                lists[na + int(v)] = [ka + 17, ka + 63]
        cls, allowed = B.constraints_from_lists(n, ka + kb, lists, na=na, ka=ka)
        try:
            start = B.admissible_start(na, nb, ka, kb, cls, allowed)
        except ValueError:
            continue
        own = allowed[:, :ka].sum(axis=1), allowed[:, ka:].sum(axis=1)
        assert allowed[0].all() and ((own[0] == 1) | (own[1] == 1)).any()
        if name == "k64_eta_in_hbm":
            row = np.ones(ka + kb, dtype=bool)
            row[ka:] = False
            row[[ka + 17, ka + 63]] = True
            assert any((r == row).all() for r in allowed) and (start == ka + 63).any()
        return cls, allowed, start
    raise AssertionError("no admissible start for %s" % name)


def _handle(name, hold, mask=None, warm=0, seed=SEED, fields=None, lists=None):
    """hold: "clamp" -- shuffle_bisbm (and `warm` unheld sweeps), then a random 30 % clamp (or `mask`); "constraints" -- the
    round-robin start of _half_lists under its table; "both" -- that start and table, and the clamp on top; "none" -- the start of
    "clamp" without the clamp.  seed: the handle's Philox seed.  fields: (class_of_node, field), set after everything else
    (tests/test_gpu_held_oracle.py).  lists: (class_of_node, allowed, start) in the place of _half_lists(name, 3)
    (tests/test_gpu_held_wide.py, whose shapes have their own recipe)"""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    if mask is None:
        mask = np.random.default_rng(77).random(n) < 0.3
    if hold in ("clamp", "none"):
        m = _model(name, CHAINS, seed=seed, first_chain_id=FIRST_ID)
        m.shuffle_bisbm()
        if warm:
            m.run_sweeps(warm)
    else:
        cls, allowed, start = _half_lists(name, 3) if lists is None else lists
        m = _model(name, CHAINS, seed=seed, first_chain_id=FIRST_ID, labels=start)
        m.init_bisbm()
        m.constrain(cls, allowed)
    if hold in ("clamp", "both"):
        m.clamp(mask)
        assert int(m.clamped().sum()) == int(mask.sum())
    if fields is not None:
        m.set_fields(*fields)
    return m


def _calls(m, n):
    """three sweeps at T = 1, one at T = 0.5, and an exponential anneal from 1.5 that is below T = 0.3 after two of its four sweeps,
    with the early stop armed (steps_await = n / 2: the bookkeeping runs through barred steps, and the schedule instance)"""
    mh = B.MetropolisHasting()
    out = []
    m.run_sweeps(3)
    out.append(_snap(m))
    m.run_sweeps(1, 0.5)
    out.append(_snap(m))
    rate = float((0.3 / 1.5) ** (1.0 / (2 * n)))
    r = np.atleast_1d(mh.anneal(m, "exponential", [1.5, rate], 4 * n, max(1, n // 2))).copy()
    out.append(_snap(m, extra=r))
    return out


def _run_pair(monkeypatch, make, calls, env=None, env_a=None, steps_a=2, steps_b=1):
    env = env or {}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for k, v in (env_a or {}).items():
        monkeypatch.setenv(k, v)
    a = make()
    snaps_a = calls(a)
    for k in (env_a or {}):
        monkeypatch.delenv(k)
    monkeypatch.setenv("BISBM_FORCE_GENERIC", "1")
    b = make()
    snaps_b = calls(b)
    monkeypatch.delenv("BISBM_FORCE_GENERIC")
    for k in env:
        monkeypatch.delenv(k)
    assert len(snaps_a) == len(snaps_b)
    for i, (x, y) in enumerate(zip(snaps_a, snaps_b)):
        _assert_same(x, y, i)
        assert x["steps"] == steps_a and y["steps"] == steps_b, (i, x["steps"], y["steps"])
    moved = sum(int(s["acc"].sum()) for s in snaps_a)
    a.close()
    b.close()
    return snaps_a, moved


# ------------------------------------------------------------------------------------------------------------- 1. cases
NAMES = ["tiny", "ka1", "hubs_isolated", "huge_hub", "eps0", "edgeless", "k32_eta_in_hbm", "k64_eta_in_hbm"]


@pytest.mark.parametrize("hold", ["clamp", "constraints", "both"])
@pytest.mark.parametrize("name", NAMES)
def test_a_held_sweep_on_the_production_kernel_is_the_generic_kernels(monkeypatch, name, hold):
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    snaps, accepted = _run_pair(monkeypatch, lambda: _handle(name, hold), lambda m: _calls(m, na + nb))
    assert accepted > 0  # (steps were accepted: the chains went somewhere)
    if hold != "constraints":  # the clamped labels are where they were
        mask = np.random.default_rng(77).random(na + nb) < 0.3
        m0 = _handle(name, hold)
        for c in range(CHAINS):
            assert (snaps[-1]["state"][c][0][mask] == m0.get_memberships(c)[mask]).all()
        m0.close()


# ------------------------------------------------------------------------------------- 2. masks built from the visit order
WARM = 3  # (as tests/test_gpu_clamp.py builds its masks: on the order of the sweep behind a shuffle and three sweeps)


def _order_mask(kind, order, n):
    mask = np.zeros(n, dtype=bool)
    if kind == "even":      # the first step of every pass that starts at an even position is barred
        mask[order[0::2]] = True
    elif kind == "odd":
        mask[order[1::2]] = True
    elif kind == "chunks":  # a whole chunk of 64 clamped, then a chunk with one open node
        mask[order[64:192]] = True
        mask[order[150]] = False
    else:                   # the first and the last position of the sweep
        mask[[order[0], order[n - 1]]] = True
    return mask


@pytest.mark.parametrize("kind", ["even", "odd", "chunks", "ends"])
def test_masks_built_from_the_visit_order(monkeypatch, kind):
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    order = _visit(FIRST_ID + CHAINS - 1, WARM, na, nb)  # chain 2's sweep after the shuffle and WARM unheld sweeps
    assert sorted(order) == list(range(n)) and all(v < na for v in order[:na])
    mask = _order_mask(kind, order, n)
    assert int(mask.sum()) == {"even": n // 2, "odd": n // 2, "chunks": 127, "ends": 2}[kind]

    def calls(m):
        out = []
        for _ in range(3):  # (sweep by sweep: the first one is the sweep the mask was built on)
            m.run_sweeps(1)
            out.append(_snap(m))
        return out
    _run_pair(monkeypatch, lambda: _handle(name, "clamp", mask, warm=WARM), calls)


# ------------------------------------------------------------------------------------------------ 3. the kernel's switches
@pytest.mark.parametrize("env", [{"BISBM_SINGLE_STEPS": "1"}, {"BISBM_PREDICT_SKEW": "3"}, {"BISBM_LAUNCH_STEPS": "1"}, {"BISBM_ETA_WINDOW": "1"},
                                 {"BISBM_FIXED_ROLES": "1"}, {"BISBM_FIXED_ROLES": "2"}], ids=lambda e: "%s=%s" % next(iter(e.items())))
@pytest.mark.parametrize("name", ["hubs_isolated", "k32_eta_in_hbm"])
def test_the_same_chain_under_every_switch_of_the_production_kernel(monkeypatch, name, env):
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    for hold in ("clamp", "constraints", "both"):
        _run_pair(monkeypatch, lambda: _handle(name, hold), lambda m: _calls(m, na + nb), env=env,
                  steps_a=1 if "BISBM_SINGLE_STEPS" in env else 2)


def test_a_call_cut_into_launches_of_one_sweep_resumes_through_barred_steps(monkeypatch):
    """a temperature table of one step: the production kernel runs the cooling call as one launch per sweep, and the early-stop
    bookkeeping travels in the chain's scalars (the generic kernel, which evaluates its schedule itself, runs it in one)"""
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    _run_pair(monkeypatch, lambda: _handle(name, "both"), lambda m: _calls(m, na + nb), env_a={"BISBM_T_TABLE_CAP": "1"})


# --------------------------------------------------------------------------------------------------------------- 4. depth
def test_a_held_launch_caps_the_depth_and_a_cleared_clamp_gives_it_back(monkeypatch):
    name = "k8_eta_in_hbm"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    monkeypatch.setenv("BISBM_PASS_DEPTH", "8")
    mask = np.random.default_rng(77).random(n) < 0.3

    def calls(m):
        m.run_sweeps(2)
        return [_snap(m)]
    a = _handle(name, "clamp", mask)
    held_a = calls(a)
    monkeypatch.setenv("BISBM_FORCE_GENERIC", "1")
    b = _handle(name, "clamp", mask)
    held_b = calls(b)
    monkeypatch.delenv("BISBM_FORCE_GENERIC")
    _assert_same(held_a[0], held_b[0], "held")
    assert held_a[0]["steps"] == 2 and held_b[0]["steps"] == 1
    a.unclamp()
    never = _model(name, CHAINS, first_chain_id=FIRST_ID)
    never.shuffle_bisbm()  # (the shuffle epoch of a)
    never.run_sweeps(2)    # (... and its sweep counter)
    for c in range(CHAINS):
        never.set_memberships(a.get_memberships(c), chain=c)
    never.init_bisbm()
    base_a, base_n = a.get_entropy().copy(), never.get_entropy().copy()
    a.run_sweeps(2)
    never.run_sweeps(2)
    sa, sn = _snap(a), _snap(never)
    assert sa["steps"] == 8 and sn["steps"] == 8
    sa["cum"], sn["cum"] = sa["cum"] - base_a, sn["cum"] - base_n
    _assert_same(sa, sn, "cleared")  # (the sums started from different values: their advances agree to the tolerance, not bit for bit)
    for m in (a, b, never):
        m.close()


# ---------------------------------------------------------------------------------------------------------- 5. the share rule
def _all_but_ten(order, n):
    """every node held except ten open ones, picked by their positions in chain 2's sweep order"""
    open_nodes = [order[i] for i in (0, 1, 63, 64, 150, 299, 300, 301, 400, 499)]
    mask = np.ones(n, dtype=bool)
    mask[open_nodes] = False
    return mask


def _three_sweeps(m):
    m.run_sweeps(3)
    return [_snap(m)]


def test_the_share_of_clamped_nodes_routes_the_launch(monkeypatch):
    """490 of 500 nodes clamped is past kHeldFastMaxClampShare: nothing pinned, the generic kernel runs; BISBM_HELD_FAST=1 pins the
    production kernel; BISBM_HELD_FAST=0 sends a 5 % clamped handle to the generic kernel.  All of them the same chains.  (On the bench
    graph the production kernel still wins at 98 % clamped, DESIGN.md section 29: the default is the route such a handle had before.)"""
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    mask = _all_but_ten(_visit(FIRST_ID + CHAINS - 1, WARM, na, nb), n)
    assert n == 500 and int(mask.sum()) == 490
    make = lambda: _handle(name, "clamp", mask, warm=WARM)
    free = make()
    snap_free = _three_sweeps(free)[0]
    assert snap_free["steps"] == 1
    monkeypatch.setenv("BISBM_HELD_FAST", "1")
    pinned = make()
    snap_pinned = _three_sweeps(pinned)[0]
    assert snap_pinned["steps"] == 2
    _assert_same(snap_pinned, snap_free, "98 % clamped")
    # a 5 % clamp takes the production kernel, and BISBM_HELD_FAST=0 sends it back
    light = np.random.default_rng(5).random(n) < 0.05
    monkeypatch.setenv("BISBM_HELD_FAST", "0")
    off = _handle(name, "clamp", light)
    snap_off = _three_sweeps(off)[0]
    assert snap_off["steps"] == 1
    monkeypatch.delenv("BISBM_HELD_FAST")
    on = _handle(name, "clamp", light)
    snap_on = _three_sweeps(on)[0]
    assert snap_on["steps"] == 2
    _assert_same(snap_on, snap_off, "5 % clamped")
    # BISBM_HELD_FAST=0 is for held handles only
    monkeypatch.setenv("BISBM_HELD_FAST", "0")
    plain = _model(name, CHAINS, first_chain_id=FIRST_ID)
    plain.shuffle_bisbm()
    plain.run_sweeps(1)
    assert plain.last_pass_steps() > 1
    for m in (free, pinned, off, on, plain):
        m.close()


# --------------------------------------------------------------------------------------------------------------- 6. fields
def test_fields_beside_a_clamp_stay_on_the_generic_kernel():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    m = _handle(name, "clamp")
    field = np.zeros((2, ka + kb))
    field[1, :ka], field[1, ka:] = 0.75, -1.25
    field[1, 0] = 2.0
    m.set_fields(np.arange(n) % 2, field)
    m.run_sweeps(1)
    assert m.last_pass_steps() == 1
    m.clear_fields()
    m.run_sweeps(1)
    assert m.last_pass_steps() == 2
    m.close()
