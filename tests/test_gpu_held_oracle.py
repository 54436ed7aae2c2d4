"""GPU tests of held Metropolis-Hastings sweeps against the held oracle.

The oracle's Philox-mode step knows the clamp, the block constraints and the block fields (oracle/bisbm_oracle.c, pinned on the CPU by
tests/test_oracle_holds.py), so orc_anneal is a full-length reference for a held call: every schedule, the early stop through barred
steps, T = 0, the return value.  Every comparison here: three chains with first chain id 5, one oracle model per chain, the same
start, hold and calls; after EVERY call and per chain the labels, m, m_r, n_r, eta, both columns of last_counts() and the anneal's
return value are the oracle's, integer for integer and float for float, the running sum (BISBM_KEEP_SUM=1) agrees as
tests/test_gpu_parity.py asks (1e-9 of the sum plus 1e-12 of the description length), under fields its advance is that of S + Phi,
the clamped labels are where they were and every label is inside its list.  Each route -- nothing forced, and
BISBM_FORCE_GENERIC=1 -- is compared with the oracle, not with the other route (tests/test_gpu_held_fast.py does that).

Two conditions on the inputs, checked on the oracle's side before the device is looked at: no accept test of a call lies within a
relative 1e-9 of its threshold (orc_last_margin: the last bits of the device's exp cannot decide a case; SEEDS below holds the seed
of every case, found on the host, where the oracle alone runs), and no case is vacuous: the oracle saw barred steps, accepted moves,
proposals of a barred target where a table is set, decisions the field turned where a field is set (pytest -s prints the counts)."""
import importlib
import math

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_heatbath import _case
from test_gpu_held_fast import CHAINS, ENV, FIRST_ID, WARM, _all_but_ten, _half_lists, _handle, _order_mask
from test_gpu_parity import sum_dS_close
from test_oracle_holds import random_field

B = importlib.import_module("bipartitesbm-mcmc_amd")

pytestmark = pytest.mark.gpu

BIG = 1 << 60
SEED = 21
# (name, hold) -> the Philox seed of the case where SEED leaves an accept test within 1e-9 of its threshold (none does so far)
SEEDS = {}
# edgeless under all three holds has one node that is neither clamped nor confined to one block, node 4: with the field classes v mod 4
# it has the zero row and the field turns no decision; (v + 1) mod 4 gives it a row
FIELD_SHIFT = {("edgeless", "all"): 1}
NAMES = ["tiny", "ka1", "hubs_isolated", "huge_hub", "eps0", "edgeless", "k32_eta_in_hbm", "k64_eta_in_hbm", "k8_eta_in_hbm"]
HOLDS = ["clamp", "constraints", "both", "fields", "all"]


@pytest.fixture(autouse=True)
def _clean_environment(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BISBM_KEEP_SUM", "1")


def _visit(seed, gid, sweep, na, nb):
    L = O.lib()
    return [int(L.orc_philox_visit(seed, gid, sweep, na, nb, i)) for i in range(na + nb)]


# ------------------------------------------------------------------------------------------------------- holds and starts
_LISTS = {}


def _tables(name, hold, mask=None):
    """The hold of a case: mask (30 % of the nodes unless given), (class_of_node, allowed) and the start of _half_lists(name, 3),
    (class_of_node, field) of four classes with entries of about 1.5 nats.  None where the hold has no such part.  (A module whose
    shapes need lists of another recipe puts them into _LISTS first: tests/test_gpu_held_wide.py.)"""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    t = dict(mask=None, cn=None, start=None, fl=None)
    if hold in ("clamp", "both", "all"):
        t["mask"] = np.random.default_rng(77).random(n) < 0.3 if mask is None else mask
    if hold in ("constraints", "both", "all"):
        if name not in _LISTS:
            _LISTS[name] = _half_lists(name, 3)
        cls, allowed, start = _LISTS[name]
        t["cn"], t["start"] = (cls, allowed), start
    if hold in ("fields", "all"):
        t["fl"] = random_field(np.random.default_rng(79), n, ka + kb, shift=FIELD_SHIFT.get((name, hold), 0))
    return t


def _oracles(name, t, seed, warm=0):
    """one oracle per chain at the device's start -- shuffle_bisbm (and `warm` unheld sweeps, which move the sweep counter) from the
    contiguous labels, or the constraints' round-robin start -- then handed the hold"""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    out = []
    for c in range(CHAINS):
        lab = O.contiguous_labels(na, nb, ka, kb) if t["start"] is None else t["start"]
        o = O.OracleModel(rowptr, col, na, nb, ka, kb, eps, lab)
        o.seed_philox(seed, FIRST_ID + c)
        if t["start"] is None:
            o.shuffle_bisbm()
            if warm:
                o.anneal("constant", [1.0], warm * (na + nb), BIG)
        else:
            o.init_bisbm()
        if t["mask"] is not None:
            o.clamp(t["mask"])
        if t["cn"] is not None:
            o.constrain(*t["cn"])
        if t["fl"] is not None:
            o.set_fields(*t["fl"])
        out.append(o)
    return out


def _device(name, t, seed, warm=0):
    """tests/test_gpu_held_fast.py's _handle for the hold of the case, with the seed of the case and the field on top"""
    hold = {(False, False): "none", (True, False): "clamp", (False, True): "constraints", (True, True): "both"}[(t["mask"] is not None, t["cn"] is not None)]
    lists = None if t["cn"] is None else t["cn"] + (t["start"],)  # (the table and the start the oracles were given)
    return _handle(name, hold, mask=t["mask"], warm=warm, seed=seed, fields=t["fl"], lists=lists)


# ------------------------------------------------------------------------------------------------------------- the calls
def _call_list(n):
    """1. three sweeps at T = 1; 2. one at T = 0.5; 3. an exponential anneal from 1.5 that is below 0.3 halfway, the early stop armed;
    4. a linear call (1.2 down to 0.4) and a logarithmic call of two sweeps; 5. abrupt_cool with its switch inside the second of
    three sweeps: held T = 0 steps; 6. constant calls at T = 0.5 with steps_await = 0 and with steps_await = n - 1 (below one sweep, and reached after the first sweep
    only if the barred steps since the last minimum count); 7. one sweep of the
    constant T = 0 route"""
    rate = float((0.3 / 1.5) ** (1.0 / (2 * n)))
    return [("constant", [1.0], 3 * n, BIG), ("constant", [0.5], n, BIG), ("exponential", [1.5, rate], 4 * n, max(1, n // 2)),
            ("linear", [1.2, 0.8 / (2 * n)], 2 * n, BIG), ("logarithmic", [1.0, 2.0], 2 * n, BIG), ("abrupt_cool", [1.5 * n], 3 * n, BIG),
            ("constant", [0.5], 2 * n, 0), ("constant", [0.5], 3 * n, n - 1), ("constant", [0.0], n, BIG)]


def _sweeps(k):
    return lambda n: [("constant", [1.0], n, BIG)] * k


def _reference(name, t, seed, calls, warm=0):
    """the oracles' side of a case: per call and chain the state, the return value, the counts, the running sum and S; per call the
    smallest margin and the hold counters summed over the chains"""
    os_ = _oracles(name, t, seed, warm)
    start = [o.memberships() for o in os_]
    out = []
    for sched, kw, dur, wait in calls:
        chains, margin, seen = [], math.inf, dict(clamped=0, barred=0, fielded=0, turned=0, accepted=0)
        for o in os_:
            ret = o.anneal(sched, kw, dur, wait)
            chains.append(dict(state=(o.memberships(), o.m(), o.m_r(), o.n_r(), o.eta()), ret=ret, acc=o.last_accepted, sweeps=o.last_sweeps,
                               cum=o.get_entropy(), S=o.entropy()))
            margin = min(margin, o.last_margin)
            for k, v in o.hold_counts().items():
                seen[k] += v
            seen["accepted"] += o.last_accepted
        out.append(dict(chains=chains, margin=margin, seen=seen))
    return start, out


class _Sum:  # (what sum_dS_close reads of an oracle model)
    def __init__(self, cum, S):
        self.cum, self.S = cum, S

    def get_entropy(self):
        return self.cum

    def entropy(self):
        return self.S


def _assert_inputs(what, t, ref):
    """the margin condition, call by call, and the vacuity guards over the calls of the case"""
    total = dict(clamped=0, barred=0, fielded=0, turned=0, accepted=0)
    for i, r in enumerate(ref):
        assert r["margin"] > 1e-9, (what, i, r["margin"], "an accept test too close to its threshold: another seed")
        for k, v in r["seen"].items():
            total[k] += v
    print("%s: smallest margin %.3g; steps of clamped nodes %d, barred targets %d, accepted %d, fielded steps %d of which the field turned %d"
          % (what, min(r["margin"] for r in ref), total["clamped"], total["barred"], total["accepted"], total["fielded"], total["turned"]))
    assert total["accepted"] >= 1 and total["clamped"] + total["barred"] + total["fielded"] >= 1, (what, total)
    if t["mask"] is not None:
        assert total["clamped"] >= 1, (what, total)
    if t["cn"] is not None:
        assert total["barred"] >= 1, (what, total)
    if t["fl"] is not None:
        assert total["fielded"] >= 1 and total["turned"] >= 1, (what, total)


def _assert_call(what, m, t, start, r, rates, before, na, ka, steps):
    acc, sw = m.last_counts()
    cum, S, phi = m.get_entropy(), m.entropy(), m.field_energy()
    for c, want in enumerate(r["chains"]):
        got = (m.get_memberships(c), m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c))
        for part, x, y in zip(("labels", "m", "m_r", "n_r", "eta"), got, want["state"]):
            assert (x == y).all(), (what, c, part, np.flatnonzero(np.asarray(x != y).ravel())[:8])
        assert int(acc[c]) == want["acc"] and int(sw[c]) == want["sweeps"], (what, c, int(acc[c]), want["acc"], int(sw[c]), want["sweeps"])
        assert rates[c] == want["ret"], (what, c, rates[c], want["ret"])
        assert sum_dS_close(cum[c], _Sum(want["cum"], want["S"])), (what, c, cum[c], want["cum"])
        if t["fl"] is not None:  # delta cum = delta S + delta Phi ("Block fields" 4.), as tests/test_gpu_fields.py asserts it
            cum0, S0, phi0 = before
            assert abs((cum[c] - cum0[c]) - ((S[c] - S0[c]) + (phi[c] - phi0[c]))) <= 1e-9 * abs(S0[c]), (what, c)
        if t["mask"] is not None:
            assert (got[0][t["mask"]] == start[c][t["mask"]]).all(), (what, c)
        if t["cn"] is not None:
            cls, allowed = t["cn"]
            assert allowed[cls, got[0]].all(), (what, c)
    assert m.last_pass_steps() == steps, (what, m.last_pass_steps(), steps)


def _held_steps(t, sched, kw, forced=False, fast=True):
    """steps per pass of a held launch as bisbm_anneal.hip routes it: the generic kernel under fields and under the force, the
    production kernel's general step alone in a constant T = 0 call, else its two-steps pass"""
    if forced or not fast or t["fl"] is not None or (sched == "constant" and kw[0] == 0.0):
        return 1
    return 2


def _run(m, t, start, ref, calls, what, na, ka, forced=False, fast=True):
    mh = B.MetropolisHasting()
    for i, ((sched, kw, dur, wait), r) in enumerate(zip(calls, ref)):
        before = (m.get_entropy().copy(), m.entropy().copy(), m.field_energy().copy())
        rates = np.atleast_1d(mh.anneal(m, sched, kw, dur, wait)).copy()
        _assert_call((what, i, sched), m, t, start, r, rates, before, na, ka, _held_steps(t, sched, kw, forced, fast))


# ------------------------------------------------------------------------------------------------------------- 1. cases
_REF = {}  # (one entry: the two routes of a case follow each other and share the oracles' run)


def _case_reference(name, hold):
    key = (name, hold)
    if key not in _REF:
        (rowptr, col), na, nb, ka, kb, eps = _case(name)
        _REF.clear()
        t = _tables(name, hold)
        calls = _call_list(na + nb)
        _REF[key] = (t, calls) + _reference(name, t, SEEDS.get(key, SEED), calls)
    return _REF[key]


@pytest.mark.parametrize("route", ["production", "generic"])
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_every_held_call_is_the_held_oracles(monkeypatch, name, hold, route):
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    t, calls, start, ref = _case_reference(name, hold)
    _assert_inputs((name, hold), t, ref)
    if route == "generic":
        monkeypatch.setenv("BISBM_FORCE_GENERIC", "1")
    m = _device(name, t, SEEDS.get((name, hold), SEED))
    _run(m, t, start, ref, calls, (name, hold, route), na, ka, forced=route == "generic")
    m.close()


# ------------------------------------------------------------------------------------- 2. masks built from the visit order
@pytest.mark.parametrize("kind", ["even", "odd", "chunks", "ends"])
def test_masks_built_from_the_visit_order_against_the_oracle(kind):
    """tests/test_gpu_held_fast.py's masks on the order of chain 2's sweep behind a shuffle and WARM sweeps: the first or the second
    step of every pass barred, a whole chunk of 64 clamped and one with a single open node, the two ends of the sweep -- sweep by sweep"""
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    mask = _order_mask(kind, _visit(SEED, FIRST_ID + CHAINS - 1, WARM, na, nb), n)
    t = _tables(name, "clamp", mask)
    calls = _sweeps(3)(n)
    start, ref = _reference(name, t, SEED, calls, warm=WARM)
    _assert_inputs((name, kind), t, ref)
    m = _device(name, t, SEED, warm=WARM)
    _run(m, t, start, ref, calls, (name, kind), na, ka)
    m.close()


# ------------------------------------------------------------------------------------------------------------ 3. cut calls
def test_a_cooling_call_cut_into_launches_of_one_sweep_is_the_oracles_single_loop(monkeypatch):
    """a temperature table of one step: the production kernel runs the exponential call as one launch per sweep, and entropy_min, the
    count of T < 1 steps and "this chain has returned" travel through barred steps in the chain's scalars"""
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    t = _tables(name, "both")
    calls = _call_list(n)[:3]
    calls[2] = calls[2][:3] + (n // 8,)  # (steps_await = n / 2 is not reached in the call's four sweeps)
    start, ref = _reference(name, t, SEED, calls)
    _assert_inputs((name, "table cap"), t, ref)
    assert [c["sweeps"] for c in ref[2]["chains"]] == [1, 4, 4]  # (the early stop of the cooling call is reached in one chain)
    monkeypatch.setenv("BISBM_T_TABLE_CAP", "1")
    m = _device(name, t, SEED)
    _run(m, t, start, ref, calls, (name, "table cap"), na, ka)
    m.close()


def test_long_constant_calls_under_every_kind_of_steps_await_are_the_oracles_single_loop():
    """tiny under a clamp and constraints: constant calls at T = 0.5 longer than ceil(100000 / n) sweeps, the length at which an unheld
    handle's call is cut into launches, with steps_await 0, below one sweep, inside the call and out of reach"""
    name = "tiny"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    t = _tables(name, "both")
    seg = (100000 + n - 1) // n
    dur = (seg + 3) * n + 5
    calls = [("constant", [0.5], dur, wait) for wait in (0, n // 2, 40 * n, BIG)]
    start, ref = _reference(name, t, SEED, calls)
    _assert_inputs((name, "long calls"), t, ref)
    stops = [[c["sweeps"] for c in r["chains"]] for r in ref]
    assert stops[0] == [1] * CHAINS and stops[1] == [1] * CHAINS and stops[3] == [seg + 3] * CHAINS
    assert all(1 < s < seg + 3 for s in stops[2]), stops[2]  # (inside the call)
    m = _device(name, t, SEED)
    _run(m, t, start, ref, calls, (name, "long calls"), na, ka)
    m.close()


# ---------------------------------------------------------------------------------------------------------- 4. the share rule
@pytest.mark.parametrize("pin", [None, "1", "0"])
@pytest.mark.parametrize("share", ["490 of 500", "5 %"])
def test_both_sides_of_the_share_rule_are_the_oracles_chain(monkeypatch, share, pin):
    """490 of 500 nodes clamped is past kHeldFastMaxClampShare and runs the generic kernel, a 5 % clamp the production kernel;
    BISBM_HELD_FAST=1 / =0 pins either: six launches, each the oracle's chain"""
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    if share == "5 %":
        mask, warm = np.random.default_rng(5).random(n) < 0.05, 0
    else:
        mask, warm = _all_but_ten(_visit(SEED, FIRST_ID + CHAINS - 1, WARM, na, nb), n), WARM
        assert n == 500 and int(mask.sum()) == 490
    t = _tables(name, "clamp", mask)
    calls = _sweeps(3)(n)
    start, ref = _reference(name, t, SEED, calls, warm=warm)
    _assert_inputs((name, share, pin), t, ref)
    if pin is not None:
        monkeypatch.setenv("BISBM_HELD_FAST", pin)
    fast = pin == "1" or (pin is None and share == "5 %")
    m = _device(name, t, SEED, warm=warm)
    _run(m, t, start, ref, calls, (name, share, pin), na, ka, fast=fast)
    m.close()
