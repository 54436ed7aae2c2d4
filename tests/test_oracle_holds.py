"""CPU tests of the oracle's held Metropolis-Hastings step (oracle/bisbm_oracle.c: orc_set_clamp, orc_set_constraints,
orc_set_fields; include/bisbm.h "Clamped nodes" 1., "Block constraints" 1., "Block fields" 1. and 4.).  The GPU tests of held sweeps
(tests/test_gpu_held_oracle.py, tests/test_gpu_fuzz_holds.py) rest on this extension, so it is pinned four ways here: with nothing
held it is the oracle it was, bit for bit; a second, literal implementation in Python agrees with it; it has the prefix property
the header states; and its chains sample the restricted / tilted target over an enumerable state space."""
import numpy as np
import pytest

import cases
import oracle_lib as O
from mh_replay import mh_replay_sweep, visit

BIG = 1 << 60
SEED = 21
GID = 7
LOW_T = 0.3  # (the low temperature of tests/test_gpu_clamp.py and tests/test_gpu_constraints.py)
_GRAPHS = {}


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _case(name):
    if name not in _GRAPHS:
        _, na, nb, ne, ka, kb, eps, hubs, iso = cases.HELD_WIDE_CASES[name] if name in cases.HELD_WIDE_CASES else cases.CASE[name]
        _GRAPHS[name] = (cases.random_graph(11, na, nb, ne, ka, kb, hubs, iso), na, nb, ka, kb, eps)
    return _GRAPHS[name]


def _oracle(name, gid=GID, seed=SEED, shuffle=True):
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    o = O.OracleModel(rowptr, col, na, nb, ka, kb, eps, O.contiguous_labels(na, nb, ka, kb))
    o.seed_philox(seed, gid)
    if shuffle:
        o.shuffle_bisbm()
    else:
        o.init_bisbm()
    return o


def _state(o):
    return o.memberships(), o.m(), o.m_r(), o.n_r(), o.eta()


def half_table(rng, labels, na, ka, kb, pools=12, unlisted=0.1):
    """Class 0 allows everything; classes 1 .. pools allow a random half of the type-a blocks, the next `pools` a random half of the
    type-b blocks (the other type's columns are set: the header ignores them).  Every node but about a tenth gets a class of its
    type; the current label of every node, in every label vector of `labels` (rows), is then added to its class's row, so the
    table is admissible for all of them.  Returns (class_of_node, allowed)."""
    labels = np.atleast_2d(labels)
    n, K = labels.shape[1], ka + kb
    allowed = np.ones((1 + 2 * pools, K), dtype=np.uint8)
    for i in range(pools):
        allowed[1 + i, :ka] = 0
        allowed[1 + i, rng.choice(ka, size=max(1, ka // 2), replace=False)] = 1
        allowed[1 + pools + i, ka:] = 0
        allowed[1 + pools + i, ka + rng.choice(kb, size=max(1, kb // 2), replace=False)] = 1
    cls = np.where(np.arange(n) < na, 1 + rng.integers(pools, size=n), 1 + pools + rng.integers(pools, size=n))
    cls[rng.random(n) < unlisted] = 0
    cls = cls.astype(np.uint8)
    for lab in labels:
        allowed[cls, lab] = 1
    return cls, allowed


def random_field(rng, n, K, n_classes=4, scale=1.5, shift=0):
    """a table of entries of about `scale` nats, row 0 the zero row, and a class per node: (v + shift) mod n_classes"""
    field = rng.normal(scale=scale, size=(n_classes, K))
    field[0] = 0.0
    return ((np.arange(n) + shift) % n_classes).astype(np.uint8), field


# ------------------------------------------------------------------------------- 1. nothing held is the oracle it was
def _three_calls(o, n):
    """three sweeps at T = 1, an exponential anneal with the early stop in reach, abrupt_cool to T = 0"""
    out = []
    for sched, kw, dur, wait in (("constant", [1.0], 3 * n, BIG),
                                 ("exponential", [1.5, float((0.3 / 1.5) ** (1.0 / (2 * n)))], 4 * n, max(1, n // 2)),
                                 ("abrupt_cool", [1.5 * n], 3 * n, BIG)):
        r = o.anneal(sched, kw, dur, wait)
        out.append((_state(o), r, o.last_accepted, o.last_sweeps, _bits(o.get_entropy())))
    return out


def _trivial_holds(name):
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, K = na + nb, ka + kb
    rng = np.random.default_rng(3)
    cls3 = (np.arange(n) % 3).astype(np.uint8)
    per_type = np.zeros((3, K))
    for k, (a, b) in enumerate(((0.75, -1.25), (2.5, 0.125), (-3.0, 1e-3))):
        per_type[k, :ka], per_type[k, ka:] = a, b
    mask = rng.random(n) < 0.3

    def real_holds_then_clear(o):
        lab = o.memberships()
        o.clamp(mask)
        o.constrain(*half_table(np.random.default_rng(4), lab, na, ka, kb))
        o.set_fields(*random_field(np.random.default_rng(5), n, K))
        o.anneal("constant", [1.0], 0, BIG)  # (a call of no sweep: the holds were set and are cleared before any step)
        o.clamp(None)
        o.constrain(None, None)
        o.set_fields(None, None)

    def zeroes_then_clear(o):
        o.clamp(np.zeros(n))
        o.constrain(cls3, np.ones((3, K)))
        o.set_fields(cls3, np.zeros((3, K)))
        o.clamp(None)
        o.constrain(cls3, None)
        o.set_fields(None, None)
    return {"a NULL clamp": lambda o: o.clamp(None),
            "an all-zero mask": lambda o: o.clamp(np.zeros(n)),
            "an all-allowing table": lambda o: o.constrain(cls3, np.ones((3, K))),
            "a zero field": lambda o: o.set_fields(cls3, np.zeros((3, K))),
            "a field constant over each type": lambda o: o.set_fields(cls3, per_type),
            "holds set and cleared": real_holds_then_clear,
            "trivial holds set and cleared": zeroes_then_clear}


@pytest.mark.parametrize("name", ["tiny", "hubs_isolated", "k64_eta_in_hbm", "mid_tier_low"])
def test_nothing_held_is_the_oracle_it_was(name):
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    want = _three_calls(_oracle(name), n)
    assert sum(w[2] for w in want) > 0
    for what, hold in _trivial_holds(name).items():
        o = _oracle(name)
        hold(o)
        got = _three_calls(o, n)
        for i, (g, w) in enumerate(zip(got, want)):
            for part, x, y in zip(("labels", "m", "m_r", "n_r", "eta"), g[0], w[0]):
                assert (x == y).all(), (what, i, part)
            assert g[1] == w[1] and g[2] == w[2] and g[3] == w[3], (what, i, g[1:4], w[1:4])
            assert g[4] == w[4], (what, i, "the running sum differs in its bits")
        assert o.hold_counts()["clamped"] == 0 and o.hold_counts()["barred"] == 0 and o.hold_counts()["turned"] == 0


# ------------------------------------------------------------------------- 2. a second, literal implementation agrees
REPLAY_BASE = 3


def _replay_holds(hold, n, na, ka, kb, lab):
    mask = np.random.default_rng(77).random(n) < 0.3
    cn = half_table(np.random.default_rng(78), lab, na, ka, kb)
    fl = random_field(np.random.default_rng(79), n, ka + kb)
    return dict(clamp=mask if hold in ("clamp", "all") else None, constraints=cn if hold in ("constraints", "all") else None,
                fields=fl if hold in ("fields", "all") else None)


@pytest.mark.parametrize("hold", ["clamp", "constraints", "fields", "all"])
@pytest.mark.parametrize("name", ["hubs_isolated"] + list(cases.HELD_WIDE_CASES))
def test_orc_anneal_under_holds_is_the_python_replay(name, hold):
    """hubs_isolated and the shapes above 64 blocks of a type, where the oracle is the one reference of the device's held sweeps
    (tests/test_gpu_held_wide.py): three unheld sweeps from the contiguous labels, then 10 sweeps at T = 1 and 10 at the low T under
    the hold, sweep by sweep: labels and accepted count of orc_anneal equal those of tests/mh_replay.py.  The replay tests
    u < (accu1 / accu0) e where the oracle tests u accu0 < accu1 e: the margin condition (no test within a relative 1e-9, by both
    counts) is what makes the two the same decision, and it is a condition on the seed."""
    import math
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    o = _oracle(name, shuffle=False)
    o.anneal("constant", [1.0], REPLAY_BASE * n, BIG)
    lab = o.memberships().astype(np.int64)
    h = _replay_holds(hold, n, na, ka, kb, lab)
    if h["clamp"] is not None:
        o.clamp(h["clamp"])
    if h["constraints"] is not None:
        o.constrain(*h["constraints"])
    if h["fields"] is not None:
        o.set_fields(*h["fields"])
    probe = _oracle(name, shuffle=False)
    cls, field = h["fields"] if h["fields"] is not None else (None, None)
    seen = dict(clamped=0, barred=0, fielded=0, turned=0, accepted=0)
    margin = float("inf")
    for k in range(20):
        T = 1.0 if k < 10 else LOW_T
        lab, accepted, mg, _ = mh_replay_sweep(probe, lab, cls, field, GID, REPLAY_BASE + k, T, na, nb, ka, SEED, math.exp,
                                               clamp=h["clamp"], constraints=h["constraints"])
        o.anneal("constant", [T], n, BIG)
        assert (o.memberships() == lab).all(), (hold, k)
        assert o.last_accepted == accepted, (hold, k, o.last_accepted, accepted)
        margin = min(margin, mg, o.last_margin)
        for key, v in o.hold_counts().items():
            seen[key] += v
        seen["accepted"] += accepted
    print("replay of %s under %s: 20 sweeps equal; margin %.3g; %s" % (name, hold, margin, seen))
    assert margin > 1e-9, margin
    assert seen["accepted"] > 0
    assert (seen["clamped"] > 0) == (h["clamp"] is not None) and (seen["barred"] > 0) == (h["constraints"] is not None)
    assert (seen["turned"] > 0) == (h["fields"] is not None)
    if h["clamp"] is not None:
        assert seen["clamped"] == 20 * int(h["clamp"].sum())


# ----------------------------------------------------------------------------------------- 3. the header's prefix property
PREFIX_WARM = 8  # unheld sweeps at the low T before the holds are set: the chain has settled, so whole sweeps pass before p*


def _settled(name):
    o = _oracle(name)
    o.anneal("constant", [LOW_T], PREFIX_WARM * (o.na + o.nb), BIG)
    return o


def _first_sweep_with_a_forbidden_move(name, forbidden, sweeps=12):
    """the unheld chain sweep by sweep, at the low T: (sweep index, p*, visit order) of the first sweep in which a step made a move
    `forbidden(v, s)` names; p* is the position of the first such step (a node is visited once per sweep)"""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    free = _settled(name)
    for k in range(sweeps):
        before = free.memberships()
        free.anneal("constant", [LOW_T], n, BIG)
        after = free.memberships()
        order = visit(SEED, GID, PREFIX_WARM + k, na, nb)
        hits = [p for p, v in enumerate(order) if after[v] != before[v] and forbidden(v, int(after[v]))]
        if hits:
            return k, hits[0], order
    raise AssertionError("the unheld chain made no forbidden move")


def _assert_prefix(name, held, k_star, p_star, order):
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    free = _settled(name)
    for k in range(k_star):  # whole sweeps before the one with p*: the same chain
        free.anneal("constant", [LOW_T], n, BIG)
        held.anneal("constant", [LOW_T], n, BIG)
        assert (free.memberships() == held.memberships()).all(), k
        assert _bits(free.get_entropy()) == _bits(held.get_entropy())
    free.anneal("constant", [LOW_T], n, BIG)
    held.anneal("constant", [LOW_T], n, BIG)
    head = order[:p_star]  # (each visited once: its label after the sweep is its label after its step)
    assert (free.memberships()[head] == held.memberships()[head]).all()
    assert free.memberships()[order[p_star]] != held.memberships()[order[p_star]]


def test_a_clamped_chain_is_the_unclamped_one_up_to_its_first_move_of_a_clamped_node():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    mask = np.zeros(n, dtype=bool)
    mask[np.random.default_rng(9).choice(n, size=3, replace=False)] = True  # (few: so that whole sweeps pass before p*)
    k_star, p_star, order = _first_sweep_with_a_forbidden_move(name, lambda v, s: mask[v])
    assert k_star >= 1 and p_star >= 1, (k_star, p_star)
    held = _settled(name)
    held.clamp(mask)
    _assert_prefix(name, held, k_star, p_star, order)


def test_a_constrained_chain_is_the_unconstrained_one_up_to_its_first_accepted_target_outside_a_list():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    start = _settled(name).memberships()
    # three nodes get the class that allows their own block alone; every other node is free
    allowed = np.ones((1 + ka + kb, ka + kb), dtype=np.uint8)
    for b in range(ka + kb):
        lo, hi = (0, ka) if b < ka else (ka, ka + kb)
        allowed[1 + b, lo:hi] = 0
        allowed[1 + b, b] = 1
    cls = np.zeros(n, dtype=np.uint8)
    for v in np.random.default_rng(9).choice(n, size=3, replace=False):
        cls[v] = 1 + start[v]
    k_star, p_star, order = _first_sweep_with_a_forbidden_move(name, lambda v, s: not allowed[cls[v], s])
    assert k_star >= 1 and p_star >= 1, (k_star, p_star)
    held = _settled(name)
    held.constrain(cls, allowed)
    _assert_prefix(name, held, k_star, p_star, order)


# ------------------------------------------------------------------------------------------------ 4. the restricted target
ENUM_HELD = {0: 0, 3: 1, 6: 2, 9: 3}  # (the clamp of tests/test_gpu_clamp.py)
ENUM_START = np.array([0, 0, 1, 1, 1, 0, 2, 2, 3, 3, 3, 2], dtype=np.uint32)  # (its start: it agrees with the clamp)
ENUM_CHAINS, ENUM_SWEEPS = 6000, 60
_ENUM = {}


def _enum():
    if not _ENUM:
        _ENUM["states"], _, _ENUM["S"] = cases.enumerable_states()
    return _ENUM["states"], _ENUM["S"]


def _enum_codes(beta, hold):
    """ENUM_CHAINS oracle chains (chain ids 0 ..) from ENUM_START, ENUM_SWEEPS sweeps at T = 1 / beta under hold(o)"""
    rowptr, col = cases.enumerable_graph()
    na, nb = cases.ENUM_NA, cases.ENUM_NB
    codes = []
    for c in range(ENUM_CHAINS):
        o = O.OracleModel(rowptr, col, na, nb, 2, 2, cases.ENUM_EPS, ENUM_START)
        o.seed_philox(4242, c)
        o.init_bisbm()
        hold(o)
        o.anneal("constant", [1.0 / beta], ENUM_SWEEPS * (na + nb), BIG)
        codes.append(cases.state_code(o.memberships()))
    return np.array(codes)


def _bit(states, v):
    return (states >> v) & 1


def _chi(codes, states, S, beta, what):
    """p against exp(-beta S) over `states` above 1e-3 (a KeyError: a chain left the restricted set); the flattened target
    exp(-beta S / 1.25) is the negative control"""
    target = np.exp(-beta * (S - S.min()))
    stat, dof, p = cases.chi_square(codes, states, target / target.sum())
    flat = np.exp(-beta * (S - S.min()) / 1.25)
    p_flat = cases.chi_square(codes, states, flat / flat.sum())[2]
    print("oracle chains %s, beta = %g: chi2 = %.1f on %d dof, p = %.3g; flattened target p = %.3g" % (what, beta, stat, dof, p, p_flat))
    assert p > 1e-3, (stat, dof, p)
    return p_flat


@pytest.mark.parametrize("beta", [1.0, 5.0 / 3.0])
def test_clamped_oracle_chains_sample_the_target_restricted_to_the_clamp(beta):
    states, S = _enum()
    keep = np.ones(len(states), dtype=bool)
    for v, b in ENUM_HELD.items():
        keep &= _bit(states, v) == (b & 1)
    assert keep.sum() == 256
    mask = np.zeros(12, dtype=bool)
    mask[sorted(ENUM_HELD)] = True
    codes = _enum_codes(beta, lambda o: o.clamp(mask))
    assert _chi(codes, states[keep], S[keep], beta, "under a clamp") < 1e-6


def test_constrained_oracle_chains_sample_the_target_restricted_to_the_table():
    """two classes: class 0 allows everything, class 1 the first block of each type; nodes 0, 1 and 6 are of class 1"""
    states, S = _enum()
    keep = (_bit(states, 0) == 0) & (_bit(states, 1) == 0) & (_bit(states, 6) == 0)
    allowed = np.array([[1, 1, 1, 1], [1, 0, 1, 0]], dtype=np.uint8)
    cls = np.zeros(12, dtype=np.uint8)
    cls[[0, 1, 6]] = 1
    codes = _enum_codes(1.0, lambda o: o.constrain(cls, allowed))
    assert _chi(codes, states[keep], S[keep], 1.0, "under a two-class table") < 1e-6


def test_fielded_oracle_chains_sample_exp_minus_beta_E():
    states, S = _enum()
    rng = np.random.default_rng(11)
    cls = (np.arange(12) % 3).astype(np.uint8)
    field = np.zeros((3, 4))
    field[1:] = rng.choice([-1.0, 1.0], size=(2, 4)) * rng.uniform(0.7, 1.3, size=(2, 4))
    bits = (states[:, None] >> np.arange(12)) & 1
    labels = np.concatenate([bits[:, :6], bits[:, 6:] + 2], axis=1)
    Phi = field[cls[None, :], labels].sum(axis=1)
    beta = 1.0
    codes = _enum_codes(beta, lambda o: o.set_fields(cls, field))
    E = S + Phi
    p_E = np.exp(-beta * (E - E.min()))
    stat, dof, p = cases.chi_square(codes, states, p_E / p_E.sum())
    p_S = np.exp(-beta * (S - S.min()))
    p_plain = cases.chi_square(codes, states, p_S / p_S.sum())[2]
    print("oracle chains under a field: chi2 = %.1f on %d dof, p = %.3g; against exp(-beta S) p = %.3g" % (stat, dof, p, p_plain))
    assert p > 1e-3, (stat, dof, p)
    assert p_plain < 1e-6  # (a step that ignored the field would sample exp(-beta S))


# ------------------------------------------------------------------------- 5. what the random sequences with holds cover
def test_the_random_sequences_with_holds_cover_what_they_are_for():
    """tests/test_gpu_fuzz_holds.py walked on the host, the oracle side alone (the ops of a sequence are drawn without a look at the
    device): over its seed list the sequences anneal under a clamp or lists and under a field, make held constant T = 0 calls and held
    calls of segmented length, clear a clamp and clear lists on the small-block seeds and anneal unheld afterwards -- the launch whose
    depth the device run asserts.  The bounds are what the scripted first calls of the sequences give alone: six small-block seeds
    (every third with a T = 0 call), eight seeds with a long call (fields in every third); a generator that stops doing any of it
    fails here, without a GPU."""
    import test_gpu_fuzz_holds as F
    seeds = F.SEEDS[:48]
    total = {}
    for seed in seeds:
        log, margin, seen, shape = F.run_sequence(seed, device=False)
        assert margin > 1e-9, (seed, margin)
        for k, v in seen.items():
            total[k] = total.get(k, 0) + v
    print(total)
    small, long_call = sum(s % 8 == 7 for s in seeds), sum(s % 6 == 2 for s in seeds)
    assert small == 6 and long_call == 8
    assert total["depth_back"] >= small and total["held_long"] >= long_call
    assert total["held_anneals"] >= small + long_call - 2 and total["fielded_anneals"] >= 2 and total["held_cold"] >= 2
    assert total["cleared_clamps"] >= 1 and total["cleared_lists"] >= 1


# ----------------------------------------------------------------- 6. what the held cases above 64 blocks of a type cover
def test_the_held_cases_above_64_blocks_cover_what_they_are_for():
    """tests/test_gpu_held_wide.py walked on the host, the oracles' side alone: every case of its matrix (four shapes, five holds)
    and its four early-stop cases meets the conditions that the device run asserts before it looks at the device -- no accept test
    within a relative 1e-9 of its threshold, steps of clamped nodes, barred targets, accepted moves and decisions the field turned
    where the hold has that part, labels up to the last block, bit 255 of the table set in one class and clear in another, a block
    barred in every word of a row, and a cooling call that one chain leaves early and another runs to its end -- so a case that
    drifts fails here, without a GPU."""
    import test_gpu_held_wide as W
    assert W.NAMES == list(cases.HELD_WIDE_CASES) and len(W.NAMES) == 4 and len(W.HOLDS) == 5
    for name in W.NAMES:
        for hold in W.HOLDS:
            W.matrix_inputs(name, hold)
        W.early_stop_inputs(name)
