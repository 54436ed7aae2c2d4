"""Metropolis-Hastings sweeps of the production kernel on the row-shape graphs, against the oracle (-m gpu).

The graphs (tests/cases.py row_shape_graph; tests/test_row_shapes.py checks them and the conditions on the inputs without a GPU)
hold, per type, one row of every length at which the feeder's walk, the hand-over word or the byte counters change behaviour
(1 .. 5, 15 .. 17, 31 .. 33, 63 .. 65, 127 .. 129, 254 .. 257, 300), rows of 255 and 128 entries whose neighbours lie in one or
two blocks (k_v bytes of 255, 128, 128 | 127 in one counter word, and 255 from one edge), rows of no entries, a last row of
col[] of 1, 3 or 255 entries, and at 20 + 27 a band of rows of 128 .. 188 entries in one block that meet in one pass.  Built like test_gpu_deep_pass_apply.py: 4 Philox chains from shuffle_bisbm, the calls of
test_row_shapes.calls (hot calls in the middle: at T = 1 a row of 255 entries hardly ever moves), and after EVERY call, per route,
  * last_pass_steps() is the pinned one and last_eta_plan() the one of the route's kind;
  * chain 0's labels, m, m_r, n_r, eta, both columns of last_counts() and the returned rate are the oracle's, its running sum is
    within 1e-9 |sum| + 1e-12 |S| (BISBM_KEEP_SUM=0) / 1e-9 |sum| (=1) of the oracle's: tests/test_gpu_target_rescue.py's bound;
  * all chains of every production route are equal bit for bit, the kept sum included; the generic kernel's chains have the same
    integers, rates and counts (its sum is another order of additions: chain 0's is held to the oracle's bound);
  * under BISBM_KEEP_SUM=1 the shape's first route and the single steps once more from the planted labels (init_bisbm), where the
    concentrated rows meet the kernel with their extreme bytes: shuffle_bisbm spreads their neighbours over the blocks;
  * the held instances (one clamped plain node and a table that allows every block -- which the library takes for no table, so the
    hold that reaches the kernel is the clamp; BISBM_HELD_FAST=1) with two steps and with one step per pass: chain 0 against the
    oracle under the same hold, all chains against each other.

Shapes, sizes and routes (a route a shape does not have is not in its list):

    blocks   nodes        graphs         routes
    8 + 7    331 + 299    sparse         depth 8 (step_oct), 4 (step_quad), 2, single steps, generic, depth 8 skewed, held, held single
    16 + 13  601 + 549    sparse, dense  depth 4 (step_quad), 2, single steps, generic, depth 4 skewed, held, held single
    20 + 27  843 + 811    sparse, dense  depth 4 with BISBM_ONE_STAGE 1 and 0 (step_quad32), 2, single, generic, one stage skewed, held, held single
    40 + 33  1211 + 1109  sparse, dense  two steps (step_pair64), single steps, generic, two steps skewed, held, held single
    64 + 50  1223 + 1217  sparse, dense  as 40 + 33 (the last lane in use), and with BISBM_ETA_WINDOW=256: two steps, held

Where the kernel keeps a window of eta in LDS -- every shape but 8 + 7 -- a row takes the hot step only inside the window of its
type, and with a row of 300 in the graph the window lies at the low degrees; the dense graph of the shape has no row above 255 and
plain degrees that draw the window up to 255.  test_every_row_takes_the_hot_step_in_one_of_the_shapes_graphs asserts from
last_eta_plan() that every ladder degree from 1 to 255 and every concentrated row is hot in one of them (at 64 + 50, where the
window holds 50 degrees, [1, 50] and [206, 255]: in one of them or under the pinned window), and prints the same for the held
instances, whose hand-over is two words longer and whose window is narrower.  Rows of 256, 257 and 300 entries and rows of none are
never hot: the kernel routes them by bit 31 of the proposal word whatever the plan says, which the rule hot() states."""
import functools
import importlib

import numpy as np
import pytest

import cases
import oracle_lib as O
import test_row_shapes as R
from test_gpu_target_rescue import ENV

pytestmark = pytest.mark.gpu

B = importlib.import_module("bipartitesbm-mcmc_amd")
SYN = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")
CHAINS = 4
ALL_ENV = tuple(ENV) + ("BISBM_ONE_STAGE", "BISBM_PREDICT_SKEW", "BISBM_HELD_FAST", "BISBM_T_TABLE_CAP")

# route: (environment, steps per pass the launches must report, kind)
_HELD = [("held", {"BISBM_HELD_FAST": "1"}, 2, "held"), ("held single", {"BISBM_HELD_FAST": "1", "BISBM_SINGLE_STEPS": "1"}, 1, "held")]
_COMMON = [("single", {"BISBM_SINGLE_STEPS": "1"}, 1, "production"), ("generic", {"BISBM_FORCE_GENERIC": "1"}, 1, "generic")]
ROUTES = {
    "8+7": [("depth 8", {"BISBM_PASS_DEPTH": "8"}, 8, "production"), ("depth 4", {"BISBM_PASS_DEPTH": "4"}, 4, "production"),
            ("depth 2", {"BISBM_PASS_DEPTH": "2"}, 2, "production"), ("depth 8 skewed", {"BISBM_PASS_DEPTH": "8", "BISBM_PREDICT_SKEW": "3"}, 8, "production")]
    + _COMMON + _HELD,
    "16+13": [("depth 4", {"BISBM_PASS_DEPTH": "4"}, 4, "production"), ("depth 2", {"BISBM_PASS_DEPTH": "2"}, 2, "production"),
              ("depth 4 skewed", {"BISBM_PASS_DEPTH": "4", "BISBM_PREDICT_SKEW": "3"}, 4, "production")] + _COMMON + _HELD,
    "20+27": [("one stage", {"BISBM_PASS_DEPTH": "4", "BISBM_ONE_STAGE": "1"}, 4, "production"),
              ("per mover", {"BISBM_PASS_DEPTH": "4", "BISBM_ONE_STAGE": "0"}, 4, "production"), ("depth 2", {"BISBM_PASS_DEPTH": "2"}, 2, "production"),
              ("one stage skewed", {"BISBM_PASS_DEPTH": "4", "BISBM_ONE_STAGE": "1", "BISBM_PREDICT_SKEW": "3"}, 4, "production")] + _COMMON + _HELD,
    "40+33": [("two steps", {}, 2, "production"), ("two steps skewed", {"BISBM_PREDICT_SKEW": "3"}, 2, "production")] + _COMMON + _HELD,
    "64+50": [("two steps", {}, 2, "production"), ("two steps skewed", {"BISBM_PREDICT_SKEW": "3"}, 2, "production")] + _COMMON + _HELD
    + [("pinned window", {"BISBM_ETA_WINDOW": "256"}, 2, "production"), ("held pinned window", {"BISBM_HELD_FAST": "1", "BISBM_ETA_WINDOW": "256"}, 2, "held")],
}


def hot(plan, t, degree):
    """whether a row of type t takes the production kernel's hot step under a plan of last_eta_plan()"""
    in_lds, w, lo = plan[0], plan[1], plan[2 + t]
    return 1 <= degree <= 255 and (in_lds == 1 or lo <= degree < lo + w)


def _handle(g, seed, held, chains=CHAINS, planted=False):
    n = g["na"] + g["nb"]
    m = B.BlockModel(g["labels"], SYN.types_vector(g["na"], g["nb"]), g["ka"] + g["kb"], g["ka"], g["kb"], 1.0, (g["rowptr"], g["col"]), n_chains=chains,
                     rng="philox", seed=seed)
    if planted:
        m.init_bisbm()
    else:
        m.shuffle_bisbm()
    if held:
        m.clamp(np.array([R.held_node(g)]))
        m.constrain(np.zeros(n, dtype=np.uint8), np.ones((1, g["ka"] + g["kb"]), dtype=np.uint8))
        assert int(m.clamped().sum()) == 1
    return m


def _set_env(monkeypatch, env, keep):
    for k in ALL_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("BISBM_KEEP_SUM", keep)


def _run(monkeypatch, g, seed, env, keep, held, planted=False):
    _set_env(monkeypatch, env, keep)
    m = _handle(g, seed, held, planted=planted)
    snaps = []
    for sched, kw, dur, wait in R.calls(g["na"] + g["nb"]):
        rates = np.atleast_1d(B.MetropolisHasting().anneal(m, sched, kw, dur, wait)).copy()
        acc, sw = m.last_counts()
        snaps.append(dict(pass_steps=m.last_pass_steps(), plan=m.last_eta_plan(), rates=rates, acc=acc.copy(), sweeps=sw.copy(), cum=m.get_entropy().copy(),
                          state=[(m.get_memberships(c), m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c)) for c in range(CHAINS)]))
    m.close()
    for k in ALL_ENV:
        monkeypatch.delenv(k, raising=False)
    return snaps


def _assert_is_the_oracles(got, want, keep, what):
    assert got["rates"][0] == want["rate"], what
    assert got["acc"][0] == want["acc"] and got["sweeps"][0] == want["sweeps"], what + (got["acc"][0], want["acc"], got["sweeps"][0], want["sweeps"])
    for part, a, b in zip(("labels", "m", "m_r", "n_r", "eta"), got["state"][0], want["state"]):
        assert (np.asarray(a) == np.asarray(b)).all(), what + (part, np.flatnonzero(np.asarray(a != b).ravel())[:8])
    tol = 1e-9 * abs(want["cum"]) + (0. if keep == "1" else 1e-12 * abs(want["entropy"]))  # (test_gpu_target_rescue.py's bound)
    assert abs(got["cum"][0] - want["cum"]) <= tol, what + (got["cum"][0], want["cum"])


def _assert_same_chains(got, ref, bits, what):
    assert (got["rates"] == ref["rates"]).all(), what
    assert (got["acc"] == ref["acc"]).all() and (got["sweeps"] == ref["sweeps"]).all(), what
    for c in range(CHAINS):
        for part, a, b in zip(("labels", "m", "m_r", "n_r", "eta"), got["state"][c], ref["state"][c]):
            assert (np.asarray(a) == np.asarray(b)).all(), what + (c, part)
    if bits:  # the running sum kept step by step: the same additions in the same order
        assert (got["cum"].view(np.uint64) == ref["cum"].view(np.uint64)).all(), what


@pytest.mark.parametrize("sid,dense", R.GRAPHS, ids=R.GRAPH_IDS)
def test_every_route_is_the_oracles_chain_on_the_row_shapes(sid, dense, monkeypatch):
    g = R.graph(sid, dense)
    n = g["na"] + g["nb"]
    seed = R.SEEDS[(sid, dense)]
    calls = R.calls(n)
    oracle = {held: R.reference(sid, dense, held)[0] for held in (False, True)}
    for held in (False, True):
        assert min(r["margin"] for r in oracle[held]) > 1e-9  # (tests/test_row_shapes.py: the inputs decide no step by a hair)
    for keep in ("0", "1"):
        first = {}
        for name, env, steps, kind in ROUTES[sid]:
            held = kind == "held"
            got = _run(monkeypatch, g, seed, env, keep, held)
            assert [s["pass_steps"] for s in got] == [steps] * len(calls), (sid, dense, keep, name, [s["pass_steps"] for s in got])
            for j, s in enumerate(got):
                what = (sid, dense, "keep", keep, name, "call", j)
                plan = s["plan"]
                if kind == "generic":
                    assert plan[1:] == (0, 0, 0), what + (plan,)
                elif sid == "8+7":
                    assert plan == (1, 0, 0, 0), what + (plan,)
                else:
                    assert plan[0] == 0 and plan[1] >= 1 and plan[2] >= 1 and plan[3] >= 1, what + (plan,)
                    if "BISBM_ETA_WINDOW" in env:
                        assert plan[1] == 256, what + (plan,)
                _assert_is_the_oracles(s, oracle[held][j], keep, what)
                if kind in first:
                    _assert_same_chains(s, first[kind][j], keep == "1", what)
                elif kind == "generic":
                    _assert_same_chains(s, first["production"][j], False, what)
            first.setdefault(kind, got)
        if keep == "1":  # from the planted labels, where the concentrated rows have their extreme bytes: the shape's first route and single steps
            planted = R.reference(sid, dense, False, planted=True)[0]
            assert min(r["margin"] for r in planted) > 1e-9
            runs = [_run(monkeypatch, g, seed, env, keep, False, planted=True) for name, env, steps, kind in (ROUTES[sid][0], _COMMON[0])]
            for j in range(len(calls)):
                for got in runs:
                    _assert_is_the_oracles(got[j], planted[j], keep, (sid, dense, "planted start", "call", j))
                _assert_same_chains(runs[1][j], runs[0][j], True, (sid, dense, "planted start", "call", j))
        print(sid, "dense" if dense else "sparse", "keep", keep, "plans", {name: first_plan for name, first_plan in
                                                                           ((k, v[0]["plan"]) for k, v in first.items())},
              "accepted per call, chain 0:", [int(s["acc"][0]) for s in first["production"]])


@functools.lru_cache(maxsize=None)
def _plans(sid):
    """the eta plan of one sweep per graph of the shape, unheld and held, plus the shape's routes that pin the window"""
    out = []
    for dense in (d for s, d in R.GRAPHS if s == sid):
        g = R.graph(sid, dense)
        for held in (False, True):
            for env in [{}] + [e for _, e, _, kind in ROUTES[sid] if "BISBM_ETA_WINDOW" in e and (kind == "held") == held]:
                out.append((dense, held, dict(env, **({"BISBM_HELD_FAST": "1"} if held else {}))))
    return out


@pytest.mark.parametrize("sid", list(cases.ROW_SHAPES))
def test_every_row_takes_the_hot_step_in_one_of_the_shapes_graphs(sid, monkeypatch):
    """The ladder must not pass with its rows on the general path: per shape, every ladder degree from 1 to 255 and every
    concentrated row lies in the hot route -- eta in LDS, or the window of the row's type -- of one of the shape's graphs, as
    last_eta_plan() reports the launch; 256, 257 and 300 never do.  The held instances are printed, and asserted for the rows of
    254 and 255 entries: their window is narrower (at 40 + 33 it leaves 127 .. 129 outside in both graphs)."""
    seen = {False: {}, True: {}}
    for dense, held, env in _plans(sid):
        g = R.graph(sid, dense)
        _set_env(monkeypatch, env, "0")
        m = _handle(g, R.SEEDS[(sid, dense)], held, chains=1)
        m.run_sweeps(1)
        plan = m.last_eta_plan()
        m.close()
        print(sid, "dense" if dense else "sparse", "held" if held else "unheld", env, "plan", plan)
        for t, name, v, d in cases.row_shape_rows(g):
            key = (t, name)
            seen[held][key] = seen[held].get(key, False) or hot(plan, t, d)
            if d > 255:
                assert not hot(plan, t, d)
        for t in (0, 1):
            assert not hot(plan, t, 0)
    for held in (False, True):
        cold = sorted(k for k, v in seen[held].items() if not v)
        print(sid, "held" if held else "unheld", "never hot:", cold)
    # (the last rows of col[] are printed above, not asserted: the row of 2 entries before a last row of 255 lies below the dense
    # graphs' windows; it is hot at 8 + 7 and under the pinned window, and the feeder walks it on either route)
    never = {k for k, v in seen[False].items() if not v and (k[1].startswith("ladder") or k[1] in R.CONCENTRATED)}
    assert never == {(t, "ladder%d" % d) for t in (0, 1) for d in (256, 257, 300)}, sorted(never)
    for t in (0, 1):
        for name in ("ladder254", "ladder255", "one_block", "copies", "split"):
            assert seen[True][(t, name)], (sid, "held", t, name)


# ------------------------------------------------------------------------------------------ the conditionals on the same rows
@pytest.mark.parametrize("start", ["swept", "planted"])
@pytest.mark.parametrize("sid", ["8+7", "40+33"])
def test_conditionals_of_every_special_row_are_the_oracles(sid, start, record_property, monkeypatch):
    """bisbm_conditionals_accumulate, whose dS rows the heat-bath and reshuffle replays take, on every special node of the sparse
    graph: after shuffle_bisbm and 3 sweeps, and from the planted labels, where the concentrated k_v are at their extremes --
    test_gpu_conditionals.py's comparison with the oracle's transition_ratio, unchanged and with its tolerance"""
    from test_gpu_conditionals import _check_dS_against_oracle, _oracle
    for k in ALL_ENV:
        monkeypatch.delenv(k, raising=False)
    g = R.graph(sid, False)
    na, nb, ka, kb = g["na"], g["nb"], g["ka"], g["kb"]
    q = np.array(sorted(v for t in (0, 1) for v in g["special"][t].values()), dtype=np.uint32)
    m = B.BlockModel(g["labels"], SYN.types_vector(na, nb), ka + kb, ka, kb, 1.0, (g["rowptr"], g["col"]), n_chains=1, rng="philox", seed=R.SEED)
    if start == "swept":
        m.shuffle_bisbm()
        m.run_sweeps(3)
    else:
        m.init_bisbm()
        assert (m.get_memberships(0) == g["labels"]).all()
    m.conditionals_set(q, beta=1.0, keep_last=True)
    m.conditionals_accumulate()
    labels = m.get_memberships(0)
    if start == "planted":
        for t in (0, 1):
            assert cases.row_k_v(g, g["special"][t]["one_block"], labels).max() == 255 and sorted(cases.row_k_v(g, g["special"][t]["split"], labels))[-2:] == [127, 128]
    o = _oracle(g["rowptr"], g["col"], na, nb, ka, kb, labels, R.SEED)
    _check_dS_against_oracle(m, o, q, na, ka, kb, record_property)
    m.close()
