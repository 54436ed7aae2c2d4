"""GPU tests of what include/bisbm.h ("Split and merge moves") promises for the time AFTER accepted moves: the chains live in
shape groups and every sampler goes on; the numbering-free analysis calls go on and average over (Ka, Kb); results are keyed by the
global chain id and depend neither on the number of device entries nor on the grouping.

Every test starts from one recipe (_regrouped): a plain handle that has become a container on its own, with shapes above the
ones it was created with and down to one block of a type, chains copied between groups several times, some groups kept while
others were formed again, and query sets made before any of that.  References: a fresh one-chain handle at the chain's present
shape, labels, global chain id and counters (bit for bit), and the host references and tolerances of the modules that test each
analysis call on chains of one shape, unchanged (tests/test_gpu_pair_scores.py and its neighbours)."""
import importlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_coassign as CO
import test_gpu_conditionals as CD
import test_gpu_edge_probs as EP
import test_gpu_edge_queries as EQ
import test_gpu_foldin as FI
import test_gpu_pair_scores as PS
import test_gpu_partition_distances as PD
import test_gpu_query_scores as QS
from test_gpu_heatbath import _assert_state_is_a_rebuild, _bits, _case, _refused
from test_gpu_split_merge import _draw
from test_pair_scores import all_pairs
from test_partition_distances import numpy_vi, relabel, vi_tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu

BETA = 0.3  # where the replays of tests/test_gpu_split_merge.py see both kinds accepted often
ALPHA = 0.25
# chains, first global chain id, seed, k_max and rounds of the recipe: rounds and seed chosen on an MI355X (_regrouped)
VARIANTS = {"tiny": dict(chains=48, first=3, seed=5, k_max=(5, 4), rounds=4),
            "n_1000": dict(chains=32, first=7, seed=4, k_max=(9, 9), rounds=4)}


@pytest.fixture(autouse=True)
def _every_launch_keeps_its_own_sum(monkeypatch):
    """the MH sweeps of these tests keep the sum of their own dS values (tests/test_gpu_heatbath.py does the same)"""
    monkeypatch.setenv("BISBM_KEEP_SUM", "1")


def _graph(v):
    """rowptr, col, na, nb and the shape and epsilon the handle is created with"""
    if v == "tiny":
        (rowptr, col), na, nb, ka, kb, eps = _case("tiny")
        return rowptr, col, na, nb, ka, kb, eps
    rowptr, col, na, nb = O.load_graph("n_1000")  # (the graph of test_gpu_pair_scores._mixed_shapes_model, created at 6 + 6)
    return rowptr, col, na, nb, 6, 6, 1.0


def _handle(v, chains=None, labels=None, shape=None, first=None, **kw):
    rowptr, col, na, nb, ka, kb, eps = _graph(v)
    cfg = VARIANTS[v]
    ka, kb = (ka, kb) if shape is None else shape
    lab = O.contiguous_labels(na, nb, ka, kb) if labels is None else labels
    return B.BlockModel(lab, syn.types_vector(na, nb), ka + kb, ka, kb, eps, (rowptr, col), n_chains=cfg["chains"] if chains is None else chains,
                        seed=cfg["seed"], first_chain_id=cfg["first"] if first is None else first, **kw)


def _entries(m):
    """the chains of every device entry, ascending"""
    first = m.device_layout()[1] + [m.n_chains]
    return [list(range(first[k], first[k + 1])) for k in range(len(first) - 1)]


def _group_order(m, shapes):
    """per device entry its chains in the order its groups hold them: the groups by the first appearance of their shape among
    the entry's chains, each group's chains ascending (regroup, as after bisbm_agg_merge_total)"""
    out = []
    for chains in _entries(m):
        seen = [shapes[c] for c in chains]
        out.append(sorted(chains, key=lambda c: (seen.index(shapes[c]), c)))
    return out


def _last_launch(m):
    """(shapes whose group the last launch kept, shapes whose group it formed again) from the chains' last records, per device
    entry: a group stays when no chain left it or joined it; nothing is formed again after a launch without an accepted move"""
    rec = m.split_merge_last()
    out = []
    for chains in _entries(m):
        if not any(rec[c]["accepted"] for c in chains):
            out.append((sorted({rec[c]["after"] for c in chains}), []))
            continue
        kept, formed = [], []
        for s in sorted({rec[c]["after"] for c in chains}):
            same = [c for c in chains if rec[c]["before"] == s] == [c for c in chains if rec[c]["after"] == s]
            (kept if same else formed).append(s)
        out.append((kept, formed))
    return out


def _regrouped(m, v, hook=None):
    """The state every test below starts from: shuffle; `hook` (query sets made and a first sample taken on the plain handle:
    reads only); a polish that stops early, so that the chains' sweeps_total differ from then on, and one pair reshuffle (both
    counters now live in the chains' scalars, which every regrouping has to carry); then rounds of {one MH sweep,
    split_merge(2, 1, 0.3, (1, 1), k_max)}.  The conditions are asserted from the handle itself, never skipped.

    Observed on an MI355X (one device entry):
    tiny (48 chains, seed 5, 4 rounds; the polish stopped after 2 to 8 sweeps): shapes 2 + 2 (1 chain), 2 + 3 (2), 3 + 3 (6),
    3 + 4 (4), 4 + 1 (1), 4 + 2 (4), 4 + 3 (10), 4 + 4 (7), 5 + 2 (5), 5 + 3 (8); 44 chains with two or more accepted moves, at
    most 6; the last launch kept the group of 2 + 2 and formed the other nine again.
    n_1000 (32 chains, seed 4, 4 rounds; the polish stopped after 8 to 22 sweeps): shapes 5 + 7 (2), 5 + 8 (1), 6 + 6 (2),
    6 + 7 (1), 6 + 8 (3), 6 + 9 (5), 7 + 6 (2), 7 + 7 (3), 7 + 8 (2), 7 + 9 (3), 8 + 7 (3), 8 + 8 (3), 9 + 7 (2); 28 chains with
    two or more accepted moves, at most 5; the last launch kept the groups of 5 + 7, 5 + 8, 6 + 6, 7 + 6 and 9 + 7 and formed the
    other eight again."""
    cfg = VARIANTS[v]
    rowptr, col, na, nb, ka0, kb0, eps = _graph(v)
    n = m.n_chains
    m.shuffle_bisbm()
    if hook is not None:
        hook(m)
    S0, cum0 = m.entropy(), m.get_entropy()
    ran = m.polish(100)[1].astype(np.int64)
    assert (ran < 100).all() and len(set(ran.tolist())) > 1, ran  # (the chains' sweep counters now differ)
    m.reshuffle(1, 2, BETA)
    assert not m.mixed_shapes and (m.chain_groups() == 0).all()  # a plain handle still
    acc = np.zeros(n, dtype=np.uint64)
    for _ in range(cfg["rounds"]):
        m.run_sweeps(1)
        acc += m.split_merge(2, 1, BETA, (1, 1), cfg["k_max"])
    shapes = [m.ka_kb(c) for c in range(n)]
    tot = m.split_merge_total().astype(np.int64)
    assert (tot[:, 0] + tot[:, 2] == 2 * cfg["rounds"]).all() and (tot[:, 1] + tot[:, 3] == acc.astype(np.int64)).all()
    groups = m.chain_groups()
    for chains in _entries(m):  # one group per shape and entry
        by_shape = {}
        for c in chains:
            by_shape.setdefault(shapes[c], set()).add(int(groups[c]))
        assert all(len(g) == 1 for g in by_shape.values()) and len({next(iter(g)) for g in by_shape.values()}) == len(by_shape), by_shape
    order = _group_order(m, shapes)
    last = _last_launch(m)
    print("%s, %d entr%s: %d rounds, shapes %s, accepted per chain %s (splits %d of %d, merges %d of %d), last launch kept %s formed %s"
          % (v, len(order), "y" if len(order) == 1 else "ies", cfg["rounds"], sorted((s, shapes.count(s)) for s in set(shapes)), acc.tolist(),
             tot[:, 1].sum(), tot[:, 0].sum(), tot[:, 3].sum(), tot[:, 2].sum(), [x[0] for x in last], [x[1] for x in last]))
    assert m.mixed_shapes and len(set(shapes)) >= 3, set(shapes)
    assert max(a for a, _ in shapes) > ka0 and max(b for _, b in shapes) > kb0, set(shapes)  # above the shape of bisbm_create
    if v == "tiny":
        assert any(min(s) == 1 for s in shapes), set(shapes)  # one block of a type
    assert acc.max() >= 2, acc  # a chain that has been copied between groups more than once
    assert sum(order, []) != list(range(n))  # the groups hold the chains in another order than the caller
    if len(order) == 1:
        assert last[0][0] and last[0][1], last  # the last launch kept some groups and formed others again
    for c in range(n):
        _assert_state_is_a_rebuild(m, rowptr, col, c)
        lab = m.get_memberships(c)
        assert sorted(set(lab[:na].tolist())) == list(range(shapes[c][0])) and sorted(set(lab[na:].tolist())) == list(range(shapes[c][0], sum(shapes[c])))
    S1, cum1 = m.entropy(), m.get_entropy()
    assert (np.abs((S1 - S0) - (cum1 - cum0)) <= 1e-9 * np.abs(S0)).all(), ((S1 - S0) - (cum1 - cum0))
    assert (m.reshuffles_total() == 1).all()
    return dict(acc=acc, shapes=shapes, order=order, last=last, sweeps=ran + cfg["rounds"], S0=S0, cum0=cum0)


# ------------------------------------------------------------------------------------- 2. samplers on regrouped chains
def _fresh_chain(v, m, c, sweeps, reshuffles):
    """a fresh one-chain handle at chain c's present shape, labels and global chain id whose sweeps_total and reshuffles_total
    are the chain's: it runs as many sweeps and reshuffles of its own, then takes the labels"""
    lab = m.get_memberships(c)
    f = _handle(v, chains=1, labels=lab, shape=m.ka_kb(c), first=VARIANTS[v]["first"] + c)
    f.init_bisbm()
    f.run_sweeps(int(sweeps))
    if reshuffles:
        f.reshuffle(int(reshuffles), 0, 1.0)
    f.set_memberships(lab)
    f.init_bisbm()
    assert int(f.reshuffles_total()[0]) == int(reshuffles)
    return f


def _same_state(m, c, f):
    return ((m.get_memberships(c) == f.get_memberships(0)).all() and (m.get_m(c) == f.get_m(0)).all() and (m.get_m_r(c) == f.get_m_r(0)).all()
            and (m.get_n_r(c) == f.get_n_r(0)).all() and (m.get_eta_rk_(c) == f.get_eta_rk_(0)).all())


def _norm(rec):
    return {k: (_bits(x).tolist() if isinstance(x, float) else [_bits(y).tolist() if isinstance(y, float) else y for y in x] if isinstance(x, tuple) else x)
            for k, x in rec.items()}


@pytest.mark.parametrize("v", ["tiny", "n_1000"])
def test_samplers_on_regrouped_chains_are_those_of_a_fresh_one_chain_handle(v):
    """A chain moved twice, a chain of a group the last launch kept, a chain of a shape above the creation shape, and (tiny) the
    chains with one block of a type: a heat-bath sweep, a polish and two pair reshuffles (0 and 2 scans) leave labels, m, m_r,
    n_r and eta of the chain and of its fresh one-chain handle equal, integer for integer, with equal move counts, records and
    reshuffles_total.  The handle ran a polish and a reshuffle BEFORE the split and merge rounds: a counter that had stayed behind
    in a destroyed group would replay draws here.  The running sum cannot be set from outside, so the two sums start at
    different values and cannot agree on bits: their advances agree within the rounding of the adds -- one add per move, each
    within 2^-53 of a partial sum, and every partial sum is the sum the call started from plus a difference of two description
    lengths of the chain, each between 0 and the largest one seen after the shuffle: (adds + 2) 2^-52 (|start| + |start'| +
    2 max S) for the difference of the two advances -- and the description length follows the running sum within 1e-9 |S|
    over everything since the shuffle."""
    cfg = VARIANTS[v]
    rowptr, col, na, nb, ka0, kb0, eps = _graph(v)
    m = _handle(v)
    info = _regrouped(m, v)
    shapes, acc, n = info["shapes"], info["acc"], m.n_chains
    kept = info["last"][0][0]
    picks = [int(np.argmax(acc >= 2)), next(c for c in range(n) if shapes[c] in kept), next(c for c in range(n) if shapes[c][0] > ka0),
             next(c for c in range(n) if shapes[c][1] > kb0)] + [c for c in range(n) if min(shapes[c]) == 1][:3]
    picks = sorted(set(picks))
    sweeps = info["sweeps"].copy()
    fresh = {c: _fresh_chain(v, m, c, sweeps[c], 1) for c in picks}

    def level(what, moves_m=None, moves_f=None):
        for c in picks:
            assert _same_state(m, c, fresh[c]), (what, c, shapes[c])
            if moves_m is not None:
                assert int(moves_m[c]) == int(moves_f[c][0]), (what, c)

    level("start")
    cum = {c: (m.get_entropy()[c], fresh[c].get_entropy()[0]) for c in picks}
    moved = m.heatbath_sweeps(1, 1.0)
    got = {c: fresh[c].heatbath_sweeps(1, 1.0) for c in picks}
    level("heat bath", moved, got)
    total_moves = {c: int(moved[c]) for c in picks}
    assert all(moved[c] == 0 for c in range(n) if shapes[c] == (1, 1))  # one block per type: nowhere to go
    moved, ran = m.polish(7)
    got = {c: fresh[c].polish(7) for c in picks}
    level("polish", moved, {c: got[c][0] for c in picks})
    assert all(int(ran[c]) == int(got[c][1][0]) for c in picks) and all(ran[c] == 1 for c in range(n) if shapes[c] == (1, 1))
    total_moves = {c: total_moves[c] + int(moved[c]) for c in picks}
    for scans, beta in ((0, 1.0), (2, BETA)):
        accepted = m.reshuffle(1, scans, beta)
        rec = m.reshuffle_last()
        got = {c: fresh[c].reshuffle(1, scans, beta) for c in picks}
        level("reshuffle, %d scans" % scans, accepted, got)
        for c in picks:
            assert _norm(rec[c]) == _norm(fresh[c].reshuffle_last()[0]), (scans, c, rec[c])
        for c in range(n):  # one block of a type: no pair of that type; one block of each: a counted no-op
            ka, kb = shapes[c]
            if (ka, kb) == (1, 1):
                assert rec[c]["type"] == B.RESHUFFLE_NONE and not rec[c]["accepted"] and rec[c]["M"] == 0
            else:
                assert rec[c]["type"] == (0 if rec[c]["s"] < ka else 1) and rec[c]["r"] < rec[c]["s"] < ka + kb
                assert (ka > 1 or rec[c]["type"] == 1) and (kb > 1 or rec[c]["type"] == 0)
    tot = m.reshuffles_total()
    assert (tot == 3).all() and all(int(fresh[c].reshuffles_total()[0]) == 3 for c in picks)
    for c in picks:  # the advances of the two running sums
        d_m, d_f = m.get_entropy()[c] - cum[c][0], fresh[c].get_entropy()[0] - cum[c][1]
        scale = abs(cum[c][0]) + abs(cum[c][1]) + 2.0 * float(info["S0"].max())
        assert abs(d_m - d_f) <= (total_moves[c] + 4) * 2.0 ** -52 * scale, (c, d_m, d_f)
    S1, cum1 = m.entropy(), m.get_entropy()
    assert (np.abs((S1 - info["S0"]) - (cum1 - info["cum0"])) <= 1e-9 * np.abs(info["S0"])).all()
    # the next move's kind and choice are those of the chain's own count of proposals, which travelled with it
    lab = [m.get_memberships(c) for c in range(n)]
    j = m.split_merge_total().astype(np.int64)[:, [0, 2]].sum(axis=1)
    m.split_merge(1, 1, BETA, (1, 1), cfg["k_max"])
    for c, r in enumerate(m.split_merge_last()):
        x = _draw(cfg["seed"], cfg["first"] + c, int(j[c]), 0)
        want = D.numpy_split_merge_choice(x[0], x[1], *shapes[c], (1, 1), cfg["k_max"], size_of=lambda g: int((lab[c] == g).sum()))
        assert (r["kind"], r["type"], r["r"], r["s"], r["refused"]) == want, (c, r, want)
        if shapes[c] == (1, 1) and r["kind"] == B.SM_MERGE:
            assert r["refused"] == B.SM_NO_PAIR and not r["accepted"]
    for f in fresh.values():
        f.close()
    m.close()


# --------------------------------------------------------------- 3. / 4. analysis calls set before the handle was a container
def _queries(v):
    rowptr, col, na, nb, ka0, kb0, eps = _graph(v)
    deg = np.diff(rowptr.astype(np.int64))
    rs = np.random.default_rng(2)
    if v == "tiny":
        nodes = np.concatenate([np.arange(na + nb), [0]])  # every node, one of them twice
        pairs = all_pairs(na, nb)
        add = pairs
        eq = nodes
        virtual = [("a", [na, na + 3]), ("b", [0, 5, 5]), ("a", [na + nb - 1]), ("b", [na - 1])]
        cond = nodes
    else:
        nodes = np.array([3, na + 3, 499, na + 499, 250, 3])
        pairs = PS._random_pairs(na, nb, 2000)
        add = np.stack([rs.integers(0, na, 24), na + rs.integers(0, nb, 24)], axis=1)
        eq = np.array([3, na + 3])
        virtual = FI._virtual_nodes(na, nb, isolated=False)[:7]
        cond = np.array([3, na + 4, 3, na - 1, na + nb - 1, int(np.argmax(deg)), 77, na + 55])
    us = np.flatnonzero(deg[:na] > 0)[::max(1, na // 12)][:12]
    rem = np.stack([us, col[rowptr[us].astype(np.int64)]], axis=1).astype(np.int64)  # every such node's first edge
    edits, kinds = np.concatenate([add, rem]), np.array([0] * len(add) + [1] * len(rem), dtype=np.uint8)
    return dict(nodes=nodes, pairs=pairs, edits=edits, kinds=kinds, eq=eq, virtual=virtual, cond=cond.astype(np.uint32), deg=deg,
                mult=D.numpy_edge_multiplicity(rowptr, col, edits), eq_mult=D.numpy_edge_query_mult(rowptr, col, na, eq),
                qs_pairs=QS._query_pairs(nodes, na, nb))


def _set_all(m, Q):
    m.pair_scores_set(Q["pairs"])
    m.query_scores_set(Q["nodes"])
    m.coassign_set(Q["nodes"])
    m.foldin_set(Q["virtual"], ALPHA)
    m.edge_probs_set(Q["edits"], Q["kinds"], keep_last=True)
    m.edge_queries_set(Q["eq"])
    m.conditionals_set(Q["cond"], 1.0, keep_last=True)


def _accumulate_all(m):
    m.pair_scores_accumulate()
    m.query_scores_accumulate()
    m.coassign_accumulate()
    m.foldin_accumulate()
    m.edge_probs_accumulate()
    m.edge_queries_accumulate()
    m.conditionals_accumulate()


class _OneChain:
    """fresh one-chain handles, one per shape, with the KEEP_LAST query sets: the rows and terms of given labels"""

    def __init__(self, v, Q):
        self.v, self.Q, self.by_shape = v, Q, {}

    def rows(self, shape, lab):
        if shape not in self.by_shape:
            f = _handle(self.v, chains=1, labels=lab, shape=shape, first=0)
            f.conditionals_set(self.Q["cond"], 1.0, keep_last=True)
            f.edge_probs_set(self.Q["edits"], self.Q["kinds"], keep_last=True)
            f.foldin_set(self.Q["virtual"], ALPHA)
            self.by_shape[shape] = f
        f = self.by_shape[shape]
        f.set_memberships(lab)
        f.init_bisbm()
        f.conditionals_reset()
        f.conditionals_accumulate()
        f.edge_probs_accumulate()
        f.foldin_accumulate()
        cond = [f.conditionals_last(i) for i in range(len(self.Q["cond"]))]
        return dict(stats=f.conditionals_stats(), dS=[x[0][0] for x in cond], P=[x[1][0] for x in cond],
                    edge=np.array([f.edge_probs_last(i)[0] for i in range(len(self.Q["edits"]))]),
                    post=[f.foldin_posteriors(i)[0] for i in range(len(self.Q["virtual"]))])

    def close(self):
        for f in self.by_shape.values():
            f.close()


class _Reference:
    """the host references of the pooled numbers, one part per device entry (every entry keeps the sums of its own chains, and
    they are added in entry order when read), each fed one chain at a time in the order given"""

    def __init__(self, m, Q, na, entries):
        self.Q, self.na = Q, na
        z = lambda k: [np.zeros(k) for _ in range(entries)]
        self.pair = np.zeros(len(Q["pairs"]))
        self.qs, self.seen = z(len(Q["qs_pairs"][0])), []
        self.fold = [[None] * len(Q["virtual"]) for _ in range(entries)]
        self.ds, self.w = z(len(Q["edits"])), z(len(Q["edits"]))
        self.eq = [EQ.zeros_like_rows(Q["eq_mult"]) for _ in range(entries)]
        self.cond = [CD._zero(len(Q["cond"])) for _ in range(entries)]
        self.terms = 0

    def sample(self, m, orders, one):
        Q, deg = self.Q, self.Q["deg"]
        per = {c: one.rows(m.ka_kb(c), m.get_memberships(c)) for c in range(m.n_chains)}
        self.pair += PS._sample_ref(m, deg, Q["pairs"])
        self.seen += CO._labels(m, range(m.n_chains))
        post, edge = {}, {}
        for d, chains in enumerate(orders):
            QS._add_chains(self.qs[d], m, deg, Q["qs_pairs"][0], chains)
            post.update(FI._add_chains(self.fold[d], m, deg, Q["virtual"], ALPHA, chains))
            edge.update(EP.model_sample(m, self.ds[d], self.w[d], Q["edits"], Q["kinds"], Q["mult"], deg, chains))
            EQ.model_sample(m, self.eq[d], Q["eq"], Q["eq_mult"], deg, self.na, chains)
            CD._add_terms(self.cond[d], {c: per[c]["stats"] for c in chains}, chains)
        self.terms += m.n_chains
        return per, post, edge

    @staticmethod
    def _fold(parts, add=lambda x, y: x + y):
        out = parts[0]
        for p in parts[1:]:
            out = add(out, p)
        return out

    def totals(self):
        fold = self._fold
        cond = fold(self.cond, lambda x, y: {k: x[k] + y[k] for k in x})
        return dict(pair=self.pair, qs=fold(self.qs), co=D.numpy_coassign(self.seen, self.Q["nodes"], self.na),
                    fold=fold(self.fold, lambda x, y: [[a[0] + b[0], a[1] + b[1]] for a, b in zip(x, y)]),
                    ds=fold([0.0 + x for x in self.ds]), w=fold([0.0 + x for x in self.w]),
                    eq=fold(self.eq, lambda x, y: [(0.0 + a) + b for a, b in zip(x, y)]), cond=cond, terms=self.terms)


_RUNS = {}
RUNS = [("tiny", 1), ("tiny", 2), ("tiny", 3), ("n_1000", 1), ("n_1000", 3)]


def _run(v, entries):
    """One handle of `entries` device entries through: the *_set calls on the plain handle at its creation shape, one sample,
    the recipe, one more sample; with the host references of both samples.  Shared by the tests below; the handle stays open."""
    if (v, entries) in _RUNS:
        return _RUNS[(v, entries)]
    rowptr, col, na, nb, ka0, kb0, eps = _graph(v)
    Q = _queries(v)
    m = _handle(v, **({} if entries == 1 else {"devices": [0] * entries}))
    one = _OneChain(v, Q)
    ref = _Reference(m, Q, na, entries)
    r = dict(m=m, Q=Q, v=v, na=na, nb=nb, rowptr=rowptr, col=col)

    def first_sample(m):
        _set_all(m, Q)
        ref.sample(m, _entries(m), one)
        _accumulate_all(m)
        r["terms1"] = dict(pair=m.pair_scores()[1], qs=m.query_scores(0)[1], co=m.coassignment(0)[1], fold=m.foldin_scores(0, FI.REC)[1],
                           edge=m.edge_probs()["terms"], eq=m.edge_queries(0)["terms"], cond=m.conditionals_stats()["terms"])
    r["info"] = _regrouped(m, v, hook=first_sample)
    r["per"], r["post"], r["edge"] = ref.sample(m, r["info"]["order"], one)
    _accumulate_all(m)
    r["want"] = ref.totals()
    r["labels"] = [m.get_memberships(c) for c in range(m.n_chains)]
    one.close()
    _RUNS[(v, entries)] = r
    return r


@pytest.fixture(scope="module", autouse=True)
def _close_the_shared_handles():
    yield
    for r in _RUNS.values():
        r["m"].close()
    _RUNS.clear()


@pytest.fixture(params=RUNS, ids=lambda p: "%s-%d" % p)
def run(request):
    return _run(*request.param)


def test_every_pooled_call_counted_every_chain_in_both_samples(run):
    m, n = run["m"], run["m"].n_chains
    assert set(run["terms1"].values()) == {n}, run["terms1"]
    now = dict(pair=m.pair_scores()[1], qs=m.query_scores(0)[1], co=m.coassignment(0)[1], fold=m.foldin_scores(0, FI.REC)[1],
               edge=m.edge_probs()["terms"], eq=m.edge_queries(0)["terms"], cond=m.conditionals_stats()["terms"])
    assert set(now.values()) == {2 * n} and run["want"]["terms"] == 2 * n, now


def test_pair_scores_pool_over_the_shapes(run):
    s, terms = run["m"].pair_scores()
    assert PS._close(s, run["want"]["pair"], terms), (np.abs(s - run["want"]["pair"]) / np.maximum(run["want"]["pair"], 1e-300)).max() / PS.EPS
    assert s.max() > 0


def test_query_scores_pool_over_the_shapes_and_topk_ranks_the_rows(run):
    m, Q = run["m"], run["Q"]
    rows, terms = QS._rows(m, len(Q["nodes"]))
    rs = Q["qs_pairs"][1]
    assert all((rows[i] == run["want"]["qs"][rs[i]]).all() for i in range(len(rs)))
    QS._check_topk(m, run["rowptr"], run["col"], run["na"], run["nb"], Q["nodes"], rows, ks=(1, 4) if run["v"] == "tiny" else (10,))


def test_coassignment_counts_every_chain_and_topk_ranks_the_rows(run):
    m, Q = run["m"], run["Q"]
    rows, terms = CO._rows(m, len(Q["nodes"]))
    assert CO._same(rows, run["want"]["co"])
    CO._check_topk(m, run["na"], Q["nodes"], rows, ks=(1, 4) if run["v"] == "tiny" else (10,))


def test_foldin_rows_posteriors_and_topk(run):
    m, Q = run["m"], run["Q"]
    rows, terms = FI._rows(m, len(Q["virtual"]))
    FI._check_rows(rows, run["want"]["fold"])
    FI._check_posteriors(m, Q["virtual"], run["post"])  # (rows of different lengths, 0.0 past a chain's own blocks)
    FI._check_topk(m, Q["virtual"], rows, ks=(1, 4) if run["v"] == "tiny" else (10,))
    for i, (t, _) in enumerate(Q["virtual"]):  # ... and bit for bit the fresh one-chain handle's, by the caller's chain index
        got = m.foldin_posteriors(i)
        for c in range(m.n_chains):
            k_own = run["info"]["shapes"][c][1 if t == "b" else 0]
            assert FI._same(got[c, :k_own], run["per"][c]["post"][i][:k_own]) and (got[c, k_own:] == 0).all(), (i, c)


def test_edge_probabilities_each_group_with_its_own_shape_and_the_last_rows(run):
    m, Q = run["m"], run["Q"]
    r = m.edge_probs()
    assert (r["mult"] == Q["mult"]).all() and EP.same(r["dS_sum"], run["want"]["ds"]) and EP.same(r["w_sum"], run["want"]["w"])
    for i in range(len(Q["edits"])):
        got = m.edge_probs_last(i)
        assert EP.same(got, [run["edge"][c][i] for c in range(m.n_chains)]), i  # the host model of every chain ...
        assert EP.same(got, [run["per"][c]["edge"][i] for c in range(m.n_chains)]), i  # ... and the fresh one-chain handle


def test_edge_queries_each_group_with_its_own_shape_and_topk(run):
    m, Q = run["m"], run["Q"]
    got = EQ.assert_rows(m, len(Q["eq"]), run["want"]["eq"], 2 * m.n_chains, Q["eq_mult"])
    k = 4 if run["v"] == "tiny" else 10
    for excl in (False, True):
        nodes, sums, t = m.edge_queries_topk(k, exclude_edges=excl)
        for i, q in enumerate(Q["eq"].tolist()):
            first = run["na"] if q < run["na"] else 0
            nbrs = EQ._neighbours(run["rowptr"], run["col"], q) - first if excl else np.zeros(0, dtype=np.int64)
            idx, val = D.numpy_query_topk(got[i]["w_sum"], k, nbrs)
            assert (nodes[i] == np.where(idx == EQ.NONE, EQ.NONE, idx.astype(np.int64) + first)).all() and EP.same(sums[i], val), (excl, i)


def test_conditionals_stats_and_every_chains_last_rows(run):
    m, Q, shapes = run["m"], run["Q"], run["info"]["shapes"]
    CD._check_stats(m.conditionals_stats(), run["want"]["cond"], 2 * m.n_chains)
    for i, v in enumerate(Q["cond"]):
        dS, P = m.conditionals_last(i)
        for c in range(m.n_chains):
            k_own, _, lo = CD._own(int(v), *shapes[c], run["na"])
            assert (dS[c, k_own:] == 0).all() and (P[c, k_own:] == 0).all(), (i, c)
            assert CD._same(dS[c, :k_own], run["per"][c]["dS"][i][:k_own]) and CD._same(P[c, :k_own], run["per"][c]["P"][i][:k_own]), (i, c, shapes[c])
            assert dS[c, int(run["labels"][c][int(v)]) - lo] == 0.0


def test_partition_distances_between_and_to_partitions_of_every_shape(run):
    m, shapes, labs, n = run["m"], run["info"]["shapes"], run["labels"], run["m"].n
    sel = list(range(m.n_chains)) if run["v"] == "tiny" else sorted({shapes.index(s) for s in set(shapes)} | {0, 1, m.n_chains - 1})
    vi, H = m.partition_distances(sel)
    PD._check_against_numpy(m, sel, vi, H, labs={c: labs[c] for c in sel})
    rng = np.random.default_rng(5)
    big = int(np.argmax([a + b for a, b in shapes]))
    small = int(np.argmin([a + b for a, b in shapes]))
    refs = [relabel(labs[big], run["na"], *shapes[big], rng), labs[small], O.contiguous_labels(run["na"], run["nb"], 1, 1), O.contiguous_labels(run["na"], run["nb"], 2, 3)]
    ref_shapes = [shapes[big], shapes[small], (1, 1), (2, 3)]
    to, H_ref = m.partition_distances_to(refs, shapes=ref_shapes)
    assert to.shape == (m.n_chains, 4) and (to >= 0).all()
    for c in range(m.n_chains):
        for g in range(4):
            want = max(numpy_vi(labs[c], refs[g], sum(shapes[c]), sum(ref_shapes[g])), 0.0)
            assert abs(to[c, g] - want) <= vi_tolerance(n, *shapes[c], *ref_shapes[g]), (c, g, to[c, g], want)
    assert to[big, 0] <= vi_tolerance(n, *shapes[big], *shapes[big]) and to[small, 1] <= vi_tolerance(n, *shapes[small], *shapes[small])


@pytest.mark.parametrize("v, entries", [r for r in RUNS if r[1] > 1], ids=lambda p: str(p))
def test_device_entries_behind_one_handle_give_one_handles_chains(v, entries):
    """the sentence of the header -- results are keyed by the global chain id and do not depend on the number of devices or on
    the grouping -- as a test: every entry regroups its own chains, so the groups differ, and every per-chain result is the
    one-entry handle's to the bit; the pooled sums are checked against the host references above, entry by entry"""
    one, many = _run(v, 1), _run(v, entries)
    a, b = one["m"], many["m"]
    assert one["info"]["order"] != many["info"]["order"] and len(many["info"]["order"]) == entries
    assert one["info"]["shapes"] == many["info"]["shapes"] and (one["info"]["acc"] == many["info"]["acc"]).all()
    assert all((x == y).all() for x, y in zip(one["labels"], many["labels"]))
    assert (_bits(a.get_entropy()) == _bits(b.get_entropy())).all() and (a.split_merge_total() == b.split_merge_total()).all()
    assert all(_norm(x) == _norm(y) for x, y in zip(a.split_merge_last(), b.split_merge_last()))
    assert (a.reshuffles_total() == b.reshuffles_total()).all()
    Q = one["Q"]
    for i in range(len(Q["cond"])):
        x, y = a.conditionals_last(i), b.conditionals_last(i)
        assert CD._same(x[0], y[0]) and CD._same(x[1], y[1]), i
    for i in range(len(Q["edits"])):
        assert EP.same(a.edge_probs_last(i), b.edge_probs_last(i)), i
    for i in range(len(Q["virtual"])):
        assert FI._same(a.foldin_posteriors(i), b.foldin_posteriors(i)), i
    s1, t1 = a.pair_scores()
    s2, t2 = b.pair_scores()
    assert t1 == t2 and PS._close(s2, s1, t1)
    assert CO._same(CO._rows(a, len(Q["nodes"]))[0], CO._rows(b, len(Q["nodes"]))[0])
    assert (a.partition_distances()[0] == b.partition_distances()[0]).all()


# ------------------------------------------------------------------ 5. label-indexed sums the caller forgot to reset
STATE = B.BISBM_ERR_STATE


def _one_shape_again(m, shape):
    """every chain to `shape` by moves with k_min = k_max = shape, which refuse every step away from it: all chains share a shape
    again, and the handle is a container still.  At beta = 0.05, where a merge is held back by its Q_rev alone: a chain that is
    three merges away needs some fifty moves (a launch of 48 tiny chains takes a fraction of a millisecond)."""
    for _ in range(2000):
        if not m.mixed_shapes and m.ka_kb(0) == shape:
            break
        m.split_merge(2, 1, 0.05, shape, shape)
    assert not m.mixed_shapes and all(m.ka_kb(c) == shape for c in range(m.n_chains))
    assert (m.KA, m.KB) == shape and len(set(m.chain_groups().tolist())) == 1


def _snapshot(m):
    return [m.get_memberships(c) for c in range(m.n_chains)], m.get_entropy()


def _untouched(m, snap):
    return all((x == y).all() for x, y in zip(snap[0], [m.get_memberships(c) for c in range(m.n_chains)])) and (_bits(snap[1]) == _bits(m.get_entropy())).all()


def _raw_histogram(m):
    """one raw sample of every chain: counts[v][label within the type]"""
    ka, kb = m.ka_kb(0)
    out = np.zeros((m.n, max(ka, kb)), dtype=np.uint32)
    for c in range(m.n_chains):
        lab = m.get_memberships(c).astype(np.int64)
        lab[m.na:] -= ka
        out[np.arange(m.n), lab] += 1
    return out


def test_a_trace_and_a_raw_histogram_the_caller_did_not_reset():
    """include/bisbm.h: bisbm_trace_record is BISBM_ERR_STATE ("bisbm_trace_reset first") when a chain's (ka, kb) differs from
    what its held snapshots were taken with; the histogram is BISBM_ERR_STATE while the chains have different block counts, and
    a histogram of other block counts starts afresh at the next sample -- of other block COUNTS, not of another row length: the
    chains come to 3 + 3 blocks and then to 3 + 2, which share max(ka, kb) and no numbering."""
    m = _handle("tiny")
    kept = {}

    def hook(m):
        m.trace_set(2)
        m.trace_record()
        m.marginals_accumulate()
        kept["counts"] = m.marginals_get()
    _regrouped(m, "tiny", hook)
    assert (kept["counts"] == 0).sum() > 0 and kept["counts"].sum() == m.n_chains * m.n
    snap, raw = _snapshot(m), m._trace_raw()
    same_trace = lambda: all((_bits(x) == _bits(y)).all() if x.dtype == np.float64 else (x == y).all() for x, y in zip(raw[:4], m._trace_raw()[:4])) and m._trace_raw()[4] == raw[4] == 1
    # chains of different shapes
    assert "bisbm_trace_reset first" in _refused(m.trace_record, STATE)
    assert "different block counts" in _refused(m.marginals_accumulate, STATE)
    assert "different block counts" in _refused(m.marginals_get, STATE)
    assert same_trace() and m.trace_series("S").shape == (1, m.n_chains) and _untouched(m, snap)
    # one shape again, the handle a container still
    _one_shape_again(m, (3, 3))
    snap = _snapshot(m)
    assert "bisbm_trace_reset first" in _refused(m.trace_record, STATE)  # (the snapshots are of 3 + 2 blocks)
    _refused(m.marginals_get, STATE)  # (the plain handle's histogram went when the chains were grouped)
    assert same_trace() and _untouched(m, snap)
    m.marginals_accumulate()  # a fresh start: this sample alone
    assert (m.marginals_get() == _raw_histogram(m)).all()
    # ... and on to 3 + 2 blocks: the container's histogram of 3 + 3 blocks has the same row length and another numbering
    _one_shape_again(m, (3, 2))
    assert "3 + 3 then, 3 + 2 now" in _refused(m.marginals_get, STATE)
    assert "present block counts" in _refused(m.marginals_map, STATE)
    m.marginals_accumulate()
    assert (m.marginals_get() == _raw_histogram(m)).all()
    m.trace_reset()
    m.trace_record()
    m.run_sweeps(1)
    m.trace_record()
    lags = m.trace_lags()
    assert lags["records"] == 2 and lags["pairs"].tolist() == [1, 0] and not np.isnan(lags["vi_last"][:, 0]).any()
    m.close()


def _aligned_sample_alone(m, ka, kb):
    """one aligned sample; the histogram and the block sums hold it alone, against a reference taken afresh; returns the perms"""
    n = m.n_chains
    m.marginals_accumulate()
    ref, chain = m.marginals_reference()
    assert chain == int(np.argmin(m.entropy())) and (ref == m.get_memberships(chain)).all()  # the chain of the lowest description length
    perms = [m.marginals_alignment(c)[0] for c in range(n)]
    want = np.zeros((m.n, max(ka, kb)), dtype=np.uint32)
    for c in range(n):
        lab = perms[c][m.get_memberships(c).astype(np.int64)].astype(np.int64)
        lab[m.na:] -= ka
        want[np.arange(m.n), lab] += 1
    assert (m.marginals_get() == want).all()
    model = B.numpy_block_sums(perms, [m.get_m(c)[:ka, ka:] for c in range(n)], [m.get_n_r(c) for c in range(n)], [m.get_m_r(c) for c in range(n)], [0] * n, 1, ka, kb)
    got = m.block_sums()
    assert got["terms"] == n and (got["e"] == model["e"][0]).all() and (got["n"] == model["n"][0]).all() and (got["d"] == model["d"][0]).all()
    return perms


def test_an_aligned_histogram_and_block_summaries_the_caller_did_not_reset():
    """the aligned histogram as the raw one; the block sums live and die with the histogram they accompany: all zero after a
    change of the block counts, then the next sample alone, with a reference taken afresh"""
    m = _handle("tiny")
    m.marginals_set_alignment(B.ALIGN_REFERENCE)
    m.block_sums_set(True, keep_last=True)
    kept = {}

    def hook(m):
        m.marginals_accumulate()
        kept.update(counts=m.marginals_get(), sums=m.block_sums(), ref=m.marginals_reference())
    _regrouped(m, "tiny", hook)
    assert kept["sums"]["terms"] == m.n_chains and kept["counts"].sum() == m.n_chains * m.n
    snap = _snapshot(m)
    assert "different block counts" in _refused(m.marginals_accumulate, STATE)
    assert "different block counts" in _refused(m.marginals_get, STATE)
    assert "different block counts" in _refused(m.block_sums, STATE)
    _refused(lambda: m.block_last(0), STATE)
    assert _untouched(m, snap)
    _one_shape_again(m, (3, 3))
    snap = _snapshot(m)
    z = m.block_sums()
    assert z["terms"] == 0 and not z["e"].any() and not z["n"].any() and not z["d"].any() and z["e"].shape == (3, 3, 3)
    _refused(m.marginals_get, STATE)  # (the plain handle's histogram went when the chains were grouped)
    _refused(lambda: m.block_last(0), STATE)
    perms = _aligned_sample_alone(m, 3, 3)
    _one_shape_again(m, (3, 2))
    z = m.block_sums()
    assert z["terms"] == 0 and not z["e"].any() and not z["n"].any() and not z["d"].any() and z["e"].shape == (3, 3, 2)
    assert "3 + 3 then, 3 + 2 now" in _refused(m.marginals_get, STATE)
    snap = _snapshot(m)
    perms = _aligned_sample_alone(m, 3, 2)
    mode, e, n_r, m_r = m.block_last(5)
    assert mode == 0 and (n_r[perms[5]] == m.get_n_r(5)).all()
    assert _untouched(m, snap)
    m.close()


def test_mode_histograms_the_caller_did_not_reset_are_refused_on_a_container_and_keep_what_they_held():
    """static modes: chains grouped by shape are BISBM_ERR_STATE at the sample, also when every chain is back in the creation
    shape (the handle stays a container); terms and histograms are what they were"""
    m = _handle("tiny")
    m.marginals_set_modes(np.arange(m.n_chains) % 2)
    kept = {}

    def hook(m):
        m.marginals_accumulate()
        kept.update(h0=m.marginals_get(mode=0), h1=m.marginals_get(mode=1))
    _regrouped(m, "tiny", hook)
    snap = _snapshot(m)
    assert "different block counts" in _refused(m.marginals_accumulate, STATE)
    assert "different block counts" in _refused(lambda: m.marginals_get(mode=0), STATE)
    assert m.marginals_modes()["terms"].tolist() == [m.n_chains // 2] * 2 and _untouched(m, snap)
    _one_shape_again(m, (3, 2))
    snap = _snapshot(m)
    assert "grouped by shape" in _refused(m.marginals_accumulate, STATE)
    assert m.marginals_modes()["terms"].tolist() == [m.n_chains // 2] * 2
    assert (m.marginals_get(mode=0) == kept["h0"]).all() and (m.marginals_get(mode=1) == kept["h1"]).all()
    m.marginals_reset()
    assert "grouped by shape" in _refused(lambda: m.marginals_set_modes(np.arange(m.n_chains) % 3), STATE)
    assert _untouched(m, snap)
    m.close()


# ----------------------------------------------------------------------------- 6. the shape term beyond the creation table
def _shape_terms_hex(m):
    return [m.split_merge_shape_term(ka, kb).hex() for ka in range(1, 13) for kb in range(1, 10)]


def test_the_shape_term_beyond_the_creation_table_is_lgamma_whatever_table_the_handle_got():
    """tiny (E = 40, created at 3 + 2): the handle's lgamma table has 2 E + 2 = 82 entries, and lbinom(ka kb + E - 1, E) leaves
    it from ka kb + E >= 82, i.e. from 7 x 6 blocks on, where the library calls lgamma itself.  Every shape up to (12, 9) against
    the same three lbinom terms from math.lgamma: within 2 x WORST of the largest lgamma that enters, WORST = the largest
    relative difference measured (5.24e-16, at 2 + 9 blocks).  And the value does not depend on the handles the process created before: a
    handle made after a larger one may be handed the larger one's cached table (more entries come from the table, fewer from the
    call), so a child process that creates a larger handle first must print the same bits."""
    (rowptr, col), na, nb, ka0, kb0, eps = _case("tiny")
    E = len(col) // 2
    assert E == 40 and 6 * 7 + E + 1 >= 2 * E + 2 > 6 * 6 + E + 1
    m = _handle("tiny", chains=1)
    lb = lambda N, k: 0.0 if (N == 0 or k == 0 or k > N) else (math.lgamma(N + 1) - math.lgamma(k + 1)) - math.lgamma(N - k + 1)
    worst = 0.0
    for ka in range(1, na + 1):
        for kb in range(1, nb + 1):
            want = (lb(ka * kb + E - 1, E) + lb(na - 1, ka - 1)) + lb(nb - 1, kb - 1)
            got = m.split_merge_shape_term(ka, kb)
            scale = math.lgamma(ka * kb + E)  # the largest term
            worst = max(worst, abs(got - want) / scale)
            assert abs(got - want) <= 2 * SHAPE_TERM_WORST * scale, (ka, kb, got, want)
    print("worst |T - T(math.lgamma)| / lgamma(ka kb + E) = %.3e" % worst)
    here = _shape_terms_hex(m)
    m.close()
    # (this process may hold any table by now: one child makes the tiny handle first, one a larger handle before it)
    for first in ("None", "T._handle_of_case('ka1')"):
        code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_after_split_merge as T\n"
                "big = %s; m = T._handle('tiny', chains=1)\n"
                "print(' '.join(T._shape_terms_hex(m)))" % (ROOT, os.path.join(ROOT, "tests"), first))
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert out.stdout.split() == here, first


SHAPE_TERM_WORST = 5.3e-16  # measured: 5.24e-16, at 2 + 9 blocks


def _handle_of_case(name):
    """a handle of 40 + 30 nodes and 300 edges: its 602-entry table is the one a tiny handle made after it is handed"""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    return B.BlockModel(O.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, eps, (rowptr, col), n_chains=1, seed=1)
