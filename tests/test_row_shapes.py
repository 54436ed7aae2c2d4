"""The row-shape graphs of tests/cases.py (row_shape_graph) and the conditions under which tests/test_gpu_row_shapes.py may compare
the device with the oracle on them -- no GPU here, the oracle alone.

  * the graphs are what they claim: one node of every ladder degree per type, concentrated rows whose k_v under the planted
    labels is 255 in one byte, 255 from one edge, 128, and 128 | 127 in two bytes of one counter word, rows of no entries, type sizes
    that are no multiple of 64, and the three ends of col[];
  * the call list of the GPU test (calls(n) below), run on the oracle for chain 0 of every graph, unheld and under the hold of the
    held instances: no accept test of any call lies within a relative 1e-9 of its threshold (orc_last_margin), and every ladder node
    and every concentrated row is accepted into another block and stays where it is at least once each.  The oracle reports no
    per-step verdicts, so the moves are counted sweep by sweep on a second model that runs the constant calls one sweep a call (a
    sweep visits every node once: a label that differs after the sweep is one accepted move, one that does not is a step refused or
    proposed into its own block) and must end every call in the state of the first; the sweeps of the cooling call are those of
    shorter cooling calls from the same state.  pytest -s prints the counts."""
import functools
import math

import numpy as np
import pytest

import cases
import oracle_lib as O

BIG = 1 << 60
SEED = 1234
# (shape, dense) -> the Philox seed of the graph's handles: SEED where chain 0 meets the conditions below with it, unheld and held, else
# the first seed after it that does (found on the host, where the oracle alone runs)
SEEDS = {("8+7", False): 1250, ("16+13", False): 1240, ("16+13", True): 1243, ("20+27", False): 1236, ("20+27", True): 1234,
         ("40+33", False): 1239, ("40+33", True): 1235, ("64+50", False): 1243, ("64+50", True): 1234}
GRAPHS = [(sid, dense) for sid, row in cases.ROW_SHAPES.items() for dense in ((False, True) if row[6] is not None else (False,))]
GRAPH_IDS = ["%s-%s" % (sid, "dense" if dense else "sparse") for sid, dense in GRAPHS]
CONCENTRATED = ("one_block", "copies", "half", "split")


@functools.lru_cache(maxsize=None)
def graph(sid, dense):
    return cases.row_shape_graph(sid, dense)


def calls(n):
    """3 sweeps at T = 1, 4 at T = 30, 4 at T = 1000 (a row of 255 entries hardly moves at T = 1), 2 at T = 1, and the cooling call of
    tests/test_gpu_deep_pass_apply.py: T = 0.9 * 2^(-1200 t / n) is below 2^-1074 before its first sweep ends, the rest is the greedy
    tail with steps_await = n in reach"""
    return [("constant", [1.0], 3 * n, BIG), ("constant", [30.0], 4 * n, BIG), ("constant", [1000.0], 4 * n, BIG), ("constant", [1.0], 2 * n, BIG),
            ("exponential", [0.9, 0.5 ** (1200.0 / n)], 3 * n, n)]


def held_node(g):
    """the node the held instances clamp: the first plain node of type a"""
    special = set(g["special"][0].values())
    return next(v for v in range(g["na"]) if v not in special)


def oracle_model(g, held, seed, planted=False):
    """chain 0 at the device's start: shuffle_bisbm from the planted labels (planted: init_bisbm, the planted labels themselves);
    held: then one clamped plain node and a table of one class that allows every block"""
    o = O.OracleModel(g["rowptr"], g["col"], g["na"], g["nb"], g["ka"], g["kb"], 1.0, g["labels"])
    o.seed_philox(seed, 0)
    if planted:
        o.init_bisbm()
    else:
        o.shuffle_bisbm()
    if held:
        mask = np.zeros(g["na"] + g["nb"], dtype=bool)
        mask[held_node(g)] = True
        o.clamp(mask)
        o.constrain(np.zeros(g["na"] + g["nb"], dtype=np.uint8), np.ones((1, g["ka"] + g["kb"]), dtype=np.uint8))
    return o


def _state(o):
    return o.memberships(), o.m(), o.m_r(), o.n_r(), o.eta()


@functools.lru_cache(maxsize=None)
def reference(sid, dense, held, seed=None, planted=False):
    """chain 0 of the oracle after every call of calls(n): state, return value, counts, running sum, S and the call's smallest margin;
    and per node the number of sweeps in which it moved / stayed"""
    g = graph(sid, dense)
    n = g["na"] + g["nb"]
    seed = SEEDS[(sid, dense)] if seed is None else seed
    o, step = oracle_model(g, held, seed, planted), oracle_model(g, held, seed, planted)
    out, moved, stayed = [], np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)

    def count(before, after):
        moved[:] += after != before
        stayed[:] += after == before
        return after

    for j, (sched, kw, dur, wait) in enumerate(calls(n)):
        before = step.memberships()
        rate = o.anneal(sched, kw, dur, wait)
        out.append(dict(rate=rate, acc=o.last_accepted, sweeps=o.last_sweeps, cum=o.get_entropy(), entropy=o.entropy(), margin=o.last_margin,
                        state=_state(o)))
        if sched == "constant":
            for _ in range(dur // n):
                step.anneal(sched, kw, n, wait)
                before = count(before, step.memberships())
        else:  # the cooling call keeps its books from sweep to sweep: its first k sweeps are the call of k sweeps from the same state
            for k in range(1, out[-1]["sweeps"]):
                part = oracle_model(g, held, seed, planted)
                for c in calls(n)[:j]:
                    part.anneal(*c)
                part.anneal(sched, kw, k * n, wait)
                assert part.last_sweeps == k
                before = count(before, part.memberships())
            step.anneal(sched, kw, dur, wait)
            count(before, step.memberships())
        for a, b in zip(out[-1]["state"], _state(step)):
            assert (a == b).all(), (sid, dense, held, sched, "a call cut into sweeps is another chain")
    return out, moved, stayed


# --------------------------------------------------------------------------------------------------------------- the graphs
@pytest.mark.parametrize("sid,dense", GRAPHS, ids=GRAPH_IDS)
def test_rows_have_the_stated_degrees_and_the_concentrated_k_v(sid, dense):
    g = graph(sid, dense)
    na, nb, ka, kb = g["na"], g["nb"], g["ka"], g["kb"]
    n = na + nb
    assert na % 64 != 0 and nb % 64 != 0 and n < 2500
    deg = np.diff(g["rowptr"].astype(np.int64))
    assert len(g["col"]) == int(g["rowptr"][-1]) and len(deg) == n
    assert (g["col"][:int(g["rowptr"][na])] >= na).all() and (g["col"][int(g["rowptr"][na]):] < na).all()  # bipartite
    assert g["ladder"] == (cases.ROW_LADDER if not dense else tuple(d for d in cases.ROW_LADDER if d <= 255))
    assert int(deg.max()) == (255 if dense else 300)
    special = set()
    for t in (0, 1):
        sp = g["special"][t]
        special |= set(sp.values())
        for d in g["ladder"]:
            assert deg[sp["ladder%d" % d]] == d, (t, d)
        for i in range(cases.ROW_ISOLATED):
            assert deg[sp["isolated%d" % i]] == 0
        k_oth = kb if t == 0 else ka
        want = {"one_block": {k_oth - 1: 255}, "half": {2: 128}, "split": {4: 128, 5: 127}, "copies": {int(g["labels"][g["special"][1 - t]["copies"]]) - (ka if t == 0 else 0): 255}}
        for name, blocks in want.items():
            k_v = cases.row_k_v(g, sp[name])
            assert {int(b): int(k_v[b]) for b in np.flatnonzero(k_v)} == blocks, (t, name, k_v)
            assert deg[sp[name]] == sum(blocks.values())
        row = g["col"][int(g["rowptr"][sp["copies"]]):int(g["rowptr"][sp["copies"] + 1])]
        assert (row == g["special"][1 - t]["copies"]).all()
        assert all(t == (v >= na) for v in sp.values())
    # (4 and 5 lie in one word of the byte counters, four consecutive blocks of the other type to a word)
    assert 4 // 4 == 5 // 4
    # every other special row ends in plain nodes, and no two special nodes are neighbours in the ids
    for t in (0, 1):
        for name, v in g["special"][t].items():
            if name != "copies":
                assert not special & set(g["col"][int(g["rowptr"][v]):int(g["rowptr"][v + 1])].tolist()), (t, name)
    banded = {v for t in (0, 1) for name, v in g["special"][t].items() if name.startswith("band")}
    ids = sorted(special - {n - 1, n - 2} - banded)
    assert min(np.diff(ids)) >= 2
    assert len(banded) == (2 * len(cases.ROW_BAND) if (sid, dense) == ("20+27", False) else 0)
    for t in (0, 1):  # the band: side by side in the ids, each row in one block
        rows = [g["special"][t]["band%d" % d] for d in cases.ROW_BAND if banded]
        assert list(np.diff(rows)) == [1] * (len(rows) - 1 if rows else 0)
        for v, d in zip(rows, cases.ROW_BAND):
            assert deg[v] == d and cases.row_k_v(g, v)[3] == d
    # every planted block keeps plain nodes
    plain = np.setdiff1d(np.arange(n), np.array(sorted(special)))
    assert (np.bincount(g["labels"][plain], minlength=ka + kb) >= 4).all()
    # the end of col[]: the node with the highest id
    assert g["special"][1]["end"] == n - 1 and deg[n - 1] == int(g["end"]) and int(g["rowptr"][n]) == len(g["col"])
    if g["end"] == "255":
        assert g["special"][1]["before_end"] == n - 2 and deg[n - 2] == 2
    print(sid, "dense" if dense else "sparse", "nodes %d + %d, adjacency entries %d, plain degrees %d..%d (mean %.1f)"
          % (na, nb, len(g["col"]), deg[plain].min(), deg[plain].max(), deg[plain].mean()))


def test_every_end_of_col_occurs():
    """a last row of 255 entries behind one of 2 on every shape but 16 + 13 (where the kernel keeps a window of eta: in the graph whose
    window ends at 255), last rows of 1 and of 3 entries on 16 + 13 and beside the former"""
    ends = {(sid, dense): graph(sid, dense)["end"] for sid, dense in GRAPHS}
    assert set(ends.values()) == {"1", "3", "255"}
    assert (ends[("16+13", False)], ends[("16+13", True)]) == ("1", "3")
    for sid in cases.ROW_SHAPES:
        if sid != "16+13":
            assert ends[(sid, cases.ROW_SHAPES[sid][6] is not None)] == "255", sid


# ------------------------------------------------------------------------------------------- the conditions on the inputs
@pytest.mark.parametrize("held", [False, True], ids=["unheld", "held"])
@pytest.mark.parametrize("sid,dense", GRAPHS, ids=GRAPH_IDS)
def test_the_call_list_moves_and_refuses_every_row_and_decides_no_step_by_a_hair(sid, dense, held):
    g = graph(sid, dense)
    n = g["na"] + g["nb"]
    assert sum(c[2] for c in calls(n)) // n < 20
    ref, moved, stayed = reference(sid, dense, held)
    margin = min(r["margin"] for r in ref)
    rows = cases.row_shape_rows(g)
    lines = ["%s%s %d: moved %d, stayed %d" % ("ab"[t], name, d, moved[v], stayed[v]) for t, name, v, d in rows]
    print("%s %s %s: smallest margin %.3g; accepted per call %s, sweeps %s\n  " % (sid, "dense" if dense else "sparse", "held" if held else "unheld", margin,
                                                                                [r["acc"] for r in ref], [r["sweeps"] for r in ref]) + "; ".join(lines))
    for i, r in enumerate(ref):
        assert r["margin"] > 1e-9, (sid, dense, held, i, r["margin"], "an accept test too close to its threshold: another seed")
    assert math.isfinite(margin)
    for t, name, v, d in rows:
        assert moved[v] >= (2 if name in CONCENTRATED else 1) and stayed[v] >= 1, (sid, dense, held, name, "ab"[t], int(moved[v]), int(stayed[v]))
    if held:
        assert moved[held_node(g)] == 0


@pytest.mark.parametrize("sid,dense", GRAPHS, ids=GRAPH_IDS)
def test_the_planted_start_meets_the_concentrated_rows_at_their_extremes(sid, dense):
    """shuffle_bisbm spreads a concentrated row's neighbours over the blocks (only the 255 copies of one edge stay in one byte), so the
    GPU test runs two routes from the planted labels as well: there the rows have the k_v checked above when the first sweep visits
    them, and most of them in the first hot sweep still.  The same margin condition; the counts are printed."""
    g = graph(sid, dense)
    ref, moved, stayed = reference(sid, dense, False, planted=True)
    for i, r in enumerate(ref):
        assert r["margin"] > 1e-9, (sid, dense, i, r["margin"], "an accept test too close to its threshold: another seed")
    rows = [(t, name, v) for t, name, v, d in cases.row_shape_rows(g) if name in CONCENTRATED]
    print(sid, "dense" if dense else "sparse", "planted start: smallest margin %.3g; accepted per call %s; " % (min(r["margin"] for r in ref), [r["acc"] for r in ref])
          + "; ".join("%s%s moved %d" % ("ab"[t], name, moved[v]) for t, name, v in rows))
    # (the largest byte of every concentrated row after the three sweeps at T = 1: the planted structure mostly stands)
    print("  largest k_v byte after the first call:", [int(cases.row_k_v(g, v, ref[0]["state"][0]).max()) for t, name, v in rows])
